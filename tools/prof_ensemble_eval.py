"""Times scoring and sampling M models as M consecutive inference / generate calls against ONE inference_many / generate_many, on
the reference's README network (2-6-2) and its regression network (16-48-16) over tspan (0, 13), README tolerances, TrainMode and
TestMode, at B = 32 and B = 256, with the data already on the device.

    python tools/prof_ensemble_eval.py --parent-lib /path/to/libcnfhip.so [--rounds 2] [--window 0.3] [--out profiles/ensemble_eval_timing.txt]

One child process per leg, started in alternation by this script (CNFHIP_LIB is read at import; a fresh child each time -- never
an exec over a process that has opened the GPU), in the manner of tools/prof_ensemble.py.  Legs, in the order of every round:

    parent   M consecutive inference (generate) calls, each member's own parameters, data and probes, with the parent build  (i)
    new      the same calls with this build                                                                                 (ii)
    many     one inference_many (generate_many) of the M members                                                            (iii)

for M in {1, 2, 64, ensemble_eval_capacity}.  Every (operation, shape, mode, B, M) is warmed up, then timed over at least
`--window` seconds with device events around synchronised work; a sample is the ms of one pass over the M members, and the file
gives the median and the interquartile range of the samples of all rounds.  The parent has no other way to compute this than
(i).  Beside many / loop the file gives many(M) / loop(M = 1): what M members cost in units of ONE member's single call (the
gradient form's figure is 1.1-1.2 at M = 64: profiles/ensemble_timing.txt).  The `parent` and `new` legs also hash one
inference of the 16-48-16 and 16-64-16 networks: the two builds must agree bit for bit.  Without --parent-lib only `new` and
`many` run.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = (("README 2-6-2", (2, 6, 2), 1, 1), ("regression 16-48-16", (16, 48, 16), 8, 8))
BS = (32, 256)
TSPAN = (0.0, 13.0)
MS = (1, 2, 64, "capacity")
OPS = ("inference", "generate")
KEEP = 400                                           # samples a child reports per figure


def _timed(fn, window, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    total, per = 0.0, []
    while total < window * 1e3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b))
        total += per[-1]
    return per[:KEEP]


def _model(cnf, dims, nvars, naugs):
    nn = cnf.Chain(cnf.Dense(dims[0], dims[1], "tanh"), cnf.Dense(dims[1], dims[2], "tanh"))
    return cnf.construct(cnf.RNODE, nn, nvars, naugs, compute_mode=cnf.HIPVecJacMatrixMode(), tspan=TSPAN, lambda3=1e-2, rng=1)


def child(leg, window, capacities):
    import numpy as np
    import torch
    from continuousnf.jl_amd import _lib
    if leg == "parent":                              # (an earlier build does not export the entry points added since)
        import ctypes
        l = ctypes.CDLL(_lib.LIB_PATH)
        for table in (_lib._SIGNATURES, _lib._SAMPLING_SIGNATURES, _lib._BASEGRAD_SIGNATURES, _lib._ENSEMBLE_SIGNATURES,
                      _lib._ENSEMBLE_EVAL_SIGNATURES):
            for name in list(table):
                if not hasattr(l, name):
                    table.pop(name)
    import continuousnf.jl_amd as cnf
    out = {"leg": leg, "lib": _lib.LIB_PATH, "samples": {}, "capacity": {}, "bits": {}}
    for name, dims, nvars, naugs in SHAPES:
        icnf = _model(cnf, dims, nvars, naugs)
        n_in, n_params = nvars + naugs, icnf.nn.n_params_internal
        lim = np.sqrt(6.0 / (dims[0] + dims[1]))
        for B in BS:
            for mode_name, mode in (("train", cnf.TrainMode()), ("test", cnf.TestMode())):
                key = f"{name} {mode_name} B={B}"
                cap = capacities.get(key) or cnf.ensemble_eval_capacity(icnf, mode, B)
                out["capacity"][key] = cap
                rng = np.random.default_rng(7)
                Mmax = max(cap, 64)
                dev = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
                ps = dev(rng.uniform(-lim, lim, size=(Mmax, n_params)))
                xs = dev(rng.beta(2.0, 4.0, size=(Mmax, nvars, B)))
                z0 = dev(rng.standard_normal((Mmax, n_in, B)))
                eps = dev(rng.standard_normal((Mmax, n_in, B)))
                train = mode_name == "train"
                for op in OPS:
                    for M in MS:
                        Mv = cap if M == "capacity" else M
                        if leg == "many" and op == "inference":
                            fn = lambda: cnf.inference_many(icnf, mode, xs[:Mv], ps[:Mv], {}, eps=eps[:Mv] if train else None)
                        elif leg == "many":
                            fn = lambda: cnf.generate_many(icnf, mode, ps[:Mv], {}, B, z0=z0[:Mv], eps=eps[:Mv])
                        elif op == "inference":
                            def fn():
                                for m in range(Mv):
                                    cnf.inference(icnf, mode, xs[m], ps[m], {}, **(dict(eps=eps[m]) if train else {}))
                        else:
                            def fn():
                                for m in range(Mv):
                                    cnf.generate(icnf, mode, ps[m], {}, B, z0=z0[m], eps=eps[m])
                        out["samples"][f"{op} {key} M={M}"] = dict(ms=_timed(fn, window, 3 if Mv <= 64 else 1), M=Mv)
        icnf.close()
    if leg != "many":
        for dims in ((16, 48, 16), (16, 64, 16)):
            icnf = _model(cnf, dims, 8, 8)
            rng = np.random.default_rng(9)
            lim = np.sqrt(6.0 / (dims[0] + dims[1]))
            p = rng.uniform(-lim, lim, size=icnf.nn.n_params_internal).astype(np.float32)
            x = torch.from_numpy(rng.standard_normal((8, 80)).astype(np.float32)).cuda()
            e = torch.from_numpy(rng.standard_normal((16, 80)).astype(np.float32)).cuda()
            lp, regs = cnf.inference(icnf, cnf.TrainMode(), x, p, {}, eps=e)
            g = cnf.generate(icnf, cnf.TrainMode(), p, {}, 80, z0=e, eps=e)
            h = hashlib.sha256(lp.cpu().numpy().tobytes() + b"".join(r.cpu().numpy().tobytes() for r in regs) + g.contiguous().cpu().numpy().tobytes())
            out["bits"]["-".join(map(str, dims))] = h.hexdigest()[:16]
            icnf.close()
    print("PROF_ENS_EVAL " + json.dumps(out), flush=True)


def run_child(leg, lib, window, capacities):
    env = dict(os.environ)
    if lib:
        env["CNFHIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("CNFHIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--window", str(window),
                        "--capacities", json.dumps(capacities)], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"child {leg} ended with status {r.returncode}")
    line = [l for l in r.stdout.splitlines() if l.startswith("PROF_ENS_EVAL ")][-1]
    return json.loads(line[len("PROF_ENS_EVAL "):])


def _quartiles(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, max(0, int(round(p * (len(v) - 1)))))]
    return q(0.5), q(0.25), q(0.75)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out")
    ap.add_argument("--child")
    ap.add_argument("--capacities", default="{}")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.window, json.loads(a.capacities))
    legs = ["parent", "new", "many"] if a.parent_lib else ["new", "many"]
    loop = legs[0]                                   # what the ensemble call is compared with: the parent's loop when there is one
    res = {l: {} for l in legs}
    bits = {}
    # the parent build cannot say the capacity: this build is asked first, its untimed figures dropped
    caps = run_child("many", None, 0.001, {})["capacity"]
    for _ in range(a.rounds):
        for leg in legs:                             # the legs alternate: one child each, one at a time
            out = run_child(leg, a.parent_lib if leg == "parent" else None, a.window, caps)
            for key, v in out["samples"].items():
                res[leg].setdefault(key, []).extend(v["ms"])
            for k, v in out["bits"].items():
                bits.setdefault(k, {}).setdefault(leg, set()).add(v)
    lines = [f"# tools/prof_ensemble_eval.py: ms per pass over M members (tspan {TSPAN}, README tolerances), median [IQR] (samples) over "
             f"{a.rounds} rounds, window {a.window} s per leg and figure",
             f"# loop = M consecutive single calls ({'parent build' if a.parent_lib else 'this build'}); many = one ensemble call; "
             "many/one = many(M) / loop(M = 1)",
             "# capacity (cnf_ensemble_eval_capacity): " + ", ".join(f"{k}: {v}" for k, v in caps.items())]
    slower = []
    for op in OPS:
        for name, *_ in SHAPES:
            for B in BS:
                for mode_name in ("train", "test"):
                    key = f"{name} {mode_name} B={B}"
                    one = _quartiles(res[loop][f"{op} {key} M=1"])[0]
                    for M in MS:
                        k = f"{op} {key} M={M}"
                        Mv = caps[key] if M == "capacity" else M
                        fmt = lambda v: "{:.3f} [{:.3f}, {:.3f}] ({})".format(*_quartiles(v), len(v))
                        s = f"{op} {key} M={Mv}: " + "; ".join(f"{'loop' if l == loop else l} {fmt(res[l][k])}" for l in legs)
                        lm, mm = _quartiles(res[loop][k])[0], _quartiles(res["many"][k])[0]
                        s += f" | many/loop {mm / lm:.4f}, many/one {mm / one:.3f}, ms per member: loop {lm / Mv:.4f}, many {mm / Mv:.4f}"
                        if a.parent_lib:
                            s += f", new/parent loop {_quartiles(res['new'][k])[0] / lm:.4f}"
                        if Mv >= 2 and mm > lm:
                            slower.append(k)
                        lines.append(s)
    lines.append("ensemble call slower than the loop at M >= 2: " + (", ".join(slower) if slower else "nowhere"))
    for k, v in bits.items():
        if "parent" in v:
            same = len(v["parent"]) == 1 and v["parent"] == v["new"]
            lines.append(f"inference + generate {k} B=80, parent build vs this build: {'bit-identical' if same else 'DIFFERENT'} "
                         f"({sorted(v['parent'])} / {sorted(v['new'])})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
