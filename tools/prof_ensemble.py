"""Times M models' losses and gradients as M consecutive loss_and_grad calls against ONE loss_and_grad_many, on the reference's
README network (2-6-2) and its regression network (16-48-16) over tspan (0, 13) at its batch_size of 32, README tolerances.

    python tools/prof_ensemble.py --parent-lib /path/to/libcnfhip.so [--rounds 2] [--window 0.5] [--out profiles/ensemble_timing.txt]

One child process per leg, started in alternation by this script (CNFHIP_LIB is read at import; a fresh child each time -- never
an exec over a process that has opened the GPU), in the manner of tools/prof_vjp.py.  Legs, in the order of every round:

    parent-a   M consecutive loss_and_grad calls (each member's own parameters, data, probes) with the parent build    (i)
    new        the same calls with this build                                                                           (ii)
    parent-b   the parent build again                                                                                   (i'): the spread
    many       one loss_and_grad_many of the M members                                                                  (iii)

for M in {1, 8, 64, ensemble_capacity}.  Every (shape, M) is warmed up, then timed over at least `--window` seconds with device
events around synchronised work; the figure is ms per pass over the M members.  (ii) / (i) must lie inside the spread (i') / (i):
the existing calls are the parent's code.  The `parent` and `new` legs also hash the loss and gradient of one loss_and_grad of the
16-48-16 and 16-64-16 networks: the two builds must agree bit for bit.  Without --parent-lib only `new` and `many` run.
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
B = 32
TSPAN = (0.0, 13.0)
MS = (1, 8, 64, "capacity")


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
    per.sort()
    return dict(ms=total / len(per), median=per[len(per) // 2], lo=per[0], hi=per[-1], n=len(per))


def _model(cnf, dims, nvars, naugs):
    nn = cnf.Chain(cnf.Dense(dims[0], dims[1], "tanh"), cnf.Dense(dims[1], dims[2], "tanh"))
    return cnf.construct(cnf.RNODE, nn, nvars, naugs, compute_mode=cnf.HIPVecJacMatrixMode(), tspan=TSPAN, lambda3=1e-2, rng=1)


def child(leg, window, capacities):
    import numpy as np
    import torch
    from continuousnf.jl_amd import _lib
    if leg.startswith("parent"):                     # (an earlier build does not export the entry points added since)
        import ctypes
        l = ctypes.CDLL(_lib.LIB_PATH)
        for table in (_lib._SIGNATURES, _lib._SAMPLING_SIGNATURES, _lib._BASEGRAD_SIGNATURES, _lib._ENSEMBLE_SIGNATURES):
            for name in list(table):
                if not hasattr(l, name):
                    table.pop(name)
    import continuousnf.jl_amd as cnf
    out = {"leg": leg, "lib": _lib.LIB_PATH, "shapes": {}, "capacity": {}, "bits": {}}
    T = cnf.TrainMode()
    for name, dims, nvars, naugs in SHAPES:
        icnf = _model(cnf, dims, nvars, naugs)
        cap = capacities.get(name) or cnf.ensemble_capacity(icnf, T, B)
        out["capacity"][name] = cap
        rng = np.random.default_rng(7)
        n_in, n_params = nvars + naugs, icnf.nn.n_params_internal
        Mmax = max(cap, 64)
        lim = np.sqrt(6.0 / (dims[0] + dims[1]))
        ps = torch.from_numpy(rng.uniform(-lim, lim, size=(Mmax, n_params)).astype(np.float32)).cuda()
        xs = torch.from_numpy(rng.beta(2.0, 4.0, size=(Mmax, nvars, B)).astype(np.float32)).cuda()
        eps = torch.from_numpy(rng.standard_normal((Mmax, n_in, B)).astype(np.float32)).cuda()
        for M in MS:
            Mv = cap if M == "capacity" else M
            if leg == "many":
                fn = lambda: cnf.loss_and_grad_many(icnf, T, xs[:Mv], ps[:Mv], {}, eps=eps[:Mv])
            else:
                def fn():
                    for m in range(Mv):
                        cnf.loss_and_grad(icnf, T, xs[m], ps[m], {}, eps=eps[m])
            out["shapes"][f"{name} M={M}"] = dict(_timed(fn, window, 3 if Mv <= 64 else 1), M=Mv)
        icnf.close()
    if leg != "many":
        for dims in ((16, 48, 16), (16, 64, 16)):
            icnf = _model(cnf, dims, 8, 8)
            rng = np.random.default_rng(9)
            lim = np.sqrt(6.0 / (dims[0] + dims[1]))
            p = rng.uniform(-lim, lim, size=icnf.nn.n_params_internal).astype(np.float32)
            x = torch.from_numpy(rng.standard_normal((8, 33)).astype(np.float32)).cuda()
            e = torch.from_numpy(rng.standard_normal((16, 33)).astype(np.float32)).cuda()
            val, g = cnf.loss_and_grad(icnf, T, x, p, {}, eps=e)
            out["bits"]["-".join(map(str, dims))] = hashlib.sha256(np.float32(val).tobytes() + g.cpu().numpy().tobytes()).hexdigest()[:16]
            icnf.close()
    print("PROF_ENS " + json.dumps(out), flush=True)


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
    line = [l for l in r.stdout.splitlines() if l.startswith("PROF_ENS ")][-1]
    return json.loads(line[len("PROF_ENS "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out")
    ap.add_argument("--child")
    ap.add_argument("--capacities", default="{}")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.window, json.loads(a.capacities))
    legs = ["parent-a", "new", "parent-b", "many"] if a.parent_lib else ["new", "many"]
    res = {l: {} for l in legs}
    caps, bits = {}, {}
    # the parent build cannot say the capacity: this build's `many` leg is asked first, untimed figures dropped
    caps = run_child("many", None, 0.01, {})["capacity"]
    for _ in range(a.rounds):
        for leg in legs:                             # the legs alternate: one child each, one at a time
            out = run_child(leg, a.parent_lib if leg.startswith("parent") else None, a.window, caps)
            for shape, v in out["shapes"].items():
                res[leg].setdefault(shape, []).append(v["ms"])
            for k, v in out["bits"].items():
                bits.setdefault(k, {}).setdefault("parent" if leg.startswith("parent") else "new", set()).add(v)
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])
    lines = [f"# tools/prof_ensemble.py: ms per pass over M members (B = {B}, tspan {TSPAN}, README tolerances), {a.rounds} rounds, "
             f"window {a.window} s per leg, shape and M; all rounds listed",
             "# capacity (cnf_ensemble_capacity, TrainMode, B = 32): " + ", ".join(f"{k}: {v}" for k, v in caps.items())]
    for name, *_ in SHAPES:
        for M in MS:
            key = f"{name} M={M}"
            row = {l: res[l].get(key, []) for l in legs}
            Mv = caps[name] if M == "capacity" else M
            s = f"{name} M={Mv}: " + "; ".join(f"{l} {med(v):.3f} ({', '.join(f'{x:.3f}' for x in v)})" for l, v in row.items() if v)
            if a.parent_lib:
                pa, pb, nw = med(row["parent-a"]), med(row["parent-b"]), med(row["new"])
                s += f" | new/parent {nw / (0.5 * (pa + pb)):.4f}, parent-b/parent-a {pb / pa:.4f}"
            s += f" | many/new {med(row['many']) / med(row['new']):.4f}, ms per member: new {med(row['new']) / Mv:.4f}, many {med(row['many']) / Mv:.4f}"
            lines.append(s)
    for k, v in bits.items():
        if "parent" in v:
            same = len(v["parent"]) == 1 and v["parent"] == v["new"]
            lines.append(f"loss_and_grad {k} B=33, parent build vs this build: {'bit-identical' if same else 'DIFFERENT'} "
                         f"({sorted(v['parent'])} / {sorted(v['new'])})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
