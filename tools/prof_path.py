"""Times flow paths (solve_path) against the solve without a path and against what a user did before -- K chained base_sol calls
over the sub-spans --, and checks that the calls that existed before cost what they did: on the reference's README network (2-6-2)
and its regression network (16-48-16) over tspan (0, 13), README tolerances, TrainMode, at B = 32 and B = 4096, data on the device;
and the streamed route on the headline network (32-128-128-32, tspan (0, 1)) at B = 1024 against inference.

    python tools/prof_path.py [--parent-lib /path/to/libcnfhip.so] [--rounds 2] [--window 0.3] [--out profiles/path_timing.txt]

One child process per leg, started in alternation by this script (CNFHIP_LIB is read at import; a fresh child each time -- never
an exec over a process that has opened the GPU), in the manner of tools/prof_ensemble_eval.py.  Legs of every round:

    parent   inference and loss_and_grad of the wave-kernel shapes with the parent build
    new      the same calls with this build; base_sol; solve_path with K = 1, 16, 256 equally spaced save times; K chained base_sol
             calls; the headline network's inference and streamed solve_path (K = 16)

Every figure is warmed up, then timed over at least `--window` seconds with device events around synchronised work; the file gives
the median and the interquartile range of the samples of all rounds.  Both legs hash one inference of each wave shape: the two
builds must agree bit for bit.
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
BS = (32, 4096)
TSPAN = (0.0, 13.0)
KS = (1, 16, 256)
KEEP = 400


def _timed(fn, window, warm=3):
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


def _model(cnf, dims, nvars, naugs, tspan=TSPAN, lam3=1e-2):
    nn = cnf.Chain(*[cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])])
    return cnf.construct(cnf.RNODE, nn, nvars, naugs, compute_mode=cnf.HIPVecJacMatrixMode(), tspan=tspan, lambda3=lam3, rng=1)


def child(leg, window):
    import numpy as np
    import torch
    from continuousnf.jl_amd import _lib
    if leg == "parent":                              # (an earlier build does not export the entry points added since)
        import ctypes
        l = ctypes.CDLL(_lib.LIB_PATH)
        for table in (_lib._SIGNATURES, _lib._SAMPLING_SIGNATURES, _lib._BASEGRAD_SIGNATURES, _lib._ENSEMBLE_SIGNATURES,
                      _lib._ENSEMBLE_EVAL_SIGNATURES, _lib._PATH_SIGNATURES):
            for name in list(table):
                if not hasattr(l, name):
                    table.pop(name)
    import continuousnf.jl_amd as cnf
    out = {"leg": leg, "lib": _lib.LIB_PATH, "samples": {}, "bits": {}, "launches": {}}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    mode = cnf.TrainMode()

    def params(icnf, dims, rng):
        lim = np.sqrt(6.0 / (dims[0] + dims[1]))
        return rng.uniform(-lim, lim, size=icnf.nn.n_params_internal).astype(np.float32)

    for name, dims, nvars, naugs in SHAPES:
        icnf = _model(cnf, dims, nvars, naugs)
        n_in = nvars + naugs
        for B in BS:
            key = f"{name} B={B}"
            rng = np.random.default_rng(7)
            ps = params(icnf, dims, rng)
            xs, eps = dev(rng.beta(2.0, 4.0, size=(nvars, B))), dev(rng.standard_normal((n_in, B)))
            out["samples"][f"inference {key}"] = _timed(lambda: cnf.inference(icnf, mode, xs, ps, {}, eps=eps), window)
            out["samples"][f"loss_and_grad {key}"] = _timed(lambda: cnf.loss_and_grad(icnf, mode, xs, ps, {}, eps=eps), window)
            lp, regs = cnf.inference(icnf, mode, xs, ps, {}, eps=eps)
            out["bits"][key] = hashlib.sha256(lp.cpu().numpy().tobytes() + b"".join(r.cpu().numpy().tobytes() for r in regs)).hexdigest()[:16]
            if leg == "parent":
                continue
            prob = cnf.inference_prob(icnf, mode, xs, ps, {}, eps=eps)
            out["samples"][f"base_sol {key}"] = _timed(lambda: cnf.base_sol(icnf, prob), window)
            out["launches"][f"base_sol {key}"] = prob.stats["launches"]
            for K in KS:
                saveat = np.linspace(TSPAN[0], TSPAN[1], K + 1)[1:]
                out["samples"][f"solve_path K={K} {key}"] = _timed(lambda: cnf.solve_path(icnf, prob, saveat), window)
                out["launches"][f"solve_path K={K} {key}"] = prob.stats["launches"]
                if K == 1:
                    continue
                edges = [TSPAN[0]] + [float(s) for s in saveat]

                def chain():
                    u = prob.u0
                    for a, b in zip(edges[:-1], edges[1:]):
                        u = cnf.base_sol(icnf, cnf.ODEProblem(icnf, mode, u, prob.eps, (a, b), ps))
                out["samples"][f"chained base_sol K={K} {key}"] = _timed(chain, window, 1)
        icnf.close()
    if leg != "parent":
        dims, B = (32, 128, 128, 32), 1024
        icnf = _model(cnf, dims, 32, 0, (0.0, 1.0), 0.0)
        rng = np.random.default_rng(11)
        ps = params(icnf, dims, rng)
        xs, eps = dev(rng.beta(2.0, 4.0, size=(32, B))), dev(rng.standard_normal((32, B)))
        key = f"headline 32-128-128-32 B={B}"
        out["samples"][f"inference {key}"] = _timed(lambda: cnf.inference(icnf, mode, xs, ps, {}, eps=eps), window)
        out["launches"][f"inference {key}"] = icnf.last_stats["launches"]
        prob = cnf.inference_prob(icnf, mode, xs, ps, {}, eps=eps)
        saveat = np.linspace(0.0, 1.0, 17)[1:]
        out["samples"][f"solve_path K=16 {key}"] = _timed(lambda: cnf.solve_path(icnf, prob, saveat), window, 1)
        out["launches"][f"solve_path K=16 {key}"] = prob.stats["launches"]
        icnf.close()
    print("PROF_PATH " + json.dumps(out), flush=True)


def run_child(leg, lib, window):
    env = dict(os.environ)
    if lib:
        env["CNFHIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("CNFHIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--window", str(window)], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"child {leg} ended with status {r.returncode}")
    line = [l for l in r.stdout.splitlines() if l.startswith("PROF_PATH ")][-1]
    return json.loads(line[len("PROF_PATH "):])


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
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.window)
    legs = ["parent", "new"] if a.parent_lib else ["new"]
    res = {l: {} for l in legs}
    bits, launches = {}, {}
    for _ in range(a.rounds):
        for leg in legs:                             # the legs alternate: one child each, one at a time
            out = run_child(leg, a.parent_lib if leg == "parent" else None, a.window)
            for key, v in out["samples"].items():
                res[leg].setdefault(key, []).extend(v)
            for k, v in out["bits"].items():
                bits.setdefault(k, {}).setdefault(leg, set()).add(v)
            launches.update(out["launches"])
    fmt = lambda v: "{:.3f} [{:.3f}, {:.3f}] ({})".format(*_quartiles(v), len(v))
    med = lambda k: _quartiles(res["new"][k])[0]
    lines = [f"# tools/prof_path.py: ms per call, median [IQR] (samples) over {a.rounds} rounds, window {a.window} s per figure; TrainMode (VJP), "
             f"README tolerances; wave shapes over tspan {TSPAN}, the headline network over (0, 1)"]
    for name, *_ in SHAPES:
        for B in BS:
            key = f"{name} B={B}"
            base = med(f"base_sol {key}")
            lines.append(f"base_sol {key}: {fmt(res['new'][f'base_sol {key}'])}, {launches[f'base_sol {key}']} launch(es)")
            for K in KS:
                k = f"solve_path K={K} {key}"
                s = f"{k}: {fmt(res['new'][k])}, {launches[k]} launch(es) | path/base_sol {med(k) / base:.3f}"
                if K > 1:
                    ck = f"chained base_sol K={K} {key}"
                    s += f" | {K} chained base_sol {fmt(res['new'][ck])}, chained/path {med(ck) / med(k):.1f}"
                lines.append(s)
    hk = "headline 32-128-128-32 B=1024"
    lines.append(f"inference {hk}: {fmt(res['new'][f'inference {hk}'])}, {launches[f'inference {hk}']} launch(es)")
    pk = f"solve_path K=16 {hk}"
    lines.append(f"{pk} (streamed): {fmt(res['new'][pk])}, {launches[pk]} launches | path/inference {med(pk) / med(f'inference {hk}'):.1f}")
    if a.parent_lib:
        lines.append("# the calls that existed before, parent build vs this build (interleaved children)")
        for op in ("inference", "loss_and_grad"):
            for name, *_ in SHAPES:
                for B in BS:
                    k = f"{op} {name} B={B}"
                    pm = _quartiles(res["parent"][k])[0]
                    lines.append(f"{k}: parent {fmt(res['parent'][k])}; new {fmt(res['new'][k])} | new/parent {med(k) / pm:.4f}")
        for k, v in bits.items():
            same = len(v["parent"]) == 1 and v["parent"] == v["new"]
            lines.append(f"inference {k}, parent build vs this build: {'bit-identical' if same else 'DIFFERENT'} "
                         f"({sorted(v['parent'])} / {sorted(v['new'])})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
