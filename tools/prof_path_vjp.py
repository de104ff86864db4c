"""Times differentiable flow paths (inference_path_vjp, generate_path_vjp) beside two baselines, both run on the PARENT build:
the same launch without the path -- inference_vjp_many / generate_vjp_many with M = 1 at the same shape, so the difference is the
cost of the feature -- and what a user could do before: K inference_record + inference_pullback pairs over the K sub-spans (each
pair started from the data again: the cost of the workaround, not its values).  On the reference's README network (2-6-2) and its
regression network (16-48-16) over tspan (0, 13), README tolerances, TrainMode, at B = 32 and at the capacity
(path_vjp_max_batch), with K = 1, 16, 256 equally spaced save times and a cotangent on every row of every slice.

    python tools/prof_path_vjp.py --parent-lib /path/to/parent/libcnfhip.so [--rounds 2] [--window 0.3] [--out profiles/path_vjp_timing.txt]

One child process per leg, started in alternation by this script (CNFHIP_LIB is read at import; a fresh child each time -- never
an exec over a process that has opened the GPU), in the manner of tools/prof_path.py.  Every figure is warmed up, then timed over
at least `--window` seconds with device events around synchronised work; the file gives the median and the interquartile range
of the samples of all rounds, the capacities, and the registers' share of them.  No threshold is asserted.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = (("README 2-6-2", (2, 6, 2), 1, 1), ("regression 16-48-16", (16, 48, 16), 8, 8))
TSPAN = (0.0, 13.0)
KS = (1, 16, 256)
KEEP = 400


def _timed(fn, window, warm=2):
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
    nn = cnf.Chain(*[cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])])
    return cnf.construct(cnf.RNODE, nn, nvars, naugs, compute_mode=cnf.HIPVecJacMatrixMode(), tspan=TSPAN, lambda3=1e-2, rng=1)


def child(leg, window, caps):
    import numpy as np
    import torch
    from continuousnf.jl_amd import _lib
    if leg == "parent":                              # (an earlier build does not export the entry points added since)
        import ctypes
        l = ctypes.CDLL(_lib.LIB_PATH)
        for table in [v for k, v in vars(_lib).items() if k.endswith("_SIGNATURES") and isinstance(v, dict)]:
            for name in list(table):
                if not hasattr(l, name):
                    table.pop(name)
    import continuousnf.jl_amd as cnf
    out = {"leg": leg, "lib": _lib.LIB_PATH, "samples": {}, "caps": {}, "steps": {}}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    mode = cnf.TrainMode()
    for name, dims, nvars, naugs in SHAPES:
        icnf = _model(cnf, dims, nvars, naugs)
        n_in = nvars + naugs
        if leg == "new":
            out["caps"][name] = {"path_vjp_max_batch": cnf.path_vjp_max_batch(icnf, mode),
                                 **{f"ensemble_vjp_capacity B={B}": cnf.ensemble_vjp_capacity(icnf, mode, B) for B in (32, 4096, 8192)}}
            cap = out["caps"][name]["path_vjp_max_batch"]
        else:
            cap = caps[name]
        for B in (32, cap):
            key = f"{name} B={B}"
            rng = np.random.default_rng(7)
            lim = np.sqrt(6.0 / (dims[0] + dims[1]))
            ps = dev(rng.uniform(-lim, lim, size=icnf.nn.n_params_internal))
            xs, eps, z0 = dev(rng.beta(2.0, 4.0, size=(nvars, B))), dev(rng.standard_normal((n_in, B))), dev(rng.standard_normal((n_in, B)))
            g1, g4 = dev(rng.standard_normal(B) / B), tuple(dev(rng.standard_normal(B) / B) for _ in range(3))
            gz = dev(rng.standard_normal((n_in, B)) / B)
            if leg == "parent":
                c1 = (g1[None], tuple(g[None] for g in g4))
                out["samples"][f"inference_vjp_many M=1 {key}"] = _timed(
                    lambda: cnf.inference_vjp_many(icnf, mode, xs[None], ps[None], {}, c1, eps=eps[None], with_x=True), window)
                out["samples"][f"generate_vjp_many M=1 {key}"] = _timed(
                    lambda: cnf.generate_vjp_many(icnf, mode, ps[None], {}, B, (gz[None], g1[None]), z0=z0[None], eps=eps[None], with_z0=True),
                    window)
                for K in KS:
                    edges = np.linspace(TSPAN[0], TSPAN[1], K + 1)

                    def chain():
                        for a, b in zip(edges[:-1], edges[1:]):
                            cnf.inference_record(icnf, mode, xs, ps, {}, eps=eps, tspan=(float(a), float(b)))
                            cnf.inference_pullback(icnf, (g1, g4), with_x=True)
                    out["samples"][f"chained record+pullback K={K} {key}"] = _timed(chain, window, 1)
                continue
            for K in KS:
                saveat = np.linspace(TSPAN[0], TSPAN[1], K + 1)[1:]
                pc = {"z": dev(rng.standard_normal((K, n_in, B)) / B), "dlogp": dev(rng.standard_normal((K, B)) / B),
                      "E": dev(rng.standard_normal((K, B)) / B), "n": dev(rng.standard_normal((K, B)) / B)}
                out["samples"][f"inference_path_vjp K={K} {key}"] = _timed(
                    lambda: cnf.inference_path_vjp(icnf, mode, xs, ps, {}, saveat=saveat, cot=(g1, g4), path_cot=pc, eps=eps, with_x=True), window)
                out["steps"][f"inference_path_vjp K={K} {key}"] = icnf.last_stats["naccept"]
                pg = {"z": pc["z"], "logq": pc["dlogp"]}
                back = np.linspace(TSPAN[1], TSPAN[0], K + 1)[1:]            # sampling runs over the reversed span
                out["samples"][f"generate_path_vjp K={K} {key}"] = _timed(
                    lambda: cnf.generate_path_vjp(icnf, mode, ps, {}, B, saveat=back, cot=(gz, g1), path_cot=pg, z0=z0, eps=eps,
                                                  with_z0=True), window)
                out["steps"][f"generate_path_vjp K={K} {key}"] = icnf.last_stats["naccept"]
        icnf.close()
    print("PROF_PATH_VJP " + json.dumps(out), flush=True)


def run_child(leg, lib, window, caps):
    env = dict(os.environ)
    if lib:
        env["CNFHIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("CNFHIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--window", str(window), "--caps", json.dumps(caps)],
                       env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"child {leg} ended with status {r.returncode}")
    line = [l for l in r.stdout.splitlines() if l.startswith("PROF_PATH_VJP ")][-1]
    return json.loads(line[len("PROF_PATH_VJP "):])


def _quartiles(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, max(0, int(round(p * (len(v) - 1)))))]
    return q(0.5), q(0.25), q(0.75)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=False)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out")
    ap.add_argument("--child")
    ap.add_argument("--caps", default="{}")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.window, json.loads(a.caps))
    res, caps, steps = {}, {}, {}
    for _ in range(a.rounds):
        out = run_child("new", None, a.window, {})   # the legs alternate: one child each, one at a time
        caps, steps = out["caps"], out["steps"]
        legs = [out]
        if a.parent_lib:
            legs.append(run_child("parent", a.parent_lib, a.window, {k: v["path_vjp_max_batch"] for k, v in caps.items()}))
        for o in legs:
            for key, v in o["samples"].items():
                res.setdefault(key, []).extend(v)
    fmt = lambda k: "{:.3f} [{:.3f}, {:.3f}] ({})".format(*_quartiles(res[k]), len(res[k])) if k in res else "not run"
    med = lambda k: _quartiles(res[k])[0] if k in res else float("nan")
    lines = [f"# tools/prof_path_vjp.py: ms per call, median [IQR] (samples) over {a.rounds} rounds, window {a.window} s per figure; "
             f"TrainMode (VJP), README tolerances, tspan {TSPAN}; the two baselines on the parent build"]
    for name, *_ in SHAPES:
        lines.append(f"{name}: capacities {json.dumps(caps[name])}")
        for B in (32, caps[name]["path_vjp_max_batch"]):
            key = f"{name} B={B}"
            for fn, base in (("inference_path_vjp", "inference_vjp_many"), ("generate_path_vjp", "generate_vjp_many")):
                bk = f"{base} M=1 {key}"
                lines.append(f"{bk} (parent build, no path): {fmt(bk)}")
                for K in KS:
                    k = f"{fn} K={K} {key}"
                    s = f"{k}: {fmt(k)}, {steps.get(k)} steps | over the no-path launch x{med(k) / med(bk):.2f} (+{med(k) - med(bk):.3f} ms)"
                    ck = f"chained record+pullback K={K} {key}"
                    if fn == "inference_path_vjp":
                        s += f" | {K} chained record+pullback pairs (parent build) {fmt(ck)}, chained/one launch {med(ck) / med(k):.1f}"
                    lines.append(s)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
