"""Times the four ensemble path calls (inference_path_many, generate_path_many, inference_path_vjp_many, generate_path_vjp_many)
beside two baselines, both run on the PARENT build: what a user does without them -- a loop of M single-model calls
(inference_path, generate_path, inference_path_vjp, generate_path_vjp) -- and the same ensemble call without a path
(inference_many, generate_many, inference_vjp_many, generate_vjp_many), so that the difference is the cost of the path itself.
On the reference's README network (2-6-2) and its regression network (16-48-16) over tspan (0, 13), README tolerances, TrainMode /
VJP, B = 32, M in {1, 64, capacity}, K in {1, 16, 256} equally spaced save times, a cotangent on every row of every slice.  The
loop is timed at M = 1 and M = 64; at M = capacity it is the M = 64 loop scaled by capacity / 64 (a loop of independent calls
is linear in M; the file says so on every such figure).

It also times calls that existed before on both builds, interleaved -- inference_path, inference_path_vjp, inference_many,
inference_vjp_many (M = 64) -- and, with --parent-tree, `bench.py --gpus 1 --steps 20 --warmup 5` in both trees, and says which of
them is slower on this build by more than the two interquartile ranges together.

    python tools/prof_ensemble_path.py --parent-lib /path/to/parent/libcnfhip.so [--parent-tree /path/to/parent/checkout]
                                       [--rounds 2] [--window 0.1] [--out profiles/ensemble_path_timing.txt]

One child process per leg, started in alternation by this script (CNFHIP_LIB is read at import; a fresh child each time -- never
an exec over a process that has opened the GPU), in the manner of tools/prof_path_vjp.py.  Every figure is warmed up, then timed
over at least `--window` seconds (at least three samples) with device events around synchronised work; the file gives the median
and the interquartile range of the samples of all rounds.  No threshold is asserted.
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
B = 32
LOOP_M = 64
KEEP = 400
TAG = "PROF_ENSEMBLE_PATH "
CALLS = ("inference_path_many", "generate_path_many", "inference_path_vjp_many", "generate_path_vjp_many")
SINGLE = dict(zip(CALLS, ("inference_path", "generate_path", "inference_path_vjp", "generate_path_vjp")))
NOPATH = dict(zip(CALLS, ("inference_many", "generate_many", "inference_vjp_many", "generate_vjp_many")))


def _timed(fn, window, warm=2):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    total, per = 0.0, []
    while total < window * 1e3 or len(per) < 3:
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
    out = {"leg": leg, "lib": _lib.LIB_PATH, "samples": {}, "caps": {}}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    mode = cnf.TrainMode()
    for name, dims, nvars, naugs in SHAPES:
        icnf = _model(cnf, dims, nvars, naugs)
        n_in = nvars + naugs
        if leg == "new":
            out["caps"][name] = {"ensemble_path_capacity": cnf.ensemble_path_capacity(icnf, mode, B),
                                 "ensemble_path_vjp_capacity": cnf.ensemble_path_vjp_capacity(icnf, mode, B),
                                 "ensemble_eval_capacity": cnf.ensemble_eval_capacity(icnf, mode, B),
                                 "ensemble_vjp_capacity": cnf.ensemble_vjp_capacity(icnf, mode, B),
                                 "ensemble_generate_vjp_capacity": cnf.ensemble_generate_vjp_capacity(icnf, mode, B)}
        cap = (out["caps"] if leg == "new" else caps)[name]
        Ms = {"plain": (1, LOOP_M, cap["ensemble_path_capacity"]), "vjp": (1, LOOP_M, cap["ensemble_path_vjp_capacity"])}
        Mx = max(Ms["plain"] + Ms["vjp"])
        rng = np.random.default_rng(7)
        lim = np.sqrt(6.0 / (dims[0] + dims[1]))
        ps = dev(rng.uniform(-lim, lim, size=(Mx, icnf.nn.n_params_internal)))
        xs, eps, z0 = dev(rng.beta(2.0, 4.0, size=(Mx, nvars, B))), dev(rng.standard_normal((Mx, n_in, B))), dev(rng.standard_normal((Mx, n_in, B)))
        g1, g4 = dev(rng.standard_normal((Mx, B)) / B), tuple(dev(rng.standard_normal((Mx, B)) / B) for _ in range(3))
        gz = dev(rng.standard_normal((Mx, n_in, B)) / B)
        put = lambda key, fn, warm=2: out["samples"].__setitem__(f"{key} | {name}", _timed(fn, window, warm))
        fwd = lambda K: np.linspace(TSPAN[0], TSPAN[1], K + 1)[1:]
        back = lambda K: np.linspace(TSPAN[1], TSPAN[0], K + 1)[1:]          # sampling runs over the reversed span
        # ---- calls that existed before: on both builds, interleaved by the parent process ----
        sv16 = fwd(16)
        pc1 = {"z": dev(rng.standard_normal((16, n_in, B)) / B), "dlogp": dev(rng.standard_normal((16, B)) / B)}
        put("existing inference_path K=16", lambda: cnf.inference_path(icnf, mode, xs[0], ps[0], {}, saveat=sv16, eps=eps[0]))
        put("existing inference_path_vjp K=16", lambda: cnf.inference_path_vjp(icnf, mode, xs[0], ps[0], {}, saveat=sv16, cot=(g1[0], tuple(g[0] for g in g4)),
                                                                              path_cot=pc1, eps=eps[0], with_x=True))
        m64 = slice(0, LOOP_M)
        c64 = (g1[m64], tuple(g[m64] for g in g4))
        put("existing inference_many M=64", lambda: cnf.inference_many(icnf, mode, xs[m64], ps[m64], {}, eps=eps[m64]))
        put("existing inference_vjp_many M=64", lambda: cnf.inference_vjp_many(icnf, mode, xs[m64], ps[m64], {}, c64, eps=eps[m64], with_x=True))
        if leg == "parent":
            # ---- the ensemble calls without a path, at the M of the path calls ----
            for kind, call in (("plain", "inference_path_many"), ("plain", "generate_path_many"), ("vjp", "inference_path_vjp_many"),
                               ("vjp", "generate_path_vjp_many")):
                for M in Ms[kind]:
                    s = slice(0, M)
                    cm = (g1[s], tuple(g[s] for g in g4))
                    fn = {"inference_path_many": lambda: cnf.inference_many(icnf, mode, xs[s], ps[s], {}, eps=eps[s]),
                          "generate_path_many": lambda: cnf.generate_many(icnf, mode, ps[s], {}, B, z0=z0[s], eps=eps[s], with_logp=True),
                          "inference_path_vjp_many": lambda: cnf.inference_vjp_many(icnf, mode, xs[s], ps[s], {}, cm, eps=eps[s], with_x=True),
                          "generate_path_vjp_many": lambda: cnf.generate_vjp_many(icnf, mode, ps[s], {}, B, (gz[s], g1[s]), z0=z0[s], eps=eps[s],
                                                                                  with_z0=True)}[call]
                    put(f"{NOPATH[call]} M={M} (no path, for {call})", fn)
            # ---- what a user does today: a loop of M single-model calls ----
            for K in KS:
                svf, svb = fwd(K), back(K)
                pc = {"z": dev(rng.standard_normal((K, n_in, B)) / B), "dlogp": dev(rng.standard_normal((K, B)) / B),
                      "E": dev(rng.standard_normal((K, B)) / B), "n": dev(rng.standard_normal((K, B)) / B)}
                pg = {"z": pc["z"], "logq": pc["dlogp"]}
                one = {"inference_path_many": lambda m: cnf.inference_path(icnf, mode, xs[m], ps[m], {}, saveat=svf, eps=eps[m]),
                       "generate_path_many": lambda m: cnf.generate_path(icnf, mode, ps[m], {}, B, saveat=svb, z0=z0[m], eps=eps[m]),
                       "inference_path_vjp_many": lambda m: cnf.inference_path_vjp(icnf, mode, xs[m], ps[m], {}, saveat=svf,
                                                                                   cot=(g1[m], tuple(g[m] for g in g4)), path_cot=pc, eps=eps[m],
                                                                                   with_x=True),
                       "generate_path_vjp_many": lambda m: cnf.generate_path_vjp(icnf, mode, ps[m], {}, B, saveat=svb, cot=(gz[m], g1[m]),
                                                                                 path_cot=pg, z0=z0[m], eps=eps[m], with_z0=True)}
                for call in CALLS:
                    for M in (1, LOOP_M):
                        put(f"loop of {M} {SINGLE[call]} K={K}", lambda: [one[call](m) for m in range(M)], 1)
            icnf.close()
            continue
        # ---- the ensemble path calls ----
        for K in KS:
            svf, svb = fwd(K), back(K)
            for call in CALLS:
                kind = "vjp" if "vjp" in call else "plain"
                for M in Ms[kind]:
                    s = slice(0, M)
                    if kind == "vjp":
                        rn = lambda *shape: torch.randn(shape, device="cuda") / B      # (drawn on the device: M K B D values)
                        pc = {"z": rn(M, K, n_in, B), "dlogp": rn(M, K, B)}
                        pi = dict(pc, E=rn(M, K, B), n=rn(M, K, B))
                        pg = {"z": pc["z"], "logq": pc["dlogp"]}
                    cm = (g1[s], tuple(g[s] for g in g4))
                    fn = {"inference_path_many": lambda: cnf.inference_path_many(icnf, mode, xs[s], ps[s], {}, saveat=svf, eps=eps[s]),
                          "generate_path_many": lambda: cnf.generate_path_many(icnf, mode, ps[s], {}, B, saveat=svb, z0=z0[s], eps=eps[s]),
                          "inference_path_vjp_many": lambda: cnf.inference_path_vjp_many(icnf, mode, xs[s], ps[s], {}, saveat=svf, cot=cm,
                                                                                         path_cot=pi, eps=eps[s], with_x=True),
                          "generate_path_vjp_many": lambda: cnf.generate_path_vjp_many(icnf, mode, ps[s], {}, B, saveat=svb, cot=(gz[s], g1[s]),
                                                                                       path_cot=pg, z0=z0[s], eps=eps[s], with_z0=True)}[call]
                    put(f"{call} M={M} K={K}", fn)
        icnf.close()
    print(TAG + json.dumps(out), flush=True)


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
    line = [l for l in r.stdout.splitlines() if l.startswith(TAG)][-1]
    return json.loads(line[len(TAG):])


def run_bench(tree):
    """`bench.py --gpus 1 --steps 20 --warmup 5` in `tree`, a fresh process: ms_per_step of its JSON line (None: no such figure)."""
    env = dict(os.environ)
    env.pop("CNFHIP_LIB", None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, env=env, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"bench.py in {tree} ended with status {r.returncode}")
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line).get("ms_per_step")
    return None


def _quartiles(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, max(0, int(round(p * (len(v) - 1)))))]
    return q(0.5), q(0.25), q(0.75)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=False)
    ap.add_argument("--parent-tree", required=False)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--out")
    ap.add_argument("--child")
    ap.add_argument("--caps", default="{}")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.window, json.loads(a.caps))
    res = {"new": {}, "parent": {}}
    caps = {}
    for _ in range(a.rounds):                        # the legs alternate: one child each, one at a time
        out = run_child("new", None, a.window, {})
        caps = out["caps"]
        legs = [out]
        if a.parent_lib:
            legs.append(run_child("parent", a.parent_lib, a.window, caps))
        for o in legs:
            print(f"round {_ + 1}: leg {o['leg']} done, {len(o['samples'])} figures", file=sys.stderr, flush=True)
            for key, v in o["samples"].items():
                res[o["leg"]].setdefault(key, []).extend(v)
        if a.parent_tree:
            for leg, tree in (("new", ROOT), ("parent", a.parent_tree)):
                ms = run_bench(tree)
                print(f"round {_ + 1}: bench.py, {leg}: {ms}", file=sys.stderr, flush=True)
                if ms is not None:
                    res[leg].setdefault("existing bench.py --gpus 1 --steps 20 --warmup 5 (ms_per_step) | flagship", []).append(ms)

    def fmt(leg, k):
        return "{:.3f} [{:.3f}, {:.3f}] ({})".format(*_quartiles(res[leg][k]), len(res[leg][k])) if k in res[leg] else "not run"

    med = lambda leg, k: _quartiles(res[leg][k])[0] if k in res[leg] else float("nan")
    lines = [f"# tools/prof_ensemble_path.py: ms per call, median [IQR] (samples) over {a.rounds} rounds, window {a.window} s per figure; "
             f"B = {B}, TrainMode (VJP), README tolerances, tspan {TSPAN}; the baselines on the parent build"]
    for name, *_ in SHAPES:
        lines.append(f"{name}: capacities at B = {B} {json.dumps(caps[name])}")
        for call in CALLS:
            cap = caps[name]["ensemble_path_vjp_capacity" if "vjp" in call else "ensemble_path_capacity"]
            for M in (1, LOOP_M, cap):
                nk = f"{NOPATH[call]} M={M} (no path, for {call}) | {name}"
                lines.append(f"  {NOPATH[call]} M={M} (parent build, no path): {fmt('parent', nk)}")
                for K in KS:
                    k = f"{call} M={M} K={K} | {name}"
                    lm = M if M in (1, LOOP_M) else LOOP_M
                    lk = f"loop of {lm} {SINGLE[call]} K={K} | {name}"
                    loop = med("parent", lk) * (M / lm)
                    how = f"{fmt('parent', lk)}" if lm == M else f"{loop:.3f} = the loop of {LOOP_M}, {fmt('parent', lk)}, x {M}/{LOOP_M}"
                    lines.append(f"  {call} M={M} K={K}: {fmt('new', k)} | loop of {M} {SINGLE[call]} (parent build) {how} | loop / one call "
                                 f"{loop / med('new', k):.1f} | over the no-path call x{med('new', k) / med('parent', nk):.2f} "
                                 f"(+{med('new', k) - med('parent', nk):.3f} ms)")
    lines.append("existing calls, this build against the parent build (interleaved):")
    for k in sorted(res["new"]):
        if not k.startswith("existing"):
            continue
        s = f"  {k}: this build {fmt('new', k)} | parent build {fmt('parent', k)}"
        if k in res["parent"]:
            (mn, ln, hn), (mp, lp, hp) = _quartiles(res["new"][k]), _quartiles(res["parent"][k])
            s += f" | ratio {mn / mp:.3f}"
            s += " | SLOWER by more than the two IQRs together" if mn - mp > (hn - ln) + (hp - lp) else " | within the two IQRs together, or faster"
        lines.append(s)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
