"""Times the ensemble calls with a base distribution per member (``bases=``: include/cnfhip_ensemble_base.h) on the reference's
README network (2-6-2) and its regression network (16-48-16) at B = 32 over tspan (0, 13), README tolerances, TrainMode / VJP, at
64 members and at the capacity, dense bases:

  (a) inference_many, loss_and_grad_many, inference_vjp_many, generate_vjp_many with bases against the same call without: the
      cost of the base (one column pass behind the launch, four MFMAs per tile inside it);
  (b) the same calls with bases against what a user does without them: a loop of 64 single-model calls on a model whose
      ``basedist`` is set per member (the recorded route, and one synchronous upload per member);
  (c) a learnable step -- differentiable_inference_many forward + backward with bases that require grad -- against 64 x
      (inference_record + inference_pullback(with_base=True) + the upload of the next member's base);
  (d) the calls that existed before, WITHOUT bases, on this build and on the parent build, interleaved, and with --parent-tree
      `bench.py --gpus 1 --steps 20 --warmup 5` in both trees: the file says which of them is slower on this build by more than
      the two interquartile ranges together.

    python tools/prof_ensemble_base.py --parent-lib /path/to/parent/libcnfhip.so [--parent-tree /path/to/parent/checkout]
                                       [--rounds 2] [--window 0.1] [--out profiles/ensemble_base_timing.txt]

One child process per leg, started in alternation by this script (CNFHIP_LIB is read at import; a fresh child each time -- never
an exec over a process that has opened the GPU), in the manner of tools/prof_ensemble_path.py.  Every figure is warmed up, then
timed over at least `--window` seconds (at least three samples) with device events around synchronised work; the file gives
the median and the interquartile range of the samples of all rounds.  No threshold is asserted.
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
B = 32
LOOP_M = 64
KEEP = 400
TAG = "PROF_ENSEMBLE_BASE "
CALLS = ("inference_many", "loss_and_grad_many", "inference_vjp_many", "generate_vjp_many")
SINGLE = dict(zip(CALLS, ("inference", "loss_and_grad", "inference_record + inference_pullback", "generate_record + generate_pullback")))
CAP_OF = dict(zip(CALLS, ("eval", "grad", "vjp", "generate_vjp")))


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


def _model(cnf, dims, nvars, naugs, **kw):
    nn = cnf.Chain(*[cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])])
    return cnf.construct(cnf.RNODE, nn, nvars, naugs, compute_mode=cnf.HIPVecJacMatrixMode(), tspan=TSPAN, lambda3=1e-2, rng=1, **kw)


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
            l, h, m = _lib.lib(), icnf.handle(), _lib.MODE_TRAIN
            out["caps"][name] = {"eval": cnf.ensemble_eval_capacity(icnf, mode, B),
                                 "grad": min(cnf.ensemble_capacity(icnf, mode, B), l.cnf_ensemble_base_capacity(h, m, B, 0)),
                                 "vjp": min(cnf.ensemble_vjp_capacity(icnf, mode, B), l.cnf_ensemble_base_capacity(h, m, B, 1)),
                                 "generate_vjp": cnf.ensemble_generate_vjp_capacity(icnf, mode, B)}
        cap = (out["caps"] if leg == "new" else caps)[name]
        Mx = max([LOOP_M] + list(cap.values()))
        rng = np.random.default_rng(7)
        lim = np.sqrt(6.0 / (dims[0] + dims[1]))
        ps = dev(rng.uniform(-lim, lim, size=(Mx, icnf.nn.n_params_internal)))
        xs, eps, z0 = dev(rng.beta(2.0, 4.0, size=(Mx, nvars, B))), dev(rng.standard_normal((Mx, n_in, B))), dev(rng.standard_normal((Mx, n_in, B)))
        g1, g4 = dev(rng.standard_normal((Mx, B)) / B), tuple(dev(rng.standard_normal((Mx, B)) / B) for _ in range(3))
        gz = dev(rng.standard_normal((Mx, n_in, B)) / B)
        mean = rng.uniform(-1.0, 1.0, (Mx, n_in))
        L = np.tril(rng.standard_normal((Mx, n_in, n_in)), -1) * (0.3 / np.sqrt(n_in)) + np.stack([np.diag(rng.uniform(0.6, 1.6, n_in)) for _ in range(Mx)])
        put = lambda key, fn, warm=2: out["samples"].__setitem__(f"{key} | {name}", _timed(fn, window, warm))

        def call(c, M, **kw):
            s = slice(0, M)
            cm = (g1[s], tuple(g[s] for g in g4))
            return {"inference_many": lambda: cnf.inference_many(icnf, mode, xs[s], ps[s], {}, eps=eps[s], **kw),
                    "loss_and_grad_many": lambda: cnf.loss_and_grad_many(icnf, mode, xs[s], ps[s], {}, eps=eps[s], **kw),
                    "inference_vjp_many": lambda: cnf.inference_vjp_many(icnf, mode, xs[s], ps[s], {}, cm, eps=eps[s], with_x=True, **kw),
                    "generate_vjp_many": lambda: cnf.generate_vjp_many(icnf, mode, ps[s], {}, B, (gz[s], g1[s]), z0=z0[s], eps=eps[s],
                                                                       with_z0=True, **kw)}[c]

        # ---- (d) calls that existed before, without bases: on both builds, interleaved by the parent process ----
        for c in CALLS:
            put(f"existing {c} M={LOOP_M}", call(c, LOOP_M))
        if leg == "parent":
            icnf.close()
            continue
        # ---- (a) with bases against without, at 64 members and at the capacity ----
        for c in CALLS:
            for M in sorted({LOOP_M, cap[CAP_OF[c]]}):
                bases = cnf.EnsembleBases(dev(mean[:M]), scale_tril=dev(L[:M]))
                put(f"{c} M={M} without bases", call(c, M))
                put(f"{c} M={M} with bases", call(c, M, bases=bases))
        # ---- (b) what a user does today: a loop of 64 single-model calls, the member's base uploaded before each ----
        single = _model(cnf, dims, nvars, naugs)
        mt, Lt = dev(mean[:LOOP_M]), dev(L[:LOOP_M])
        single.basedist = cnf.LearnableNormal(mt[0], scale_tril=Lt[0])

        def one(c, m):
            single.basedist.update(mt[m], scale_tril=Lt[m])          # (the next call uploads it: cnf_set_basedist, synchronous)
            if c == "inference_many":
                return cnf.inference(single, mode, xs[m], ps[m], {}, eps=eps[m])
            if c == "loss_and_grad_many":
                return cnf.loss_and_grad(single, mode, xs[m], ps[m], {}, eps=eps[m])
            if c == "inference_vjp_many":
                cnf.inference_record(single, mode, xs[m], ps[m], {}, eps=eps[m])
                return cnf.inference_pullback(single, (g1[m], tuple(g[m] for g in g4)), with_x=True)
            cnf.generate_record(single, mode, ps[m], {}, B, z0=z0[m], eps=eps[m])
            return cnf.generate_pullback(single, (gz[m], g1[m]), with_z0=True)

        for c in CALLS:
            put(f"loop of {LOOP_M} {SINGLE[c]} with basedist", lambda: [one(c, m) for m in range(LOOP_M)], 1)

        # ---- (c) a learnable step ----
        def learnable(m):
            single.basedist.update(mt[m], scale_tril=Lt[m])
            cnf.inference_record(single, mode, xs[m], ps[m], {}, eps=eps[m])
            return cnf.inference_pullback(single, (g1[m], None), with_base=True)

        put(f"learnable step: loop of {LOOP_M} (upload + inference_record + inference_pullback(with_base=True))",
            lambda: [learnable(m) for m in range(LOOP_M)], 1)
        mu_t, L_t = dev(mean[:LOOP_M]).requires_grad_(True), dev(L[:LOOP_M]).requires_grad_(True)
        p_t = ps[:LOOP_M].clone().requires_grad_(True)

        def step():
            for t in (mu_t, L_t, p_t):
                t.grad = None
            lp, _ = cnf.differentiable_inference_many(icnf, mode, xs[:LOOP_M], p_t, {}, eps=eps[:LOOP_M],
                                                      bases=cnf.EnsembleBases(mu_t, scale_tril=L_t))
            (g1[:LOOP_M] * lp).sum().backward()

        put(f"learnable step: differentiable_inference_many M={LOOP_M} forward + backward + base pullback", step)
        single.close()
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
    for r in range(a.rounds):                        # the legs alternate: one child each, one at a time
        out = run_child("new", None, a.window, {})
        caps = out["caps"]
        legs = [out]
        if a.parent_lib:
            legs.append(run_child("parent", a.parent_lib, a.window, caps))
        for o in legs:
            print(f"round {r + 1}: leg {o['leg']} done, {len(o['samples'])} figures", file=sys.stderr, flush=True)
            for key, v in o["samples"].items():
                res[o["leg"]].setdefault(key, []).extend(v)
        if a.parent_tree:
            for leg, tree in (("new", ROOT), ("parent", a.parent_tree)):
                ms = run_bench(tree)
                print(f"round {r + 1}: bench.py, {leg}: {ms}", file=sys.stderr, flush=True)
                if ms is not None:
                    res[leg].setdefault("existing bench.py --gpus 1 --steps 20 --warmup 5 (ms_per_step) | flagship", []).append(ms)

    def fmt(leg, k):
        return "{:.3f} [{:.3f}, {:.3f}] ({})".format(*_quartiles(res[leg][k]), len(res[leg][k])) if k in res[leg] else "not run"

    med = lambda leg, k: _quartiles(res[leg][k])[0] if k in res[leg] else float("nan")
    lines = [f"# tools/prof_ensemble_base.py: ms per call, median [IQR] (samples) over {a.rounds} rounds, window {a.window} s per figure; "
             f"B = {B}, TrainMode (VJP), README tolerances, tspan {TSPAN}, dense bases"]
    for name, *_ in SHAPES:
        lines.append(f"{name}: capacities at B = {B} (with bases) {json.dumps(caps[name])}")
        for c in CALLS:
            lk = f"loop of {LOOP_M} {SINGLE[c]} with basedist | {name}"
            for M in sorted({LOOP_M, caps[name][CAP_OF[c]]}):
                kb, k0 = f"{c} M={M} with bases | {name}", f"{c} M={M} without bases | {name}"
                s = (f"  (a) {c} M={M}: with bases {fmt('new', kb)} | without {fmt('new', k0)} | x{med('new', kb) / med('new', k0):.3f} "
                     f"(+{med('new', kb) - med('new', k0):.3f} ms)")
                if M == LOOP_M:
                    s += f" | (b) loop of {LOOP_M} {SINGLE[c]}, basedist set per member: {fmt('new', lk)} | loop / one call {med('new', lk) / med('new', kb):.1f}"
                lines.append(s)
        ka = f"learnable step: differentiable_inference_many M={LOOP_M} forward + backward + base pullback | {name}"
        kl = f"learnable step: loop of {LOOP_M} (upload + inference_record + inference_pullback(with_base=True)) | {name}"
        lines.append(f"  (c) learnable step, M={LOOP_M}: differentiable_inference_many forward + backward {fmt('new', ka)} | loop of {LOOP_M} x "
                     f"(upload + inference_record + inference_pullback(with_base=True)) {fmt('new', kl)} | loop / one step "
                     f"{med('new', kl) / med('new', ka):.1f}")
    lines.append("(d) existing calls without bases, this build against the parent build (interleaved):")
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
