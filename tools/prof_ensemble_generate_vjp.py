"""Times ONE generate_vjp_many of M members -- sampling with log-density and its vector-Jacobian product for a per-sample
cotangent, the sampling form of the ensemble gradient kernel -- against what it replaces and what it should cost about as much
as, on the reference's README network (2-6-2) and its regression network (16-48-16) at 32 samples per member over tspan (0, 13),
TrainMode, README tolerances:

    python tools/prof_ensemble_generate_vjp.py [--rounds 3] [--window 1.0] [--out profiles/ensemble_generate_vjp_timing.txt]

Legs, alternated in every round in this order (one process: they share the model, the inputs and the device's state):

    gvjp    one generate_vjp_many of the M members, a random cotangent of (x, logq), with grad_z0       (the sampling form)
    ivjp    one inference_vjp_many of the same members on random data: the same sweeps in the density direction
    gen     one generate_many(with_logp=True) of the same members: the forward half alone, plain form
    loop    M times generate_record + generate_pullback on the handle, the same draws and cotangents    (what a user does
            today; M = capacity: timed on the first 64 members and scaled to M, said in its row)

for M in {64, ensemble_generate_vjp_capacity}.  Every (shape, M, leg) is warmed up, then timed over at least `--window` seconds
with device events around synchronised work; a row gives the mean over the rounds' means in ms per pass over the M members, and
the spread (lowest and highest round).  Two ratios per row: gvjp / ivjp and loop / gvjp.  Before timing, the gvjp leg's gradient
and accepted steps of member 0 are compared with the loop leg's (each is the adjoint of its own solve's steps: a comparison at the
level of the solver's tolerances unless the sequences coincide; the bar of the tests is against float64 on each route's own steps).
"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = (("README 2-6-2", (2, 6, 2), 1, 1), ("regression 16-48-16", (16, 48, 16), 8, 8))
B = 32
TSPAN = (0.0, 13.0)
MS = (64, "capacity")
LOOP_MAX = 64


def _timed(fn, window, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    total, n = 0.0, 0
    while total < window * 1e3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
        n += 1
    return total / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_generate_vjp_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import continuousnf.jl_amd as cnf
    T = cnf.TrainMode()
    lines = [f"generate_vjp_many against inference_vjp_many, generate_many and a loop of generate_record + generate_pullback: B = {B}, "
             f"tspan {TSPAN}, TrainMode, {args.rounds} rounds of {args.window} s windows per leg, device events; ms per pass over the M "
             f"members", f"device: {torch.cuda.get_device_name(0)}", ""]
    for name, dims, nvars, naugs in SHAPES:
        nn = cnf.Chain(cnf.Dense(dims[0], dims[1], "tanh"), cnf.Dense(dims[1], dims[2], "tanh"))
        icnf = cnf.construct(cnf.RNODE, nn, nvars, naugs, compute_mode=cnf.HIPVecJacMatrixMode(), tspan=TSPAN, lambda3=1e-2, rng=1)
        cap = cnf.ensemble_generate_vjp_capacity(icnf, T, B)
        lines.append(f"{name}: ensemble_generate_vjp_capacity {cap}, ensemble_vjp_capacity {cnf.ensemble_vjp_capacity(icnf, T, B)}, "
                     f"ensemble_eval_capacity {cnf.ensemble_eval_capacity(icnf, T, B)}")
        lines.append(f"  {'M':>6} {'gvjp ms (lo..hi)':>26} {'ivjp ms (lo..hi)':>26} {'gen ms (lo..hi)':>26} {'loop ms (lo..hi)':>30} "
                     f"{'gvjp/ivjp':>9} {'loop/gvjp':>9}")
        n_in = nvars + naugs
        for M in MS:
            M = cap if M == "capacity" else M
            rng = np.random.default_rng(100 + M)
            dev = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
            ps = torch.from_numpy(np.stack([cnf.setup(np.random.default_rng(s), icnf.nn)[0] for s in range(M)])).cuda()
            xs = dev(rng.standard_normal((M, nvars, B)))
            z0 = dev(rng.standard_normal((M, n_in, B)))
            eps = dev(rng.standard_normal((M, n_in, B)))
            gx, gl = dev(rng.standard_normal((M, nvars, B)) / B), dev(rng.standard_normal((M, B)) / B)
            cot4 = dev(rng.standard_normal((M, 4, B)) / B)
            cot4_arg = (cot4[:, 0], (cot4[:, 1], cot4[:, 2], cot4[:, 3]))
            n_loop = min(M, LOOP_MAX)

            def gvjp():
                return cnf.generate_vjp_many(icnf, T, ps, {}, B, (gx, gl), z0=z0, eps=eps, with_z0=True)

            def ivjp():
                return cnf.inference_vjp_many(icnf, T, xs, ps, {}, cot4_arg, eps=eps, with_x=True)

            def gen():
                return cnf.generate_many(icnf, T, ps, {}, B, z0=z0, eps=eps, with_logp=True)

            def loop():
                for m in range(n_loop):
                    cnf.generate_record(icnf, T, ps[m], {}, B, z0=z0[m], eps=eps[m], tspan=TSPAN)
                    cnf.generate_pullback(icnf, (gx[m], gl[m]), with_z0=True)

            # member 0 on both routes.  Each gradient is the exact adjoint of the steps ITS OWN solve accepted, and the two solves
            # evaluate tanh differently: where their step sequences differ, the gradients differ at the level of the tolerances
            first = cnf.generate_vjp_many(icnf, T, ps, {}, B, (gx, gl), z0=z0, eps=eps, with_steps=True)
            g1, s1, steps = first[2][0], first[-1]["steps"][0], first[-1]["stats"]
            cnf.generate_record(icnf, T, ps[0], {}, B, z0=z0[0], eps=eps[0], tspan=TSPAN)
            s2 = np.asarray(icnf.last_steps, np.float32)
            g2 = cnf.generate_pullback(icnf, (gx[0], gl[0]))
            agree = float((g1 - g2).abs().max() / (g2.abs().max() + g2.pow(2).mean().sqrt()))
            seq = "the same step sequence" if np.array_equal(s1, s2) else (
                f"step sequences differ by up to {np.abs(s1 - s2).max():.1e}" if len(s1) == len(s2) else "other step counts")
            res = {"gvjp": [], "ivjp": [], "gen": [], "loop": []}
            for _ in range(args.rounds):
                res["gvjp"].append(_timed(gvjp, args.window, 2))
                res["ivjp"].append(_timed(ivjp, args.window, 2))
                res["gen"].append(_timed(gen, args.window, 2))
                res["loop"].append(_timed(loop, args.window, 1) * (M / n_loop))
            cell = lambda v: f"{np.mean(v):9.3f} ({min(v):.3f}..{max(v):.3f})"
            mg, mi, mp = (float(np.mean(res[k])) for k in ("gvjp", "ivjp", "loop"))
            note = f"   loop: {n_loop} members timed, scaled to {M}" if n_loop < M else ""
            acc = [s["naccept"] for s in steps]
            lines.append(f"  {M:>6} {cell(res['gvjp']):>26} {cell(res['ivjp']):>26} {cell(res['gen']):>26} {cell(res['loop']):>30} "
                         f"{mg / mi:9.3f} {mp / mg:9.1f}   accepted steps per member {min(acc)}..{max(acc)}; member 0 against the loop's: "
                         f"{len(s1)} and {len(s2)} accepted steps, {seq}, gradients differ by {agree:.1e} of their scale{note}")
            print(lines[-1], flush=True)
        icnf.close()
        lines.append("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
