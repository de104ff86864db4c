"""Times ONE inference_vjp_many of M members -- inference and its vector-Jacobian product for a per-sample cotangent, the CW form
of the ensemble gradient kernel -- against its two baselines, on the reference's README network (2-6-2) and its regression
network (16-48-16) at batch_size 32 over tspan (0, 13), TrainMode, README tolerances:

    python tools/prof_ensemble_vjp.py [--rounds 3] [--window 1.0] [--out profiles/ensemble_vjp_timing.txt]

Legs, alternated in every round in this order (one process: the three share the model, the inputs and the device's state):

    vjp     one inference_vjp_many of the M members, a random per-sample cotangent                       (the CW form)
    loss    one loss_and_grad_many of the same members: the same kernel without CW                       (baseline 1)
    loop    M times inference_record + inference_pullback on the handle, the same cotangents             (baseline 2: what
            a user does today; M = capacity: timed on the first 64 members and scaled to M, said in its row)

for M in {1, 64, ensemble_vjp_capacity}.  Every (shape, M, leg) is warmed up, then timed over at least `--window` seconds with
device events around synchronised work; a row gives the mean over the rounds' means in ms per pass over the M members, and the
spread (lowest and highest round).  Two ratios per row: vjp / loss (what CW costs over the built-in loss) and loop / vjp (what
one launch saves).  Before timing, the vjp leg's gradient for the loss's own cotangent is compared with the loss leg's.
"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = (("README 2-6-2", (2, 6, 2), 1, 1), ("regression 16-48-16", (16, 48, 16), 8, 8))
B = 32
TSPAN = (0.0, 13.0)
MS = (1, 64, "capacity")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_vjp_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import continuousnf.jl_amd as cnf
    T = cnf.TrainMode()
    lines = [f"inference_vjp_many against loss_and_grad_many and a loop of inference_record + inference_pullback: B = {B}, tspan {TSPAN}, "
             f"TrainMode, {args.rounds} rounds of {args.window} s windows per leg, device events; ms per pass over the M members",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    for name, dims, nvars, naugs in SHAPES:
        nn = cnf.Chain(cnf.Dense(dims[0], dims[1], "tanh"), cnf.Dense(dims[1], dims[2], "tanh"))
        icnf = cnf.construct(cnf.RNODE, nn, nvars, naugs, compute_mode=cnf.HIPVecJacMatrixMode(), tspan=TSPAN, lambda3=1e-2, rng=1)
        cap = cnf.ensemble_vjp_capacity(icnf, T, B)
        lines.append(f"{name}: ensemble_vjp_capacity {cap}, ensemble_capacity {cnf.ensemble_capacity(icnf, T, B)}")
        lines.append(f"  {'M':>6} {'vjp ms (lo..hi)':>26} {'loss ms (lo..hi)':>26} {'loop ms (lo..hi)':>30} {'vjp/loss':>9} {'loop/vjp':>9}")
        for M in MS:
            M = cap if M == "capacity" else M
            rng = np.random.default_rng(100 + M)
            ps = torch.from_numpy(np.stack([cnf.setup(np.random.default_rng(s), icnf.nn)[0] for s in range(M)])).cuda()
            xs = torch.from_numpy(rng.standard_normal((M, nvars, B)).astype(np.float32)).cuda()
            eps = torch.from_numpy(rng.standard_normal((M, nvars + naugs, B)).astype(np.float32)).cuda()
            cot = torch.from_numpy((rng.standard_normal((M, 4, B)) / B).astype(np.float32)).cuda()
            cot_arg = (cot[:, 0], (cot[:, 1], cot[:, 2], cot[:, 3]))
            n_loop = min(M, LOOP_MAX)

            def vjp():
                return cnf.inference_vjp_many(icnf, T, xs, ps, {}, cot_arg, eps=eps)

            def loss():
                return cnf.loss_and_grad_many(icnf, T, xs, ps, {}, eps=eps)

            def loop():
                for m in range(n_loop):
                    cnf.inference_record(icnf, T, xs[m], ps[m], {}, eps=eps[m], tspan=TSPAN)
                    cnf.inference_pullback(icnf, cot[m])

            # the two one-launch legs agree on the loss's own cotangent (same steps; the terminal cotangents round differently)
            ones = torch.ones((M, B), device="cuda") / B
            lc = (-ones, (icnf.lambda1 * ones, icnf.lambda2 * ones, icnf.lambda3 * ones))
            g1 = cnf.inference_vjp_many(icnf, T, xs, ps, {}, lc, eps=eps)[2]
            g2 = loss()[1]
            agree = float((g1 - g2).abs().max() / (g2.abs().max() + g2.pow(2).mean().sqrt()))
            res = {"vjp": [], "loss": [], "loop": []}
            for _ in range(args.rounds):
                res["vjp"].append(_timed(vjp, args.window, 2))
                res["loss"].append(_timed(loss, args.window, 2))
                res["loop"].append(_timed(loop, args.window, 1) * (M / n_loop))
            cell = lambda v: f"{np.mean(v):9.3f} ({min(v):.3f}..{max(v):.3f})"
            mv, ml, mp = (float(np.mean(res[k])) for k in ("vjp", "loss", "loop"))
            note = f"   loop: {n_loop} members timed, scaled to {M}" if n_loop < M else ""
            lines.append(f"  {M:>6} {cell(res['vjp']):>26} {cell(res['loss']):>26} {cell(res['loop']):>30} {mv / ml:9.3f} {mp / mv:9.1f}"
                         f"   loss cotangent: gradients differ by {agree:.1e} of their scale{note}")
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
