"""Times differentiable sampling (generate_record + generate_pullback) beside differentiable inference (inference_record +
inference_pullback) on the headline network: the two run the same solve and pullback kernels, one forward and one backward in time.

    python tools/prof_gen_vjp.py [--rounds 3] [--window 1.0] [--out profiles/gen_vjp_timing.txt]

One process; per shape both legs are warmed up and then timed in alternation, `--rounds` times each, over a window of at least
`--window` seconds of device-event time around synchronised calls.  Reported per leg: the median over the rounds of the
window's ms per call, the accepted steps of its solve, and the ratio of the medians.
"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = (("cfg3 B=32", 3, 32), ("cfg3 B=8192", 3, 8192))


def _window(fn, window):
    import torch
    n, total = 0, 0.0
    while total < window * 1e3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(4):
            fn()
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
        n += 4
    return total / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import configs
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["# ms per call (median of %d alternated rounds, %.1f s windows): inference_record + inference_pullback | "
             "generate_record + generate_pullback | ratio | accepted steps of the two solves" % (a.rounds, a.window)]
    for name, i, B in SHAPES:
        wl = configs.BASELINE[i]
        flat = torch.from_numpy(configs.glorot_params(wl.dims, i, 0.05)).cuda()
        xs_h, eps_h = configs.synthetic_inputs(wl, B, i)
        xs, eps = torch.from_numpy(xs_h).cuda(), torch.from_numpy(eps_h).cuda()
        z0 = torch.from_numpy(np.random.default_rng(i).standard_normal(eps_h.shape).astype(np.float32)).cuda()
        icnf = configs.build(wl, sol_kwargs=configs.README_TOLERANCES)
        m = cnf.TrainMode()
        lam = (icnf.lambda1, icnf.lambda2, icnf.lambda3)
        cot = torch.from_numpy(np.stack([np.full(B, -1.0 / B)] + [np.full(B, v / B) for v in lam]).astype(np.float32)).cuda()
        gx = torch.full((icnf.nvars, B), 1.0 / B, dtype=torch.float32, device="cuda")
        gq = torch.full((B,), 1.0 / B, dtype=torch.float32, device="cuda")
        steps = {}

        def inf():
            cnf.inference_record(icnf, m, xs, flat, {}, eps=eps)
            steps["inf"] = len(icnf.last_steps)
            cnf.inference_pullback(icnf, cot)

        def gen():
            cnf.generate_record(icnf, m, flat, {}, B, z0=z0, eps=eps)
            steps["gen"] = len(icnf.last_steps)
            cnf.generate_pullback(icnf, (gx, gq))

        for fn in (inf, gen):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {"inf": [], "gen": []}
        for _ in range(a.rounds):
            t["inf"].append(_window(inf, a.window))
            t["gen"].append(_window(gen, a.window))
        icnf.close()
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        lines.append(f"{name}: {med['inf']:.3f} | {med['gen']:.3f} | {med['gen'] / med['inf']:.3f} | {steps['inf']} / {steps['gen']}"
                     f"   (rounds: {', '.join(f'{x:.3f}' for x in t['inf'])} | {', '.join(f'{x:.3f}' for x in t['gen'])})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
