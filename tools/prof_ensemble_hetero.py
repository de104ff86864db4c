"""Timings for heterogeneous ensembles (per-member batch size, lambdas, tolerances), B = 32, tspan (0, 13), TrainMode, README
tolerances, on the reference's README network (2-6-2) and its regression network (16-48-16):

    python tools/prof_ensemble_hetero.py homogeneous [--package DIR] [--label NAME] [--rounds 3] [--window 0.4] [--out FILE]
        the HOMOGENEOUS calls -- loss_and_grad_many, inference_many, inference_vjp_many at M = 64 and M = capacity, no new
        argument -- of the package found under DIR (default: this tree).  Run on the parent commit's tree, on this one and on the
        parent's again, in one session, it says what the member prologue costs a call that does not use it, beside the parent's
        own run-to-run spread.  Appends its table to FILE.

    python tools/prof_ensemble_hetero.py ragged [--rounds 3] [--window 0.4] [--out FILE]
        64 members: the ragged call (``counts``) against the rectangular call at max(counts) it replaces, for k-fold-like counts
        (31 / 32) and a skewed set (one member at 32, the others at 1..4); and ``EnsembleDist.rand(1024, ragged=True)`` against the
        default ``rand`` for uniform weights and a one-hot mixture.  Appends its table to FILE.

Every leg is warmed up, then timed over at least ``--window`` seconds with device events around synchronised work; a cell is the
mean over the rounds' means in ms per call, with the lowest and highest round."""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SHAPES = (("README 2-6-2", (2, 6, 2), 1, 1), ("regression 16-48-16", (16, 48, 16), 8, 8))
B = 32
TSPAN = (0.0, 13.0)


def _timed(fn, window, warm=2):
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


def _cell(v):
    import numpy as np
    return f"{np.mean(v):9.3f} ({min(v):.3f}..{max(v):.3f})"


def _model(cnf, dims, nvars, naugs, **kw):
    nn = cnf.Chain(cnf.Dense(dims[0], dims[1], "tanh"), cnf.Dense(dims[1], dims[2], "tanh"))
    return cnf.construct(cnf.RNODE, nn, nvars, naugs, compute_mode=cnf.HIPVecJacMatrixMode(), tspan=TSPAN, lambda3=1e-2, rng=1, **kw)


def _inputs(cnf, icnf, M, nvars, naugs, seed):
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    ps = torch.from_numpy(np.stack([cnf.setup(np.random.default_rng(s), icnf.nn)[0] for s in range(M)])).cuda()
    xs = torch.from_numpy(rng.standard_normal((M, nvars, B)).astype(np.float32)).cuda()
    eps = torch.from_numpy(rng.standard_normal((M, nvars + naugs, B)).astype(np.float32)).cuda()
    cot = torch.from_numpy((rng.standard_normal((M, 4, B)) / B).astype(np.float32)).cuda()
    return ps, xs, eps, cot


def homogeneous(args, cnf, torch, np):
    T = cnf.TrainMode()
    lines = [f"[{args.label}] homogeneous ensemble calls, no new argument: B = {B}, tspan {TSPAN}, TrainMode, {args.rounds} rounds of "
             f"{args.window} s windows per leg, device events; ms per call", f"device: {torch.cuda.get_device_name(0)}"]
    for name, dims, nvars, naugs in SHAPES:
        icnf = _model(cnf, dims, nvars, naugs)
        caps = dict(loss=cnf.ensemble_capacity(icnf, T, B), inference=cnf.ensemble_eval_capacity(icnf, T, B),
                    vjp=cnf.ensemble_vjp_capacity(icnf, T, B))
        lines.append(f"{name}: capacities {caps}")
        lines.append(f"  {'M':>9} {'loss_and_grad_many':>28} {'inference_many':>28} {'inference_vjp_many':>28}")
        for which in (64, "capacity"):
            res, ms = {}, {}
            for leg in ("loss", "inference", "vjp"):
                M = caps[leg] if which == "capacity" else which
                ms[leg] = M
                ps, xs, eps, cot = _inputs(cnf, icnf, M, nvars, naugs, 100 + M)
                cot_arg = (cot[:, 0], (cot[:, 1], cot[:, 2], cot[:, 3]))
                fn = {"loss": lambda: cnf.loss_and_grad_many(icnf, T, xs, ps, {}, eps=eps),
                      "inference": lambda: cnf.inference_many(icnf, T, xs, ps, {}, eps=eps),
                      "vjp": lambda: cnf.inference_vjp_many(icnf, T, xs, ps, {}, cot_arg, eps=eps)}[leg]
                res[leg] = [_timed(fn, args.window) for _ in range(args.rounds)]
            tag = "/".join(str(ms[k]) for k in ("loss", "inference", "vjp")) if which == "capacity" else str(which)
            lines.append(f"  {tag:>9} {_cell(res['loss']):>28} {_cell(res['inference']):>28} {_cell(res['vjp']):>28}")
            print(lines[-1], flush=True)
        icnf.close()
    return lines


def ragged(args, cnf, torch, np):
    T = cnf.TrainMode()
    M = 64
    rng = np.random.default_rng(7)
    sets = (("k-fold (31 / 32)", np.asarray([32 if m % 2 else 31 for m in range(M)], dtype=np.int32)),
            ("skewed (one at 32, others 1..4)", np.concatenate([[32], rng.integers(1, 5, M - 1)]).astype(np.int32)))
    lines = [f"ragged against rectangular calls: {M} members, rectangle B = {B}, tspan {TSPAN}, TrainMode, {args.rounds} rounds of "
             f"{args.window} s windows per leg, device events; ms per call", f"device: {torch.cuda.get_device_name(0)}"]
    for name, dims, nvars, naugs in SHAPES:
        icnf = _model(cnf, dims, nvars, naugs)
        ps, xs, eps, _ = _inputs(cnf, icnf, M, nvars, naugs, 300)
        lines.append(f"{name}")
        lines.append(f"  {'counts':>34} {'live columns':>13} {'call':>20} {'rectangular':>28} {'ragged':>28} {'ragged/rect':>12}")
        for label, counts in sets:
            for call, fn in (("loss_and_grad_many", lambda **kw: cnf.loss_and_grad_many(icnf, T, xs, ps, {}, eps=eps, **kw)),
                             ("inference_many", lambda **kw: cnf.inference_many(icnf, T, xs, ps, {}, eps=eps, **kw))):
                rect, rag = [], []
                for _ in range(args.rounds):
                    rect.append(_timed(lambda: fn(), args.window))
                    rag.append(_timed(lambda: fn(counts=counts), args.window))
                lines.append(f"  {label:>34} {int(counts.sum()):>6}/{M * B:<6} {call:>20} {_cell(rect):>28} {_cell(rag):>28} "
                             f"{np.mean(rag) / np.mean(rect):12.3f}")
                print(lines[-1], flush=True)
        icnf.close()
    n = 1024
    lines.append(f"EnsembleDist.rand({n}) of 64 members, README network, TestMode, tspan {TSPAN}: default (every member at max count "
                 f"columns) against ragged=True")
    lines.append(f"  {'weights':>10} {'default':>28} {'ragged':>28} {'ragged/default':>15}")
    name, dims, nvars, naugs = SHAPES[0]
    icnf = _model(cnf, dims, nvars, naugs)
    ps = _inputs(cnf, icnf, M, nvars, naugs, 300)[0]
    for label, w in (("uniform", None), ("one-hot", [1.0] + [0.0] * (M - 1))):
        d = cnf.EnsembleDist(icnf, cnf.TestMode(), ps, {}, weights=w)
        dflt, rag = [], []
        for _ in range(args.rounds):
            dflt.append(_timed(lambda: d.rand(n), args.window))
            rag.append(_timed(lambda: d.rand(n, ragged=True), args.window))
        lines.append(f"  {label:>10} {_cell(dflt):>28} {_cell(rag):>28} {np.mean(rag) / np.mean(dflt):15.3f}")
        print(lines[-1], flush=True)
    icnf.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("homogeneous", "ragged"))
    ap.add_argument("--package", default=ROOT, help="the tree whose continuousnf.jl_amd is measured (homogeneous)")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_hetero_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import numpy as np
    import torch

    import continuousnf.jl_amd as cnf
    assert os.path.abspath(cnf.__file__).startswith(os.path.abspath(args.package)), cnf.__file__
    lines = (homogeneous if args.what == "homogeneous" else ragged)(args, cnf, torch, np)
    text = "\n".join(lines) + "\n\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
