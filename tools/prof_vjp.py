"""Times the recorded inference + pullback against loss_and_grad, and loss_and_grad against an EARLIER build of the library.

    python tools/prof_vjp.py --parent-lib /path/to/libcnfhip.so [--rounds 2] [--window 1.0] [--out profiles/vjp_timing.txt]

One child process per library, started in alternation by this script (CNFHIP_LIB is read at import; a fresh child each time --
never an exec over a process that has opened the GPU).  Legs, in the order they are run in every round:

    parent-a   loss_and_grad with the parent build                       (i)
    new        loss_and_grad with this build                             (ii)
    parent-b   loss_and_grad with the parent build again                 (i'): (i) against itself = the spread
    vjp        inference_record + inference_pullback, uniform cotangent  (iii)

Every shape is warmed up, then timed over a window of at least `--window` seconds with device events around synchronised
work.  (ii) vs (i) must lie inside the spread of (i) against (i'); (iii) vs (ii) is reported per shape.  Last: one `fit`
iteration with a custom loss against the built-in one, synchronous on both sides (headline network, B = 32): reported only --
the autograd round trip is host time.  Without --parent-lib only `new`, `vjp` and the fit leg run.

Which kernel pays for a difference: one leg under the profiler, in a run of its own,
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prof_vjp.py --child vjp --only "cfg3 B=8192" --calls 200
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = (("cfg3 B=8192", 3, 8192, False, "train"), ("cfg3 B=32", 3, 32, False, "train"), ("cfg5 B=2048", 5, 2048, False, "train"),
          ("cfg3 JVP B=8192", 3, 8192, True, "train"), ("TestMode 32-128-128-32 B=256", 3, 256, False, "test"))


CALLS = 0          # --calls n: exactly n calls after the warm-up instead of a timed window (a child under a profiler)


def _timed(fn, window):
    """ms per call: warm-up, then calls until `window` seconds of device time have passed (device events around the loop)."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    if CALLS:
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        return dict(ms=float("nan"), n=CALLS)
    n, total = 0, 0.0
    per = []
    while total < window * 1e3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(4):
            fn()
        b.record()
        torch.cuda.synchronize()
        dt = a.elapsed_time(b)
        per.append(dt / 4)
        total += dt
        n += 4
    per.sort()
    return dict(ms=total / n, median=per[len(per) // 2], lo=per[0], hi=per[-1], n=n)


def child(leg, window):
    import numpy as np
    import torch
    from continuousnf.jl_amd import _lib
    if leg.startswith("parent"):                     # (an earlier build does not export the entry points added since)
        import ctypes
        l = ctypes.CDLL(_lib.LIB_PATH)
        for table in (_lib._SIGNATURES, _lib._SAMPLING_SIGNATURES):
            for name in list(table):
                if not hasattr(l, name):
                    table.pop(name)
    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import configs
    out = {"leg": leg, "lib": _lib.LIB_PATH, "shapes": {}}
    for name, i, B, jvp, mode in SHAPES:
        wl = configs.BASELINE[i]
        flat = torch.from_numpy(configs.glorot_params(wl.dims, i, 0.05)).cuda()
        xs_h, eps_h = configs.synthetic_inputs(wl, B, i)
        xs, eps = torch.from_numpy(xs_h).cuda(), torch.from_numpy(eps_h).cuda()
        icnf = configs.build(wl, jvp=jvp, sol_kwargs=configs.README_TOLERANCES)
        m = cnf.TrainMode() if mode == "train" else cnf.TestMode()
        kw = dict(eps=eps) if mode == "train" else {}
        if leg == "vjp":
            lam = (icnf.lambda1, icnf.lambda2, icnf.lambda3) if mode == "train" else (0.0, 0.0, 0.0)
            cot = torch.from_numpy(np.stack([np.full(B, -1.0 / B)] + [np.full(B, v / B) for v in lam]).astype(np.float32)).cuda()

            def fn():
                cnf.inference_record(icnf, m, xs, flat, {}, **kw)
                cnf.inference_pullback(icnf, cot)
        else:
            def fn():
                cnf.loss_and_grad(icnf, m, xs, flat, {}, **kw)
        out["shapes"][name] = _timed(fn, window)
        icnf.close()
    if leg == "fit":
        out["shapes"] = {}
        from continuousnf.jl_amd import mlj
        import time

        def restated(ic, mode_, x, *args):
            logpx, (E, n, A) = cnf.differentiable_inference(ic, mode_, x, *args)
            return (-logpx + ic.lambda1 * E + ic.lambda2 * n + ic.lambda3 * A).mean()

        r = np.random.default_rng(0).beta(2.0, 4.0, size=(1024, 32)).astype(np.float32)
        for tag, loss in (("built-in loss, synchronous", None), ("custom loss (autograd)", restated)):
            nn = cnf.Chain(*[cnf.Dense(a, b, "tanh") for a, b in zip((32, 128, 128), (128, 128, 32))])
            icnf = cnf.construct(cnf.RNODE, nn, 32, 0, compute_mode=cnf.HIPVecJacMatrixMode(), tspan=(0.0, 1.0), rng=1,
                                 sol_kwargs=configs.README_TOLERANCES)
            mlj.fit(mlj.ICNFModel(icnf, loss, n_epochs=1, pipelined=False), 0, r)
            t0 = time.perf_counter()
            _, _, rep = mlj.fit(mlj.ICNFModel(icnf, loss, n_epochs=3, pipelined=False), 0, r)
            el = time.perf_counter() - t0
            out["shapes"][tag] = dict(ms=el / rep["stats"]["iterations"] * 1e3, n=rep["stats"]["iterations"])
            icnf.close()
    print("PROF_VJP " + json.dumps(out), flush=True)


ONLY = None


def run_child(leg, lib, window):
    env = dict(os.environ)
    if lib:
        env["CNFHIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("CNFHIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--window", str(window)] +
                       (["--only", ONLY] if ONLY else []), env=env,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"child {leg} ended with status {r.returncode}")
    line = [l for l in r.stdout.splitlines() if l.startswith("PROF_VJP ")][-1]
    return json.loads(line[len("PROF_VJP "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out")
    ap.add_argument("--only", help="only the shapes whose name contains this")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--calls", type=int, default=0, help="with --child: exactly this many calls per shape (for a profiler run)")
    ap.add_argument("--child")
    a = ap.parse_args()
    global SHAPES, CALLS
    CALLS = a.calls
    if a.only:
        SHAPES = tuple(sh for sh in SHAPES if a.only in sh[0])
    if a.child:
        if a.child == "fit":
            SHAPES = ()
        return child(a.child, a.window)
    global ONLY
    ONLY = a.only
    legs = (["parent-a", "new", "parent-b", "vjp"] if a.parent_lib else ["new", "vjp"])
    res = {l: {} for l in legs}
    for _ in range(a.rounds):
        for leg in legs:                             # the legs alternate: one child each, one at a time
            out = run_child(leg, a.parent_lib if leg.startswith("parent") else None, a.window)
            for shape, v in out["shapes"].items():
                res[leg].setdefault(shape, []).append(v["ms"])
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])
    lines = [f"# tools/prof_vjp.py: ms per call, {a.rounds} rounds, window {a.window} s per leg and shape; all rounds listed"]
    for name, *_ in SHAPES:
        row = {l: res[l].get(name, []) for l in legs}
        s = f"{name}: " + "; ".join(f"{l} {med(v):.3f} ({', '.join(f'{x:.3f}' for x in v)})" for l, v in row.items() if v)
        if a.parent_lib:
            pa, pb, nw = med(row["parent-a"]), med(row["parent-b"]), med(row["new"])
            s += f" | new/parent {nw / (0.5 * (pa + pb)):.4f}, parent-b/parent-a {pb / pa:.4f}"
        s += f" | vjp/new {med(row['vjp']) / med(row['new']):.4f}"
        lines.append(s)
    fit = {"shapes": {}} if a.no_fit else run_child("fit", None, a.window)
    for tag, v in fit["shapes"].items():
        lines.append(f"fit iteration, headline network B=32, {tag}: {v['ms']:.3f} ms per iteration ({v['n']} iterations)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
