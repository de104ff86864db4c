"""Times loss_and_grad of conditional models with and without the gradient w.r.t. ys, and the switch-off path against an EARLIER
build of the library.

    python tools/prof_cond_grad.py --parent-lib /path/to/libcnfhip.so [--rounds 3] [--window 1.0] [--out profiles/cond_grad_timing.txt]

One child process per library, started in alternation by this script (CNFHIP_LIB is read at import; a fresh child each time --
never an exec over a process that has opened the GPU).  Legs, in the order they are run in every round:

    parent-a   loss_and_grad with the parent build                       (i)
    off        loss_and_grad with this build, the switch off             (ii)
    parent-b   loss_and_grad with the parent build again                 (i'): (i) against itself = the spread
    ys         loss_and_grad(with_ys=True) with this build               (iii)

Every shape is warmed up, then timed over a window of at least `--window` seconds with device events around synchronised
work; medians over the rounds.  (ii) / (i) must lie inside the spread (i') / (i); (iii) / (ii) is reported beside the byte
model: k_cond_rowsum streams 6 steps B dims[1] 4 bytes per pullback, k_wgrad_wave 12 (sum_in + sum_out) as many per sample.
Without --parent-lib only `off` and `ys` run.

k_cond_rowsum on its own: one leg under the profiler, in a run of its own,
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prof_cond_grad.py --child ys --only "B=8192" --calls 50
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

#          name                              dims (first entry: n_in + n_cond)   nvars naugs B
SHAPES = (("CondRNODE 32+8-128-128-32 B=8192", (40, 128, 128, 32), 32, 0, 8192),
          ("CondRNODE 32+8-128-128-32 B=32", (40, 128, 128, 32), 32, 0, 32),
          ("CondRNODE 128+16-384-128 B=2048", (144, 384, 128), 64, 64, 2048))
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
    n, total, per = 0, 0.0, []
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
    parent = leg.startswith("parent")
    if parent:                                       # (an earlier build does not export the entry points added since)
        import ctypes
        l = ctypes.CDLL(_lib.LIB_PATH)
        for table in (_lib._SIGNATURES, _lib._SAMPLING_SIGNATURES):
            for name in list(table):
                if not hasattr(l, name):
                    table.pop(name)
    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import base_icnf, configs
    if parent:                                       # ... and has no switch to set
        base_icnf.set_grad_ys = lambda icnf, with_ys: None
    out = {"leg": leg, "lib": _lib.LIB_PATH, "shapes": {}}
    for i, (name, dims, nvars, naugs, B) in enumerate(SHAPES):
        n_in = nvars + naugs
        rng = np.random.default_rng(100 + i)
        flat = torch.from_numpy(configs.glorot_params(dims, 100 + i, 0.05)).cuda()
        xs = torch.from_numpy(rng.standard_normal((nvars, B)).astype(np.float32)).cuda()
        eps = torch.from_numpy(rng.standard_normal((n_in, B)).astype(np.float32)).cuda()
        ys = torch.from_numpy(rng.standard_normal((dims[0] - n_in, B)).astype(np.float32)).cuda()
        nn = cnf.Chain(*[cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])])
        icnf = cnf.construct(cnf.CondRNODE, nn, nvars, naugs, compute_mode=cnf.HIPVecJacMatrixMode(), tspan=(0.0, 1.0),
                             lambda1=1e-2, lambda2=1e-2, lambda3=1e-2 if naugs else 0.0, sol_kwargs=configs.README_TOLERANCES, rng=0)
        kw = dict(with_ys=True) if leg == "ys" else {}

        def fn():
            cnf.loss_and_grad(icnf, cnf.TrainMode(), xs, ys, flat, {}, eps=eps, **kw)
        res = _timed(fn, window)
        res["steps"] = int(len(icnf.last_steps))
        out["shapes"][name] = res
        icnf.close()
    print("PROF_COND " + json.dumps(out), flush=True)


ONLY = None


def run_child(leg, lib, window):
    env = dict(os.environ)
    if lib:
        env["CNFHIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("CNFHIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--window", str(window)] +
                       (["--only", ONLY] if ONLY else []), env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"child {leg} ended with status {r.returncode}")
    line = [l for l in r.stdout.splitlines() if l.startswith("PROF_COND ")][-1]
    return json.loads(line[len("PROF_COND "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out")
    ap.add_argument("--only", help="only the shapes whose name contains this")
    ap.add_argument("--calls", type=int, default=0, help="with --child: exactly this many calls per shape (for a profiler run)")
    ap.add_argument("--child")
    a = ap.parse_args()
    global SHAPES, CALLS, ONLY
    CALLS = a.calls
    if a.only:
        SHAPES = tuple(sh for sh in SHAPES if a.only in sh[0])
    if a.child:
        return child(a.child, a.window)
    ONLY = a.only
    legs = ["parent-a", "off", "parent-b", "ys"] if a.parent_lib else ["off", "ys"]
    res, steps = {l: {} for l in legs}, {}
    for _ in range(a.rounds):
        for leg in legs:                             # the legs alternate: one child each, one at a time
            out = run_child(leg, a.parent_lib if leg.startswith("parent") else None, a.window)
            for shape, v in out["shapes"].items():
                res[leg].setdefault(shape, []).append(v["ms"])
                steps[shape] = v["steps"]
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])
    lines = [f"# tools/prof_cond_grad.py: ms per call, {a.rounds} rounds, window {a.window} s per leg and shape; median (all rounds)"]
    for name, dims, nvars, naugs, B in SHAPES:
        row = {l: res[l].get(name, []) for l in legs}
        s = f"{name} ({steps[name]} steps): " + "; ".join(f"{l} {med(v):.3f} ({', '.join(f'{x:.3f}' for x in v)})" for l, v in row.items() if v)
        if a.parent_lib:
            pa, pb, off = med(row["parent-a"]), med(row["parent-b"]), med(row["off"])
            s += f" | off/parent-a {off / pa:.4f}, parent-b/parent-a {pb / pa:.4f}"
        sum_in, sum_out = sum(dims[:-1]), sum(dims[1:])
        s += f" | ys/off {med(row['ys']) / med(row['off']):.4f} (byte model: rowsum reads {dims[1] / (2.0 * (sum_in + sum_out)):.3f} of what the contraction reads)"
        lines.append(s)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
