"""Times ``inference_jvp`` at R = 1, 8, 32 directions against ``inference`` alone and against ``inference_record`` +
``inference_pullback`` (both baselines on an EARLIER build of the library), and ``loss_and_grad`` beside them.

    python tools/prof_jvp.py --parent-lib /path/to/libcnfhip.so [--rounds 3] [--window 0.5] [--out profiles/jvp_timing.txt]

The method of tools/prof_vjp.py: one child process per library, started in alternation by this script (CNFHIP_LIB is read at
import; a fresh child each time -- never an exec over a process that has opened the GPU); every leg is warmed up, then timed over
a window of device time with device events around synchronised work.  Legs of a round, in order:

    parent   inference | inference_record + inference_pullback | loss_and_grad     with the parent build
    new      inference_jvp at R = 1, 8, 32 (directions of ps) | loss_jvp with the n_params one-hot directions where n_params <= 64
    parent-b the parent legs again: against the first = the spread

Shapes: the README network (2-6-2) and 16-48-16, tspan (0, 13), TrainMode / VJP, the README tolerances, B = 32 and B = 4096.
Reported: the median over the rounds with the lowest and highest round.  Without --parent-lib the parent legs run on this build.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = (("2-6-2 B=32", 1, 32), ("2-6-2 B=4096", 1, 4096), ("16-48-16 B=32", 2, 32), ("16-48-16 B=4096", 2, 4096))
RS = (1, 8, 32)


def _timed(fn, window):
    """ms per call: warm-up, then calls until `window` seconds of device time have passed (device events around the loop)."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
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


def child(leg, window):
    import dataclasses

    import numpy as np
    import torch
    from continuousnf.jl_amd import _lib
    if leg.startswith("parent"):                     # (an earlier build does not export the entry points added since)
        import ctypes
        l = ctypes.CDLL(_lib.LIB_PATH)
        for table in [getattr(_lib, n) for n in dir(_lib) if n.endswith("_SIGNATURES")]:
            for name in list(table):
                if not hasattr(l, name):
                    table.pop(name)
    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import configs
    out = {"leg": leg, "lib": _lib.LIB_PATH, "ms": {}}
    T = cnf.TrainMode()
    for name, i, B in SHAPES:
        wl = dataclasses.replace(configs.BASELINE[i], tspan=(0.0, 13.0))
        flat = torch.from_numpy(configs.glorot_params(wl.dims, i, 0.05)).cuda()
        xs_h, eps_h = configs.synthetic_inputs(wl, B, i)
        xs, eps = torch.from_numpy(xs_h).cuda(), torch.from_numpy(eps_h).cuda()
        icnf = configs.build(wl, sol_kwargs=configs.README_TOLERANCES)
        n = flat.numel()
        legs = {}
        if leg.startswith("parent"):
            cot = torch.from_numpy(np.stack([np.full(B, -1.0 / B)] + [np.full(B, v / B) for v in wl.lambdas]).astype(np.float32)).cuda()

            def rec():
                cnf.inference_record(icnf, T, xs, flat, {}, eps=eps)
                cnf.inference_pullback(icnf, cot)
            legs = {"inference": lambda: cnf.inference(icnf, T, xs, flat, {}, eps=eps), "record+pullback": rec,
                    "loss_and_grad": lambda: cnf.loss_and_grad(icnf, T, xs, flat, {}, eps=eps)}
        else:
            g = torch.Generator(device="cuda").manual_seed(1)
            for R in RS:
                d = torch.randn(R, n, device="cuda", generator=g)
                legs[f"jvp R={R}"] = (lambda d=d: cnf.inference_jvp(icnf, T, xs, flat, {}, d_ps=d, eps=eps))
            if n <= 64:
                eye = torch.eye(n, device="cuda")
                legs[f"loss_jvp one-hot R={n}"] = lambda: cnf.loss_jvp(icnf, T, xs, flat, {}, d_ps=eye, eps=eps)
        for tag, fn in legs.items():
            out["ms"][f"{name} | {tag}"] = _timed(fn, window)
        icnf.close()
    print("PROF_JVP " + json.dumps(out), flush=True)


def run_child(leg, lib, window):
    env = dict(os.environ)
    if lib:
        env["CNFHIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("CNFHIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--window", str(window)], env=env,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"child {leg} ended with status {r.returncode}")
    line = [l for l in r.stdout.splitlines() if l.startswith("PROF_JVP ")][-1]
    return json.loads(line[len("PROF_JVP "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.window)
    res = {}
    for _ in range(a.rounds):
        for leg in ("parent", "new", "parent-b"):    # the legs alternate: one child each, one at a time
            out = run_child(leg, a.parent_lib if leg.startswith("parent") else None, a.window)
            for k, v in out["ms"].items():
                res.setdefault((leg, k), []).append(v)
    med = lambda v: sorted(v)[len(v) // 2]
    lines = [f"# tools/prof_jvp.py: ms per call, median of {a.rounds} rounds (lowest .. highest), window {a.window} s per leg; "
             f"tspan (0, 13), TrainMode / VJP, README tolerances; parent legs on {'the parent build' if a.parent_lib else 'THIS build'}"]
    for name, _, _ in SHAPES:
        row = lambda leg, tag: res.get((leg, f"{name} | {tag}"))
        fmt = lambda v: f"{med(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
        inf, rp, lg = row("parent", "inference"), row("parent", "record+pullback"), row("parent", "loss_and_grad")
        lines.append(f"{name}: inference {fmt(inf)} [again {fmt(row('parent-b', 'inference'))}]; record+pullback {fmt(rp)} "
                     f"[again {fmt(row('parent-b', 'record+pullback'))}]; loss_and_grad {fmt(lg)} [again {fmt(row('parent-b', 'loss_and_grad'))}]")
        for (leg, k), v in res.items():
            if leg == "new" and k.startswith(name + " | "):
                lines.append(f"    {k.split(' | ')[1]}: {fmt(v)} = {med(v) / med(inf):.2f} x inference, {med(v) / med(rp):.2f} x record+pullback, "
                             f"{med(v) / med(lg):.2f} x loss_and_grad")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
