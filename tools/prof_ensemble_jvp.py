"""Times ``inference_jvp_many`` (M members' tangents in two launches) against a loop of M single ``inference_jvp`` calls on an
EARLIER build of the library, and the calls that existed before -- ``inference_jvp``, ``inference_many``, ``generate_many`` -- on
both builds.

    python tools/prof_ensemble_jvp.py --parent-lib /path/to/libcnfhip.so [--rounds 3] [--window 0.3] [--out profiles/ensemble_jvp_timing.txt]

The method of tools/prof_jvp.py: one child process per library, started in alternation by this script (CNFHIP_LIB is read at
import; a fresh child each time -- never an exec over a process that has opened the GPU; every child under a time limit); every
leg is warmed up, then timed over a window of device time with device events around synchronised work.  Legs of a round, in order:

    parent   (i)  the existing calls: inference_jvp at R = 1, 8, 32 | a LOOP of 64 inference_jvp calls over 64 members' own inputs |
                  inference_many and generate_many at M = 64                                    with the parent build
    new           the same existing calls with this build | inference_jvp_many at M = 1, 64 and the capacity with R = 1, 8, 32 |
                  generate_jvp_many at M = 64, R = 8 | loss_jvp_many with the n_params one-hot directions at M = 64 (n_params <= 64)
    parent-b (i') the parent legs again: (i') / (i) = the spread of the parent against itself

Shapes: the README network (2-6-2) and 16-48-16, B = 32, tspan (0, 13), TrainMode / VJP, the README tolerances.  The loop at the
capacity is not run (thousands of synchronous calls per sample): it is M x the single call, and is reported as such.
Reported: the median over the rounds with the lowest and highest round.  Without --parent-lib the parent legs run on this build.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = (("2-6-2", 1), ("16-48-16", 2))
B = 32
RS = (1, 8, 32)
M_LOOP = 64
CHILD_LIMIT = 420                                          # seconds a child may take


def _timed(fn, window):
    """ms per call: warm-up, then calls until `window` seconds of device time have passed (device events around the loop)."""
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    n, total = 0, 0.0
    while total < window * 1e3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(2):
            fn()
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
        n += 2
    return total / n


def child(leg, window):
    import dataclasses

    import numpy as np
    import torch
    from continuousnf.jl_amd import _lib
    parent = leg.startswith("parent")
    if parent:                                             # (an earlier build does not export the entry points added since)
        import ctypes
        l = ctypes.CDLL(_lib.LIB_PATH)
        for table in [getattr(_lib, n) for n in dir(_lib) if n.endswith("_SIGNATURES")]:
            for name in list(table):
                if not hasattr(l, name):
                    table.pop(name)
    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import configs
    out = {"leg": leg, "lib": _lib.LIB_PATH, "ms": {}, "cap": {}}
    T = cnf.TrainMode()
    for name, i in SHAPES:
        wl = dataclasses.replace(configs.BASELINE[i], tspan=(0.0, 13.0))
        icnf = configs.build(wl, sol_kwargs=configs.README_TOLERANCES)
        cap = cnf.ensemble_eval_capacity(icnf, T, B)
        out["cap"][name] = cap
        Mmax = M_LOOP if parent else max(cap, M_LOOP)
        g = torch.Generator(device="cuda").manual_seed(1)
        ps = torch.from_numpy(np.stack([configs.glorot_params(wl.dims, 100 + m, 0.05) for m in range(M_LOOP)])).cuda()
        ps = ps.repeat((Mmax + M_LOOP - 1) // M_LOOP, 1)[:Mmax].contiguous()       # (beyond 64 members the parameters repeat)
        n = ps.shape[1]
        xs_h, eps_h = configs.synthetic_inputs(wl, B, i)
        xs = torch.from_numpy(xs_h).cuda()[None] + 0.05 * torch.randn(Mmax, *xs_h.shape, device="cuda", generator=g)
        eps = torch.randn(Mmax, *eps_h.shape, device="cuda", generator=g)
        z0 = torch.randn(Mmax, *eps_h.shape, device="cuda", generator=g)
        dirs = {R: torch.randn(Mmax, R, n, device="cuda", generator=g) for R in RS}
        legs = {}
        for R in RS:
            legs[f"inference_jvp R={R}"] = (lambda R=R: cnf.inference_jvp(icnf, T, xs[0], ps[0], {}, d_ps=dirs[R][0], eps=eps[0]))

            def loop(R=R):
                for m in range(M_LOOP):
                    cnf.inference_jvp(icnf, T, xs[m], ps[m], {}, d_ps=dirs[R][m], eps=eps[m])
            if parent:
                legs[f"loop of {M_LOOP} inference_jvp R={R}"] = loop
        legs[f"inference_many M={M_LOOP}"] = lambda: cnf.inference_many(icnf, T, xs[:M_LOOP], ps[:M_LOOP], {}, eps=eps[:M_LOOP])
        legs[f"generate_many M={M_LOOP}"] = lambda: cnf.generate_many(icnf, T, ps[:M_LOOP], {}, B, z0=z0[:M_LOOP], eps=eps[:M_LOOP], with_logp=True)
        if not parent:
            for M in (1, M_LOOP, cap):
                for R in RS:
                    legs[f"inference_jvp_many M={'cap' if M == cap else M} R={R}"] = \
                        (lambda M=M, R=R: cnf.inference_jvp_many(icnf, T, xs[:M], ps[:M], {}, d_ps=dirs[R][:M], eps=eps[:M]))
            legs[f"generate_jvp_many M={M_LOOP} R=8"] = lambda: cnf.generate_jvp_many(icnf, T, ps[:M_LOOP], {}, B, d_ps=dirs[8][:M_LOOP],
                                                                                    z0=z0[:M_LOOP], eps=eps[:M_LOOP])
            if n <= 64:
                eye = torch.eye(n, device="cuda").expand(M_LOOP, n, n).contiguous()
                legs[f"loss_jvp_many one-hot M={M_LOOP} R={n}"] = lambda: cnf.loss_jvp_many(icnf, T, xs[:M_LOOP], ps[:M_LOOP], {}, d_ps=eye,
                                                                                           eps=eps[:M_LOOP])
        for tag, fn in legs.items():
            out["ms"][f"{name} | {tag}"] = _timed(fn, window)
        icnf.close()
    print("PROF_ENSEMBLE_JVP " + json.dumps(out), flush=True)


def run_child(leg, lib, window):
    env = dict(os.environ)
    if lib:
        env["CNFHIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("CNFHIP_LIB", None)
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", leg, "--window", str(window)],
                       env=env, capture_output=True, text=True)
    if r.returncode != 0:                                  # (a child that failed ends the run: nothing more is started on the device)
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"child {leg} ended with status {r.returncode}")
    line = [l for l in r.stdout.splitlines() if l.startswith("PROF_ENSEMBLE_JVP ")][-1]
    return json.loads(line[len("PROF_ENSEMBLE_JVP "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.window)
    res, caps = {}, {}
    for _ in range(a.rounds):
        for leg in ("parent", "new", "parent-b"):          # the legs alternate: one child each, one at a time
            out = run_child(leg, a.parent_lib if leg.startswith("parent") else None, a.window)
            caps.update(out["cap"] if leg == "new" else {})
            for k, v in out["ms"].items():
                res.setdefault((leg, k), []).append(v)
    med = lambda v: sorted(v)[len(v) // 2]
    fmt = lambda v: f"{med(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
    lines = [f"# tools/prof_ensemble_jvp.py: ms per call, median of {a.rounds} rounds (lowest .. highest), window {a.window} s per leg; B = {B}, "
             f"tspan (0, 13), TrainMode / VJP, README tolerances; parent legs on {'the parent build' if a.parent_lib else 'THIS build'}"]
    for name, _ in SHAPES:
        cap = caps.get(name, 0)
        row = lambda leg, tag: res.get((leg, f"{name} | {tag}"))
        lines.append(f"{name} (capacity {cap} members at B = {B})")
        lines.append("  the calls that existed before: parent (i) | this build | parent again (i'); this build / (i), (i') / (i)")
        for tag in [f"inference_jvp R={R}" for R in RS] + [f"inference_many M={M_LOOP}", f"generate_many M={M_LOOP}"]:
            p, nw, pb = row("parent", tag), row("new", tag), row("parent-b", tag)
            lines.append(f"    {tag}: {fmt(p)} | {fmt(nw)} | {fmt(pb)}; {med(nw) / med(p):.3f}, {med(pb) / med(p):.3f}")
        lines.append(f"  inference_jvp_many against the loop of single calls on the parent build (M = {M_LOOP}: measured; the capacity: M x the single call)")
        for R in RS:
            one, loop = row("parent", f"inference_jvp R={R}"), row("parent", f"loop of {M_LOOP} inference_jvp R={R}")
            lines.append(f"    R={R}: single {fmt(one)}; loop of {M_LOOP} {fmt(loop)}")
            for M, tagM in ((1, "1"), (M_LOOP, str(M_LOOP)), (cap, "cap")):
                v = row("new", f"inference_jvp_many M={tagM} R={R}")
                base = med(one) if M == 1 else med(loop) if M == M_LOOP else med(one) * M
                lines.append(f"      M={M}: {fmt(v)} = {med(v) / med(one):.2f} x one single call, loop / many = {base / med(v):.1f}")
        for (leg, k), v in res.items():
            if leg == "new" and k.startswith(name + " | ") and ("generate_jvp_many" in k or "loss_jvp_many" in k):
                lines.append(f"  {k.split(' | ')[1]}: {fmt(v)}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
