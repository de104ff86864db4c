"""Times the gradient entry points of this build against an EARLIER one, the sampling direction (generate_record +
generate_pullback) first of all: what tools/prof_vjp.py does for loss_and_grad, with its shapes, warm-up and timed window.
(tools/prof_gen_vjp.py compares the two directions within ONE build.)

    python tools/prof_grad_ab.py --parent-lib /path/to/libcnfhip.so [--rounds 3] [--window 1.0] [--out FILE]
    python tools/prof_grad_ab.py --parent-tree /path/to/checkout --what loss,vjp,gen --only "B=32" ...

--parent-lib: this tree's Python over the parent's library -- the library alone.  --parent-tree: a built checkout of the parent
with its own library against this tree -- the Python layer included (the small batches are where host time is a visible share).
Legs parent-a, new, parent-b, alternated, one fresh child process each (never an exec over a process that has opened the GPU);
parent-b against parent-a is the spread a ratio new/parent has to be read against.  --what: gen (the default), vjp
(inference_record + inference_pullback) and loss (loss_and_grad), each timed per shape.  --out appends.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def child(tree, what, only, window):
    sys.path.insert(0, tree)                          # the package of the tree under test; the timing loop is this tool's
    sys.path.insert(1, HERE)
    import ctypes
    import numpy as np
    import torch
    from continuousnf.jl_amd import _lib            # (first: prof_vjp puts ITS tree in front of the path)
    import prof_vjp
    l = ctypes.CDLL(_lib.LIB_PATH)
    for table in (_lib._SIGNATURES, _lib._SAMPLING_SIGNATURES):       # (an earlier build may not export every entry point)
        for name in list(table):
            if not hasattr(l, name):
                table.pop(name)
    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import configs
    out = {}
    for name, i, B, jvp, mode in prof_vjp.SHAPES:
        if only and only not in name:
            continue
        wl = configs.BASELINE[i]
        flat = torch.from_numpy(configs.glorot_params(wl.dims, i, 0.05)).cuda()
        xs_h, eps_h = configs.synthetic_inputs(wl, B, i)
        xs, eps = torch.from_numpy(xs_h).cuda(), torch.from_numpy(eps_h).cuda()
        icnf = configs.build(wl, jvp=jvp, sol_kwargs=configs.README_TOLERANCES)
        m = cnf.TrainMode() if mode == "train" else cnf.TestMode()
        kw = dict(eps=eps) if mode == "train" else {}
        rng = np.random.default_rng(i)
        z0 = torch.from_numpy(rng.standard_normal(eps_h.shape).astype(np.float32)).cuda()
        cot = torch.full((4, B), 1.0 / B, device="cuda")
        cz, cl = torch.full(tuple(eps.shape), 1.0 / B, device="cuda"), torch.full((B,), 1.0 / B, device="cuda")

        def gen():
            cnf.generate_record(icnf, m, flat, None, B, z0=z0, **kw)
            cnf.generate_pullback(icnf, (cz, cl), with_z0=True)

        def vjp():
            cnf.inference_record(icnf, m, xs, flat, {}, **kw)
            cnf.inference_pullback(icnf, cot, with_x=True)

        def loss():
            cnf.loss_and_grad(icnf, m, xs, flat, {}, with_x=True, **kw)
        for w in what:
            out[f"{w} {name}"] = prof_vjp._timed(dict(gen=gen, vjp=vjp, loss=loss)[w], window)["ms"]
        icnf.close()
    print("PROF_AB " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent-tree")
    ap.add_argument("--what", default="gen")
    ap.add_argument("--only")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    what = a.what.split(",")
    if a.child:
        return child(a.child, what, a.only, a.window)
    if bool(a.parent_lib) == bool(a.parent_tree):
        raise SystemExit("one of --parent-lib and --parent-tree")
    root = os.path.abspath(os.path.join(HERE, ".."))
    res = {}
    for _ in range(a.rounds):
        for leg in ("parent-a", "new", "parent-b"):
            env = dict(os.environ)
            env.pop("CNFHIP_LIB", None)
            tree = root
            if leg != "new" and a.parent_lib:
                env["CNFHIP_LIB"] = os.path.abspath(a.parent_lib)
            elif leg != "new":
                tree = os.path.abspath(a.parent_tree)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--what", a.what, "--window", str(a.window)] +
                               (["--only", a.only] if a.only else []), env=env, cwd=tree, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
                raise SystemExit(f"child {leg} ended with status {r.returncode}")
            line = [x for x in r.stdout.splitlines() if x.startswith("PROF_AB ")][-1]
            for k, v in json.loads(line[len("PROF_AB "):]).items():
                res.setdefault(k, {}).setdefault(leg, []).append(v)
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])
    against = f"--parent-lib {a.parent_lib} (the library alone)" if a.parent_lib else "--parent-tree (Python layer included)"
    lines = [f"# tools/prof_grad_ab.py {against}: ms per call, {a.rounds} rounds, window {a.window} s per leg and shape; all rounds listed"]
    for k, legs in res.items():
        pa, pb, nw = med(legs["parent-a"]), med(legs["parent-b"]), med(legs["new"])
        lines.append(f"{k}: " + "; ".join(f"{leg} {med(v):.3f} ({', '.join(f'{x:.3f}' for x in v)})" for leg, v in legs.items()) +
                     f" | new/parent {nw / (0.5 * (pa + pb)):.4f}, parent-b/parent-a {pb / pa:.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
