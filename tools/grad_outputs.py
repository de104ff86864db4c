"""Every gradient entry point once per case, every output array into one .npz: what two builds of the package are compared on.

    python tools/grad_outputs.py --out FILE.npz

Per case and mode: loss_and_grad (device tensors, then host arrays) with d / d xs and, for a conditional model, d / d ys;
inference_record + inference_pullback; generate_record + generate_pullback; loss_and_grad_submit / collect; and on a second
model with a LearnableNormal base the first three again with the base's gradient.  A call the package refuses with
NotImplementedError is listed under "refused" (both builds must refuse the same ones).  Everything is seeded: two runs of one
build give the same file bit for bit, and so must two builds that compute the same thing.  Under a profiler
(rocprofv3 --kernel-trace -- python tools/grad_outputs.py --out ...) the ordered kernel list is the second thing to compare;
`--compare A.npz B.npz` and `--compare-traces A.csv B.csv` do both comparisons.
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CASES = ("wave-6x18-B40-cond", "adj3-28x128x128-cond", "mfma-12x64x48-cond-vjp", "mfma-12x64x48-cond-jvp", "generic-cfg2")


def _arrays(x):
    import torch
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in _arrays(y)]
    if torch.is_tensor(x):
        return [x.detach().cpu().numpy().copy()]
    return [np.asarray(x, dtype=np.float32).copy()]


def _models():
    """(name, modes, make(basedist) -> icnf, (flat, xs, eps, ys) as float32 host arrays)"""
    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import configs
    from tests import grad_terms as GT, helpers
    for name in CASES:
        case = GT.GPU_CASES[name]

        def make(basedist, case=case):
            net = case.net
            layers = [cnf.Dense(a, b, helpers.ACT_NAME[k]) for a, b, k in zip(net.dims[:-1], net.dims[1:], net.acts)]
            cm = cnf.HIPJacVecMatrixMode(case.kernel) if case.jvp else cnf.HIPVecJacMatrixMode(case.kernel)
            return cnf.construct(cnf.CondRNODE if case.n_cond else cnf.RNODE, cnf.Chain(*layers), case.nvars, case.naugs, compute_mode=cm,
                                 tspan=case.tspan, lambda1=1.0, lambda2=1.0, lambda3=1.0 if case.naugs else 0.0,
                                 sol_kwargs=case.sol_kw, rng=0, basedist=basedist)
        yield name, ("train", "test"), make, case.inputs()

    def deep(basedist):          # the lifecycle suite's deep network: the generic TestMode adjoint behind a recorded solve
        dims, acts = (6, 24, 24, 6), ("tanh", "tanh", "identity")
        nn = cnf.Chain(*[cnf.Dense(i, o, a) for i, o, a in zip(dims[:-1], dims[1:], acts)])
        return cnf.construct(cnf.RNODE, nn, 4, 2, compute_mode=cnf.HIPVecJacMatrixMode("auto"), lambda3=1e-2,
                             sol_kwargs=dict(configs.README_TOLERANCES), rng=0, basedist=basedist)
    rng = np.random.default_rng(24032)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    yield "lifecycle-deep-6x24x24", ("test",), deep, ((0.3 * f32(6 * 24 + 24 + 24 * 24 + 24 + 24 * 6 + 6)), f32(4, 32), f32(6, 32), None)


def run(out_path):
    import torch
    import continuousnf.jl_amd as cnf
    out, refused = {}, []

    def keep(tag, call):
        try:
            res = call()
        except NotImplementedError:
            refused.append(tag)
            return None
        for i, a in enumerate(_arrays(res)):
            out[f"{tag}/{i}"] = a
        return res

    for name, modes, make, (flat, xs, eps, ys) in _models():
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        n_in, B = eps.shape
        rng = np.random.default_rng(len(name) + B)
        cot = rng.standard_normal((4, B)).astype(np.float32)
        cz, cl = rng.standard_normal((n_in, B)).astype(np.float32), rng.standard_normal(B).astype(np.float32)
        cond = ys is not None
        for with_base in (False, True):
            base = None
            if with_base:
                base = cnf.LearnableNormal(torch.linspace(-0.2, 0.3, n_in).cuda(), std=torch.linspace(0.7, 1.4, n_in).cuda())
            ic = make(base)
            for mode_name in modes:
                mode = cnf.TrainMode() if mode_name == "train" else cnf.TestMode()
                tag = f"{name}/{mode_name}/{'base' if with_base else 'plain'}"
                kw = dict(eps=dev(eps)) if mode_name == "train" else {}
                hkw = dict(eps=eps) if mode_name == "train" else {}
                args = (dev(xs),) + ((dev(ys),) if cond else ()) + (dev(flat), {})
                hargs = (xs,) + ((ys,) if cond else ()) + (flat, {})
                if keep(tag + "/loss_and_grad", lambda: cnf.loss_and_grad(ic, mode, *args, with_x=True, with_ys=cond, with_base=with_base,
                                                                          **kw)) is None:
                    continue             # (no gradient of this network in this mode at all)
                out[tag + "/loss_and_grad/steps"] = np.asarray(ic.last_steps, dtype=np.float32).copy()
                if not with_base:
                    keep(tag + "/loss_and_grad_host", lambda: cnf.loss_and_grad(ic, mode, *hargs, with_x=True, with_ys=cond, **hkw))
                    keep(tag + "/loss_and_grad_plain", lambda: cnf.loss_and_grad(ic, mode, *args, **kw))

                    def submitted():
                        res = cnf.loss_and_grad_submit(ic, mode, *args, **kw)
                        cnf.loss_and_grad_collect(ic)
                        torch.cuda.synchronize()
                        return res
                    keep(tag + "/submit", submitted)
                keep(tag + "/inference_record", lambda: cnf.inference_record(ic, mode, *args, **kw))
                out[tag + "/inference_record/steps"] = np.asarray(ic.last_steps, dtype=np.float32).copy()
                keep(tag + "/inference_pullback", lambda: cnf.inference_pullback(ic, dev(cot), with_x=True, with_ys=cond, with_base=with_base))
                keep(tag + "/generate_record", lambda: cnf.generate_record(ic, mode, dev(flat), None, B, ys=dev(ys), z0=dev(eps), **kw))
                out[tag + "/generate_record/steps"] = np.asarray(ic.last_steps, dtype=np.float32).copy()
                keep(tag + "/generate_pullback", lambda: cnf.generate_pullback(ic, (dev(cz), dev(cl)), with_z0=True, with_ys=cond,
                                                                               with_base=with_base))
            ic.close()
    out["refused"] = np.array(refused, dtype=str)
    np.savez(out_path, **out)
    print(f"{len(out) - 1} arrays, {len(refused)} refused calls -> {out_path}")
    for r in refused:
        print("refused:", r)


def compare(a, b):
    za, zb = np.load(a), np.load(b)
    bad = sorted(set(za.files) ^ set(zb.files))
    for k in sorted(set(za.files) & set(zb.files)):
        if za[k].shape != zb[k].shape or not np.array_equal(za[k], zb[k]):
            bad.append(k)
    print(f"outputs: {len(za.files)} arrays in {a}, {len(zb.files)} in {b}: " + ("all bit-identical" if not bad else f"{len(bad)} DIFFER: {bad[:20]}"))
    return not bad


def _launches(path):
    """The ordered (kernel name with its template arguments, grid) list of a rocprofv3 --kernel-trace csv."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    return [(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"]) for r in rows]


def compare_traces(a, b):
    la, lb = _launches(a), _launches(b)
    first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None)
    same = first is None and len(la) == len(lb)
    print(f"launches: {len(la)} in {a}, {len(lb)} in {b}: " +
          ("identical names, template arguments and grids, in order" if same else f"DIFFER at launch {first}: {la[first] if first is not None else None} "
           f"vs {lb[first] if first is not None else None}"))
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--compare-traces", nargs=2)
    a = ap.parse_args()
    ok = True
    if a.out:
        run(a.out)
    if a.compare:
        ok = compare(*a.compare) and ok
    if a.compare_traces:
        ok = compare_traces(*a.compare_traces) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
