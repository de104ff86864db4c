"""What a non-default base distribution (cnf_set_basedist) costs at the headline shape (BASELINE config 3:
RNODE 32, 32-128-128-32, B = 8192, device tensors, resident eps):
  (a) inference(icnf, TrainMode(), xs, ps, st, eps=eps) with the default base, a diagonal and a dense Gaussian base;
  (b) loss_and_grad the same three ways at B = 32 and B = 8192;
  (c) cnf_draw_rademacher beside cnf_draw_normal and cnf_draw_uint32 at 32 x 8192 elements (`--draw-only`, for a
      `rocprofv3 --kernel-trace --stats` run of its own).
Every figure is the median over `--reps` calls after a warm-up, each call timed with device events around it; the variants
alternate call by call, and the spread is the inter-quartile range of the same calls.  On a checkout without
``basedist`` (the parent commit) only the default variant runs, so that the two commits can be timed in one session:

    python tools/prof_basedist.py [--reps 200] [--out profiles/basedist_prof.json]
    rocprofv3 --kernel-trace --stats -d OUTDIR -- python tools/prof_basedist.py --draw-only"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import continuousnf.jl_amd as cnf  # noqa: E402
from continuousnf.jl_amd import _lib, configs  # noqa: E402

HAVE_BASE = hasattr(cnf, "MvNormal")


def _variants(wl):
    out = {"default": None}
    if HAVE_BASE:
        rng = np.random.default_rng(1)
        n = wl.n_in
        mean = rng.standard_normal(n)
        ev = np.exp(rng.uniform(np.log(0.1), np.log(10.0), n))
        q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        out["diagonal"] = cnf.MvNormal(mean, ev)
        out["dense"] = cnf.MvNormal(mean, (q * ev) @ q.T)
    return out


def _timed(fns, reps):
    """Each function of `fns` called reps times, alternating; device-event time of every call (ms)."""
    for f in fns.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    res = {}
    for k, v in ev.items():
        t = np.array([a.elapsed_time(b) for a, b in v])
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        res[k] = {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4), "reps": reps}
    base = res["default"]["median_ms"]
    for k in res:
        res[k]["over_default"] = round(res[k]["median_ms"] / base, 4)
    return res


def model_calls(reps):
    wl = configs.BASELINE[3]
    ps = torch.from_numpy(configs.glorot_params(wl.dims, 3, 0.05)).cuda()
    out = {}
    for B in (8192, 32):
        xs_h, eps_h = configs.synthetic_inputs(wl, B, 1)
        xs = torch.from_numpy(np.ascontiguousarray(xs_h.T)).cuda().t()
        eps = torch.from_numpy(np.ascontiguousarray(eps_h.T)).cuda().t()
        ics = {}
        for k, d in _variants(wl).items():
            kw = {"basedist": d} if d is not None else {}
            ics[k] = cnf.construct(wl.tag, cnf.Chain(*[cnf.Dense(i, o, "tanh") for i, o in zip(wl.dims[:-1], wl.dims[1:])]), wl.nvars,
                                   wl.naugs, tspan=wl.tspan, sol_kwargs=configs.README_TOLERANCES, rng=0, **kw)
        if B == 8192:
            out["inference B=8192"] = _timed({k: (lambda ic=ic: cnf.inference(ic, cnf.TrainMode(), xs, ps, {}, eps=eps))
                                              for k, ic in ics.items()}, reps)
        out[f"loss_and_grad B={B}"] = _timed({k: (lambda ic=ic: cnf.loss_and_grad(ic, cnf.TrainMode(), xs, ps, {}, eps=eps))
                                              for k, ic in ics.items()}, max(20, reps // 4))
        for ic in ics.values():
            ic.close()
    return out


def draws(reps):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = 32 * 8192
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    res = {}
    for fn in ("cnf_draw_normal", "cnf_draw_uint32", "cnf_draw_rademacher"):
        f = getattr(_lib.lib(), fn, None)
        if f is None:
            continue
        for i in range(20):
            _lib.check(f(0, 1, 0, i * n, out.data_ptr(), n, st))
        torch.cuda.synchronize()
        ev = []
        for i in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(f(0, 1, 0, i * n, out.data_ptr(), n, st))
            b.record()
            ev.append((a, b))
        torch.cuda.synchronize()
        res[fn] = {"us_event_median": round(float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3), 2), "elements": n}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--draw-only", action="store_true")
    a = ap.parse_args()
    res = {"commit_has_basedist": HAVE_BASE, "device": torch.cuda.get_device_name(0), "draws": draws(a.reps)}
    if not a.draw_only:
        res.update(model_calls(a.reps))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
