"""The device generator (cnf_draw_normal) and what it changes for a caller that lets the library draw
the Hutchinson probes:
  (a) cnf_draw_normal alone at 32 x 8192 and 32 x 65536 normals: us per call (device events) and write GB/s;
  (b) inference(icnf, TrainMode(), xs_dev, ps, st) at the headline shape (BASELINE config 3, B = 8192) with a HIPRNG, with
      the default numpy rng (host draw + copy), and with a resident eps passed by the caller (what bench.py times);
  (c) loss_and_grad the same three ways at B = 32 and B = 8192.
Every figure is the median of many calls after a warm-up, each call ended by a device synchronise; the three ways alternate
call by call.  Kernel time: run `--draw-only` under `rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/prof_device_rng.py [--reps 100] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d OUTDIR -- python tools/prof_device_rng.py --draw-only"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import continuousnf.jl_amd as cnf  # noqa: E402
from continuousnf.jl_amd import _lib, configs  # noqa: E402

SIZES = ((32, 8192), (32, 65536))


def draw_kernel(reps, fn="cnf_draw_normal"):
    """(a): device-event time of one draw call, median over reps calls (cnf_draw_uint32 beside it: the same stores without
    the double-precision Box-Muller transform)."""
    f = getattr(_lib.lib(), fn)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    for rows, cols in SIZES:
        n = rows * cols
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for i in range(20):
            _lib.check(f(0, 1, 0, i * n, out.data_ptr(), n, st))
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(ev):
            a.record()
            _lib.check(f(0, 1, 0, i * n, out.data_ptr(), n, st))
            b.record()
        torch.cuda.synchronize()
        us = float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)
        res[f"{rows}x{cols}"] = {"us_event": round(us, 2), "write_GBps": round(4 * n / (us * 1e-6) / 1e9, 1)}
    return res


def _median_ms(fns, reps):
    """Each function of `fns` called reps times, alternating, each call timed to its device synchronise."""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t[k].append(time.perf_counter() - t0)
    return {k: round(float(np.median(v)) * 1e3, 4) for k, v in t.items()}


def _three(wl, B, seed):
    xs_h, eps_h = configs.synthetic_inputs(wl, B, seed)
    xs = torch.from_numpy(np.ascontiguousarray(xs_h.T)).cuda().t()
    eps = torch.from_numpy(np.ascontiguousarray(eps_h.T)).cuda().t()
    ps = torch.from_numpy(configs.glorot_params(wl.dims, 3, 0.05)).cuda()
    ics = {"hiprng": configs.build(wl, sol_kwargs=configs.README_TOLERANCES, rng=cnf.HIPRNG(seed)),
           "numpy_rng": configs.build(wl, sol_kwargs=configs.README_TOLERANCES, rng=seed),
           "resident_eps": configs.build(wl, sol_kwargs=configs.README_TOLERANCES, rng=seed)}
    return xs, eps, ps, ics


def callers(reps):
    wl = configs.BASELINE[3]
    res = {}
    xs, eps, ps, ics = _three(wl, wl.batch, 1)
    tm = cnf.TrainMode()
    fns = {"hiprng": lambda: cnf.inference(ics["hiprng"], tm, xs, ps, {}),
           "numpy_rng": lambda: cnf.inference(ics["numpy_rng"], tm, xs, ps, {}),
           "resident_eps": lambda: cnf.inference(ics["resident_eps"], tm, xs, ps, {}, eps=eps)}
    r = _median_ms(fns, reps)
    r["hiprng_over_resident"] = round(r["hiprng"] / r["resident_eps"], 4)
    r["numpy_over_resident"] = round(r["numpy_rng"] / r["resident_eps"], 4)
    res[f"inference B={wl.batch} (ms)"] = r
    for ic in ics.values():
        ic.close()
    for B in (32, 8192):
        xs, eps, ps, ics = _three(wl, B, 2)
        fns = {"hiprng": lambda: cnf.loss_and_grad(ics["hiprng"], tm, xs, ps, {}),
               "numpy_rng": lambda: cnf.loss_and_grad(ics["numpy_rng"], tm, xs, ps, {}),
               "resident_eps": lambda: cnf.loss_and_grad(ics["resident_eps"], tm, xs, ps, {}, eps=eps)}
        r = _median_ms(fns, reps)
        r["hiprng_over_resident"] = round(r["hiprng"] / r["resident_eps"], 4)
        r["numpy_over_resident"] = round(r["numpy_rng"] / r["resident_eps"], 4)
        res[f"loss_and_grad B={B} (ms)"] = r
        for ic in ics.values():
            ic.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--draw-only", action="store_true", help="only the draw kernel (for the rocprofv3 run)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_device_rng.py needs the MI355X")
    res = {"device": torch.cuda.get_device_name(0), "draw_normal": draw_kernel(max(args.reps, 200)),
           "draw_uint32": draw_kernel(max(args.reps, 200), "cnf_draw_uint32")}
    if not args.draw_only:
        res.update(callers(args.reps))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
