"""What a learnable base distribution (``LearnableNormal``) costs at the headline shape (BASELINE config 3:
32-128-128-32, n_in = 32, device tensors), wall-clock medians on the host with the device drained before and after each call:
  (a) the upload of changed values -- ``ICNF.set_basedist``: the float64 reduction on the host and the synchronous
      cnf_set_basedist -- for the diagonal and the dense kind: the host wait every optimiser step on the base pays;
  (b) cnf_base_logpdf_pullback on an inference record and cnf_base_sample_pullback, at B = 256 and B = 8192;
  (c) one optimiser step on the base, ``reverse_kl(...).backward()`` at B = 256, beside the same step with the base constant.

    python tools/prof_base_grad.py [--reps 100] [--out profiles/base_grad_prof.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import continuousnf.jl_amd as cnf  # noqa: E402
from continuousnf.jl_amd import configs  # noqa: E402


def _wall(f, reps, warm=5):
    for _ in range(warm):
        f()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return {"median_us": round(float(med), 1), "iqr_us": round(float(q3 - q1), 1), "reps": reps}


def _model(wl, base, fixed=False):
    kw = dict(adaptive=False, dt=0.25) if fixed else configs.README_TOLERANCES
    return cnf.construct(wl.tag, cnf.Chain(*[cnf.Dense(i, o, "tanh") for i, o in zip(wl.dims[:-1], wl.dims[1:])]), wl.nvars, wl.naugs,
                         tspan=wl.tspan, sol_kwargs=kw, rng=0, basedist=base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    wl = configs.BASELINE[3]
    n = wl.n_in
    ps = torch.from_numpy(configs.glorot_params(wl.dims, 3, 0.05)).cuda()
    rng = np.random.default_rng(1)
    res = {"device": torch.cuda.get_device_name(0), "n_in": n}
    for kind in ("diagonal", "dense"):
        mean = torch.zeros(n, requires_grad=True)
        scale = torch.tensor(np.eye(n, dtype=np.float32) if kind == "dense" else np.ones(n, np.float32), requires_grad=True)
        base = cnf.LearnableNormal(mean, scale_tril=scale) if kind == "dense" else cnf.LearnableNormal(mean, std=scale)
        ic = _model(wl, base)
        ic.set_params(ps)

        def upload():
            with torch.no_grad():
                mean.add_(1e-3)
            ic.set_basedist()
        r = {"upload (host reduction + cnf_set_basedist)": _wall(upload, a.reps)}
        for B in (256, 8192):
            xs_h, eps_h = configs.synthetic_inputs(wl, B, 1)
            xs = torch.from_numpy(np.ascontiguousarray(xs_h.T)).cuda().t()
            eps = torch.from_numpy(np.ascontiguousarray(eps_h.T)).cuda().t()
            cnf.inference_record(ic, cnf.TrainMode(), xs, ps, {}, eps=eps)
            w = torch.full((B,), -1.0 / B, device="cuda")
            r[f"cnf_base_logpdf_pullback B={B}"] = _wall(lambda: cnf.base_logpdf_pullback(ic, w), a.reps)
            nrm = torch.from_numpy(rng.standard_normal((n, B)).astype(np.float32)).cuda()
            r[f"cnf_base_sample_pullback B={B}"] = _wall(lambda: cnf.base_sample_pullback(ic, nrm, nrm), a.reps)
        ic.close()
        res[kind] = r
    # one optimiser step on the base beside the same step with the base constant
    B = 256
    target = lambda x: -0.5 * (x * x).sum(0)
    steps = {}
    for name in ("constant base", "learnable base"):
        mean, log_std = torch.zeros(n, requires_grad=name == "learnable base"), torch.zeros(n, requires_grad=name == "learnable base")
        base = cnf.LearnableNormal(mean, std=log_std.exp())
        ic = _model(wl, base)
        p = ps.clone().requires_grad_(True)
        opt = torch.optim.Adam([p] + ([mean, log_std] if name == "learnable base" else []), lr=1e-3)

        def step():
            opt.zero_grad()
            if name == "learnable base":
                base.update(mean, std=log_std.exp())
            cnf.reverse_kl(ic, cnf.TrainMode(), p, {}, B, target).backward()
            opt.step()
        steps[name] = _wall(step, max(20, a.reps // 4))
        ic.close()
    res[f"reverse_kl step B={B}"] = steps
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
