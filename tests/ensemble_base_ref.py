"""Cases and references of the ensembles with a base distribution per member (``bases=``; helper module, no GPU needed).

The cases are those of tests/ensemble_vjp_ref.py (the same networks, modes, spans, end times and step settings: every tile shape
and masking edge of the ensemble kernels), each with the kinds of base the device tests run it with.  The members' bases: means
of O(1) that differ per member, covariances from ``basedist_ref.random_cov`` (eigenvalues log-uniform in [0.1, 10]), each
member its own -- and member ``UNIT`` exactly N(0, I).  The references are the tree's own, member by member, nothing restated:
``vjp_ref.vjp64`` / ``vjp32`` and ``gen_vjp_ref.vjp64`` / ``vjp32`` with ``base=``, ``base_grad_ref.density`` /
``sampling_drawn`` for the base's own gradient.  tests/test_ensemble_base_host.py checks on the CPU that the float32 floor of
every case leaves the bars where tests/test_gpu_ensemble_base.py needs them.
"""
from __future__ import annotations

import numpy as np

from tests import base_grad_ref as BG
from tests import basedist_ref as BR
from tests import ensemble_vjp_ref as R
from tests import gen_vjp_ref as GR
from tests import vjp_ref as V

M = R.M
UNIT = 1                           # the member whose base is exactly (0, I)
BY_NAME = {c.name: c for c in R.CASES}

# case -> the kinds the device tests run it with ("dense" / "diag"): 2-6-2 (per-member t1) dense; 16-48-16 both (n_in = 16
# exactly: the whole P tile is live); 7-13-7 dense (rows 7..15 of P and mu are padding; reversed tspan); 6-9-6 diagonal
KINDS = {
    "readme-vjp-B33": ("dense",),
    "regr-vjp-B17-rejects": ("diag", "dense"),
    "regr-jvp-B33": ("diag", "dense"),
    "regr-test-B17": ("diag", "dense"),
    "noaug-vjp-B1": ("dense",),
    "id2-vjp-B17": ("diag",),
}
CASE_KINDS = [(BY_NAME[n], k) for n, ks in KINDS.items() for k in ks]
IDS = [f"{c.name}-{k}" for c, k in CASE_KINDS]
RAGGED = ("readme-vjp-B33", "dense", (1, 17, 33))       # counts, with lambdas and bases together
RAGGED_LAMBDAS = np.asarray([[1e-2, 1e-2, 1e-2], [3e-2, 5e-3, 2e-2], [5e-3, 2e-2, 4e-2]], np.float32)


def bases(case, kind, seed=0):
    """``(mean (M, n_in), scale)`` float32: ``scale`` is sigma (M, n_in) for "diag", the Cholesky factor L (M, n_in, n_in) for
    "dense" -- what ``EnsembleBases(mean, std= | scale_tril=)`` takes.  Member ``UNIT`` is exactly (0, I)."""
    n = case.cfg.n_in
    rng = np.random.default_rng(4200 + 10 * case.seed + (1 if kind == "dense" else 0) + 100 * seed)
    mean = rng.uniform(-1.0, 1.0, (M, n)) + np.asarray([0.5, 0.0, -0.5])[:, None]
    if kind == "dense":
        scale = np.stack([np.linalg.cholesky(BR.random_cov(rng, n, "full")) for _ in range(M)])
        scale[UNIT] = np.eye(n)
    else:
        scale = np.stack([np.sqrt(BR.random_cov(rng, n, "diag")) for _ in range(M)])
        scale[UNIT] = 1.0
    mean[UNIT] = 0.0
    return mean.astype(np.float32), scale.astype(np.float32)


def gauss(mean, scale, kind, m):
    """Member m's base as the ``basedist_ref.Gauss`` the references take (from the float32 values the device is given)."""
    return BG.gauss(mean[m], scale[m], kind == "dense")


def reference(case, m, ps, xs, eps, cot, dts, g):
    """``(out64 (4, B), (grad64, gx64), (grad32, gx32))`` of member m under its base ``g`` (None: N(0, I)) through ``dts``."""
    cfg = R.member_cfg(case, m)
    e = eps[m] if case.train else None
    out, g64, x64 = V.vjp64(cfg, ps[m], xs[m], e, cot, dts, train=case.train, base=g)
    _, g32, x32 = V.vjp32(cfg, ps[m], xs[m], e, cot, dts, train=case.train, base=g)
    return out, (g64, x64), (g32, x32)


def base_reference(case, m, ps, xs, eps, w, dts, mean, scale, kind):
    """``(ref64, ref32, summands)`` of d / d (mean_m, scale_m) of ``sum_b w_b logpx[m, b]``: ``base_grad_ref.density``."""
    cfg = R.member_cfg(case, m)
    e = eps[m] if case.train else None
    dense = kind == "dense"
    r64 = BG.density(cfg, ps[m], xs[m], e, w, dts, mean[m], scale[m], dense, train=case.train, dtype=np.float64)
    r32 = BG.density(cfg, ps[m], xs[m], e, w, dts, mean[m], scale[m], dense, train=case.train, dtype=np.float32)
    return r64, r32, BG.summands_of(r64[1], float(np.sum(np.asarray(w, np.float64))), scale[m], dense)


def loss_of(case, m, out, lambdas=None):
    """The member's loss from its float64 outputs (4, B): src/icnf.jl:489 (TrainMode), src/base_icnf.jl:496 (TestMode)."""
    c = case.cfg
    lam = (c.lam1, c.lam2, c.lam3) if lambdas is None else tuple(float(v) for v in lambdas)
    if not case.train:
        return float(-out[0].mean())
    return float((-out[0] + lam[0] * out[1] + lam[1] * out[2] + (lam[2] * out[3] if c.naugs else 0.0)).mean())


# ---- sampling ----
def sampling_inputs(case, n):
    """``(normals (M, n_in, n), eps (M, n_in, n))`` float32 of the sampling tests."""
    rng = np.random.default_rng(5300 + case.seed)
    k = case.cfg.n_in
    return rng.standard_normal((M, k, n)).astype(np.float32), rng.standard_normal((M, k, n)).astype(np.float32)


def sampling_cfg(case, m):
    """Member m's configuration for sampling: generate integrates reverse(tspan) (gen_vjp_ref takes the forward span)."""
    return R.member_cfg(case, m)


def sampling_reference(case, m, ps, normals, eps, cot_z, cot_logq, dts, mean, scale, kind, dtype=np.float64):
    """``base_grad_ref.sampling_drawn`` of member m: the TOTAL ``(g_mean, g_scale)`` and ``grad_z0``."""
    return BG.sampling_drawn(sampling_cfg(case, m), ps[m], normals[m], eps[m] if case.train else None, cot_z, cot_logq, dts, mean[m],
                             scale[m], kind == "dense", train=case.train, dtype=dtype)


def sampling_grads(case, m, ps, normals, eps, cot_z, cot_logq, dts, mean, scale, kind):
    """``(grad64, grad32)``: the parameter gradient of member m's sampling from the drawn ``z0 = mean_m + L_m n`` under its base
    -- ``gen_vjp_ref.vjp64`` / ``vjp32`` with ``base=`` (the run ``base_grad_ref.sampling_drawn`` takes ``grad_z0`` from)."""
    cfg, dense, out = sampling_cfg(case, m), kind == "dense", []
    for dtype, run in ((np.float64, GR.vjp64), (np.float32, GR.vjp32)):
        z0 = BG.drawn_z0(normals[m], mean[m], scale[m], dense, dtype)
        out.append(np.asarray(run(cfg, ps[m], z0, eps[m] if case.train else None, cot_z, cot_logq, dts, None, case.train,
                                  gauss(mean, scale, kind, m))[2], np.float64))
    return tuple(out)


def sampling_forward(case, m, ps, z0, eps, dts, g, dtype=np.float64):
    """``gen_vjp_ref.forward`` of member m from ``z0`` under its base: (x, logq, ...)."""
    c = lambda a: None if a is None else np.asarray(a).astype(dtype)
    return GR.forward(sampling_cfg(case, m), c(ps[m]), c(z0), c(eps[m]) if case.train else None, dts, train=case.train, base=g)
