"""Float64 / float32 reference of the gradient w.r.t. a learnable Gaussian base distribution N(mean, L L') -- ``mean`` and the
scale (the lower-triangular ``L``, or the vector ``sigma`` of the diagonal kind) as torch autograd leaves (helper module; no
GPU needed).

Built on the references of the two directions: tests/vjp_ref.py gives the final state ``z_b(t1)`` of ``inference`` (which does
not depend on the base), tests/gen_vjp_ref.py the total derivative ``grad_z0`` of sampling, tests/basedist_ref.py the Gaussian
they evaluate.  What is differentiated here, in torch:

    density direction              S = sum_b w_b logpdf(z_b(t1); mean, L)                      w = the cotangent of logpx
    sampling, z0 given             S = sum_b w_b logpdf(z0_b; mean, L)                         w = the cotangent of logq
    sampling, z0 = mean + L n_b    S = sum_b w_b logpdf(stop(z0_b); mean, L) + <grad_z0, mean + L n>      (the total derivative)

``formulas`` restates the first two in closed form (tests/test_base_grad_ref_host.py holds autograd to it):

    g_mean = W' sum_b w_b n_b,   g_L = tril(W' sum_b w_b n_b n_b') - (sum_b w_b) diag(1 / L_ii),   n_b = W (z_b - mean), W = inv(L)
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import basedist_ref as BR
from tests import gen_vjp_ref as R
from tests import vjp_ref as V


def gauss(mean, scale, dense):
    """The tests.basedist_ref.Gauss of (mean, scale)."""
    s = np.asarray(scale, np.float64)
    return BR.Gauss(np.asarray(mean, np.float64), np.tril(s) @ np.tril(s).T if dense else s * s)


def logpdf_t(z, mean, scale, dense):
    """logpdf of the columns of ``z`` (n x B) in torch, in the parametrisation cnf_set_basedist takes."""
    n = z.shape[0]
    d = z - mean[:, None]
    if dense:
        L = torch.tril(scale)
        w = torch.linalg.solve_triangular(L, d, upper=False)
        logdet = torch.log(torch.diagonal(L)).sum()
    else:
        w = d / scale[:, None]
        logdet = torch.log(scale).sum()
    return -logdet - 0.5 * n * math.log(2.0 * math.pi) - 0.5 * (w * w).sum(0)


def _leaves(mean, scale, dtype):
    t = torch.float64 if dtype == np.float64 else torch.float32
    return (torch.tensor(np.asarray(mean, np.float64), dtype=t, requires_grad=True),
            torch.tensor(np.asarray(scale, np.float64), dtype=t, requires_grad=True), t)


def logpdf_grads(z, w, mean, scale, dense, dtype=np.float64):
    """(g_mean, g_scale) = d / d (mean, scale) of sum_b w_b logpdf(z_b) by autograd, computed in ``dtype``, returned float64."""
    m, s, t = _leaves(mean, scale, dtype)
    S = (torch.tensor(np.asarray(w, np.float64), dtype=t) * logpdf_t(torch.tensor(np.asarray(z, np.float64), dtype=t), m, s, dense)).sum()
    gm, gs = torch.autograd.grad(S, (m, s))
    return gm.double().numpy(), gs.double().numpy()


def formulas(z, w, mean, scale, dense):
    """(g_mean, g_scale, quad, logdet) in float64 from the closed form; g_scale = quad + logdet, its two summands."""
    z, w, mean, s = (np.asarray(a, np.float64) for a in (z, w, mean, scale))
    if dense:
        L = np.tril(s)
        W = np.linalg.inv(L)
        n = W @ (z - mean[:, None])
        return W.T @ (n @ w), np.tril(W.T @ ((n * w) @ n.T)) - w.sum() * np.diag(1.0 / np.diag(L)), \
            np.tril(W.T @ ((n * w) @ n.T)), -w.sum() * np.diag(1.0 / np.diag(L))
    n = (z - mean[:, None]) / s[:, None]
    quad, logdet = ((n * n) @ w) / s, -w.sum() / s
    return (n @ w) / s, quad + logdet, quad, logdet


def sample_pullback(normals, gz0, dense):
    """The pullback of z0 = mean + L n: (sum_b g_b, tril(sum_b g_b n_b')) or the diagonal of the latter; float64."""
    n, g = np.asarray(normals, np.float64), np.asarray(gz0, np.float64)
    return g.sum(1), (np.tril(g @ n.T) if dense else (g * n).sum(1))


def final_state(cfg, flat, xs, eps, dts, ys=None, train=True, dtype=np.float64):
    """z_b(t1) of ``inference`` through the steps ``dts`` (n_in x B), computed in ``dtype``."""
    c = lambda a: V._cast(a, dtype)
    _, us, _ = V.outputs(cfg, c(flat), c(xs), c(eps), dts, c(ys), train)
    return us[-1][:cfg.n_in]


def density(cfg, flat, xs, eps, w, dts, mean, scale, dense, ys=None, train=True, dtype=np.float64):
    """The density direction: (g_mean, g_scale) for the cotangent ``w`` of logpx."""
    return logpdf_grads(final_state(cfg, flat, xs, eps, dts, ys, train, dtype), w, mean, scale, dense, dtype)


def drawn_z0(normals, mean, scale, dense, dtype=np.float64):
    n, m, s = (np.asarray(a).astype(dtype) for a in (normals, mean, scale))
    return (m[:, None] + (np.tril(s) @ n if dense else s[:, None] * n)).astype(dtype)


def sampling_drawn(cfg, flat, normals, eps, cot_z, cot_logq, dts, mean, scale, dense, ys=None, train=True, dtype=np.float64):
    """The sampling direction with z0 = mean + L n drawn from ``normals``: the TOTAL (g_mean, g_scale) for the cotangent
    (cot_z, cot_logq) of (z, logq), and grad_z0 of the reference it went through."""
    B = np.asarray(normals).shape[1]
    z0 = drawn_z0(normals, mean, scale, dense, dtype)
    run = R.vjp64 if dtype == np.float64 else R.vjp32
    gz0 = run(cfg, flat, z0, eps, cot_z, cot_logq, dts, ys, train, gauss(mean, scale, dense))[3]
    m, s, t = _leaves(mean, scale, dtype)
    tt = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=t)
    nrm = tt(normals)
    z0_t = m[:, None] + (torch.tril(s) @ nrm if dense else s[:, None] * nrm)
    cl = tt(np.zeros(B) if cot_logq is None else cot_logq)
    S = (cl * logpdf_t(z0_t.detach(), m, s, dense)).sum() + (tt(gz0) * z0_t).sum()
    gm, gs = torch.autograd.grad(S, (m, s))
    return gm.double().numpy(), gs.double().numpy(), np.asarray(gz0, np.float64)


# ---- the bar: tests/grad_terms.py's convention, per block (g_mean, g_scale) ----
RTOL, FLOOR_FACTOR, RTOL_CAP = V.RTOL, V.FLOOR_FACTOR, V.RTOL_CAP


def block_scales(ref64, summands=None):
    """scale of g_mean and of g_scale: max-abs + rms of the block; for g_scale at least the max-abs of each of its two summands
    (the quadratic term and the diag(1 / L) term cancel near the optimum)."""
    sm, ss = V.scale(ref64[0]), V.scale(ref64[1])
    if summands is not None:
        ss = max([ss] + [float(np.abs(np.asarray(a, np.float64)).max()) for a in summands])
    return sm, ss


def report(got, ref64, ref32, summands=None):
    """[(block, err / scale, floor, rtol, scale, ok)] for got = (g_mean, g_scale): err <= rtol scale, rtol = max(1e-4, 8 floor)
    <= 1e-3, floor = the float32 run of the same reference against its float64 run over that scale (never a device number)."""
    recs = []
    for name, g, r64, r32, s in zip(("g_mean", "g_scale"), got, ref64, ref32, block_scales(ref64, summands)):
        r64 = np.asarray(r64, np.float64)
        floor = float(np.abs(np.asarray(r32, np.float64) - r64).max()) / s if s > 0 else np.inf
        rtol = max(RTOL, FLOOR_FACTOR * floor)
        err = np.inf
        if g is not None:
            g = np.asarray(g, np.float64)
            err = float(np.abs(g - r64).max()) / s if s > 0 and g.shape == r64.shape else np.inf
        recs.append((name, err, floor, rtol, s, bool(np.isfinite(err) and err <= rtol and rtol <= RTOL_CAP)))
    return recs


def assert_floor(ref64, ref32, summands, what):
    """The float32 floor of a device case leaves the bar in force: 8 floor <= 1e-3 on both blocks."""
    recs = report((None, None), ref64, ref32, summands)
    print(f"base-grad floor | {what}: " + "; ".join(f"{n} floor {f:.2e} rtol {r:.1e} scale {s:.2e}" for n, _, f, r, s, _ in recs))
    for n, _, f, r, s, _ in recs:
        assert s > 0, f"{what} {n}: the reference is zero over this block"
        assert r <= RTOL_CAP, f"{what} {n}: the float32 reference's own error {f:.3g} asks for rtol {r:.3g} > the cap {RTOL_CAP:g}"
    return recs


def assert_base(got, ref64, ref32, summands, what):
    recs = report(got, ref64, ref32, summands)
    print(f"base-grad | {what} | block err/scale floor rtol: " + "; ".join(f"{n} {e:.2e} {f:.2e} {r:.1e}" for n, e, f, r, _, _ in recs))
    for n, e, f, r, s, ok in recs:
        assert s > 0, f"{what} {n}: the reference is zero over this block (nothing to compare against)"
        assert r <= RTOL_CAP, f"{what} {n}: the float32 reference's own error {f:.3g} asks for rtol {r:.3g} > the cap {RTOL_CAP:g}"
    bad = [x for x in recs if not x[-1]]
    assert not bad, f"{what}: " + "; ".join(f"{n} off by {e:.3g} of its scale {s:.3g} (rtol {r:.3g}, float32 floor {f:.3g})"
                                           for n, e, f, r, s, _ in bad)
    return recs


def summands_of(g_scale, w_sum, scale, dense):
    """The two summands of a g_scale: the diag(1 / L) term -(sum w) diag(1 / L_ii) and the rest."""
    s = np.asarray(scale, np.float64)
    logdet = -float(w_sum) * (np.diag(1.0 / np.diag(s)) if dense else 1.0 / s)
    return np.asarray(g_scale, np.float64) - logdet, logdet


# ---- the cases of the device tests (tests/test_gpu_base_grad.py); their float32 floors are held by the host test ----
def base_of(n_in, dense, seed):
    """(mean, scale) of a case: a shifted mean, and a scale with a diagonal in [0.6, 1.6] (dense: plus a strict lower part)."""
    rng = np.random.default_rng(seed)
    mean = (0.4 * rng.standard_normal(n_in)).astype(np.float32)
    d = rng.uniform(0.6, 1.6, n_in)
    if not dense:
        return mean, d.astype(np.float32)
    L = np.tril(rng.standard_normal((n_in, n_in)), -1) * (0.3 / math.sqrt(n_in)) + np.diag(d)
    return mean, L.astype(np.float32)


def _cases():
    from tests import grad_terms as GT
    from oracle import cnf_oracle as O
    T = O.ACT_TANH
    C = GT.Case
    #  GT.Case (network, batch, seed, route of the pullback), dense?, TrainMode?
    return {
        "n3-diag-B17": (C("n3-diag-B17", "generic", (3, 8, 3), (T, T), 2, 1, 17, 2101, scale=0.3, kernel="auto"), False, True),
        "n3-dense-B300": (C("n3-dense-B300", "generic", (3, 8, 3), (T, T), 2, 1, 300, 2102, scale=0.3, kernel="auto"), True, True),
        "n16-dense-B17-jvp": (C("n16-dense-B17-jvp", "adj_mfma", (16, 32, 16), (T, T), 16, 0, 17, 2103, jvp=True, scale=0.3, kernel="auto"), True, True),
        "n16-dense-cond-B17": (C("n16-dense-cond-B17", "adj_mfma", (16, 32, 16), (T, T), 12, 4, 17, 2104, n_cond=3, scale=0.3, kernel="auto"), True, True),
        "n17-diag-B1": (C("n17-diag-B1", "adj_mfma", (17, 24, 17), (T, T), 12, 5, 1, 2105, scale=0.3, kernel="auto"), False, True),
        "n17-dense-B300": (C("n17-dense-B300", "adj_mfma", (17, 24, 17), (T, T), 12, 5, 300, 2106, scale=0.3, kernel="auto"), True, True),
        "n33-dense-B1": (C("n33-dense-B1", "adj_mfma", (33, 40, 33), (T, T), 33, 0, 1, 2107, scale=0.3, kernel="auto"), True, True),
        "n33-dense-B17-test": (C("n33-dense-B17-test", "test", (33, 40, 33), (T, T), 33, 0, 17, 2108, scale=0.3, kernel="auto"), True, False),
        "n33-diag-B300-test": (C("n33-diag-B300-test", "test", (33, 40, 33), (T, T), 33, 0, 300, 2109, scale=0.3, kernel="auto"), False, False),
        "headline-dense-B33": (C("headline-dense-B33", "adj3b", (32, 128, 128, 32), (T,) * 3, 32, 0, 33, 2110), True, True),
        "headline-diag-B33": (C("headline-diag-B33", "adj3b", (32, 128, 128, 32), (T,) * 3, 32, 0, 33, 2111), False, True),
    }


CASES = _cases()
LAM = (1.0, 1.0)          # lambda1 = lambda2 = 1 (lambda3 = 1 with augmented rows): the E and n rows are integrated


def case_setup(name):
    """Everything a test of case ``name`` needs, host side: (case, dense, train, cfg, (flat, xs, eps, ys), mean, scale, normals,
    rng) -- ``normals`` n_in x B (seed + 11, as gen_vjp_ref.case_z0), ``rng`` seeded for the cotangents."""
    case, dense, train = CASES[name]
    cfg = case.cfg(LAM + (1.0 if case.naugs else 0.0,))
    mean, scale = base_of(case.nvars + case.naugs, dense, case.seed + 3)
    return case, dense, train, cfg, case.inputs(), mean, scale, R.case_z0(case), np.random.default_rng(case.seed + 7)


def cotangents_w(rng, B, k=3):
    """k different per-sample cotangents (N(0, 1)/B entries; the first with a non-zero sum pushed to -1: the loss's)."""
    ws = [(rng.standard_normal(B) / B).astype(np.float32) for _ in range(k)]
    ws[0] = (ws[0] - ws[0].mean() - 1.0 / B).astype(np.float32)
    return ws
