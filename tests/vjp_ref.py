"""Float64 reference of the vector-Jacobian product of ``inference`` for an arbitrary cotangent of its four outputs (helper
module; no GPU needed).

The weighted discrete adjoint restated from the oracle's own pieces -- ``G.forward_record``, ``G.rhs_vjp`` and
``G.rhs_vjp_test`` (both take a per-column cotangent), ``O.inference_sol``, the Tsit5 tables -- with the terminal cotangent

    lam_z(t1)[., b] = g_logpx[b] d logpdf(basedist, z_b) / d z + g_A[b] unit(z_aug, b)        (N(0, I): -g_logpx[b] z_b)
    lam_dlogp[b] = -g_logpx[b]   (logpx = logpz - dlogp, src/base_icnf.jl:177-178),   lam_E[b] = g_E[b],   lam_n[b] = g_n[b]

With g = (-1/B, lam1/B, lam2/B, lam3/B) it is ``G.loss_and_grad``'s adjoint (tests/test_vjp_ref_host.py pins that, central
differences, and the independence of the samples).  Rows the model does not integrate carry no cotangent: lam1 = 0 means
E = 0 and g_E is ignored, likewise lam2 / n and lam3 / A, and all three in TestMode.  Nothing under oracle/ is changed.
"""
from __future__ import annotations

import numpy as np

from oracle import cnf_grad_oracle as G
from oracle import cnf_oracle as O
from tests.grad_terms import param_blocks  # noqa: F401  (re-exported: the blocks the bars are taken over)


def _cast(a, dtype):
    return None if a is None else np.asarray(a).astype(dtype)


def outputs(cfg, flat, xs, eps, dts, ys=None, train=True, base=None):
    """(out = [logpx, E, n, A] as a 4 x B array, us, f): the four outputs of ``inference`` through the steps ``dts``.
    ``base``: a tests.basedist_ref.Gauss in place of N(0, I)."""
    u0 = O.inference_u0(cfg, xs, train)
    f = cfg.rhs(flat, eps if train else None, train, ys)
    us = G.forward_record(f, u0, cfg.tspan[0], cfg.tspan[1], [abs(float(d)) for d in dts])
    logpx, (E, n, A) = O.inference_sol(cfg, us[-1], train)
    if base is not None:
        z = us[-1][:cfg.n_in]
        logpx = (base.logpdf(z) - us[-1][cfg.n_in]).astype(us[-1].dtype)
    z = np.zeros_like(logpx)
    rows = [logpx] + [np.broadcast_to(np.asarray(r, dtype=logpx.dtype), logpx.shape) if train else z for r in (E, n, A)]
    return np.stack(rows), us, f


def _stages(f, u, h, T):
    A = O.TSIT5_A
    ks, Us = [], []
    for s in range(6):
        acc = np.zeros_like(u)
        for j in range(s):
            acc = acc + T(A[s][j]) * ks[j]
        Us.append(u + h * acc)
        ks.append(f(Us[-1]))
    return Us


def vjp(cfg, flat, xs, eps, cot, dts, ys=None, train=True, base=None):
    """(out, grad, grad_x): ``out`` as ``outputs`` gives it, grad = sum_b sum_r cot[r][b] d out_r[b] / d flat and the same
    w.r.t. xs (nvars x B), through the fixed steps ``dts``, in the dtype of ``flat``.  ``cot``: 4 x B, rows (logpx, E, n, A)."""
    flat = np.asarray(flat)
    dts = [abs(float(d)) for d in dts]
    out, us, f = outputs(cfg, flat, xs, eps, dts, ys, train, base)
    fsol = us[-1]
    T = fsol.dtype.type
    cot = np.asarray(cot).astype(fsol.dtype)
    n_in = cfg.n_in
    z = fsol[:n_in]
    neg_grad = z if base is None else base.neg_grad(z).astype(fsol.dtype)         # -d logpdf / d z
    lam = np.zeros_like(fsol)
    lam[:n_in] = -cot[0] * neg_grad
    lam[n_in] = -cot[0]
    if train:
        if cfg.lam3 != 0 and cfg.naugs > 0:
            lam[cfg.nvars:n_in] += cot[3] * G._unit(z[cfg.nvars:])
        lam[n_in + 1] = cot[1]
        lam[n_in + 2] = cot[2]
    grad = np.zeros(flat.size, dtype=flat.dtype)
    A, Bc = O.TSIT5_A, O.TSIT5_B
    nz, nj = cfg.lam1 != 0, cfg.lam2 != 0
    tdir = 1.0 if cfg.tspan[1] >= cfg.tspan[0] else -1.0
    wl = lam[n_in][None, :]
    lz = lam[:n_in].copy()
    for n in reversed(range(len(dts))):
        h = T(tdir * dts[n])
        Us = _stages(f, us[n], h, T)
        ws = [None] * 6
        for i in reversed(range(6)):
            if train:
                kbar = T(Bc[i]) * lam
                for m in range(i + 1, 6):
                    kbar[:n_in] += T(A[m][i]) * ws[m]
                ws[i], g = G.rhs_vjp(cfg.net, flat, Us[i][:n_in], eps, h * kbar, nz, nj, cfg.use_jvp, ys)
            else:
                kb = T(Bc[i]) * lz
                for m in range(i + 1, 6):
                    kb = kb + T(A[m][i]) * ws[m]
                ws[i], g = G.rhs_vjp_test(cfg.net, flat, Us[i][:n_in], h * kb, h * T(Bc[i]) * wl, ys)
            grad += g
        if train:
            lam = lam.copy()
            for i in range(6):
                lam[:n_in] += ws[i]
        else:
            lz = lz + sum(ws)
    gx = (lam if train else lz)[:cfg.nvars].copy()
    return out, grad, gx


def vjp64(cfg, flat, xs, eps, cot, dts, ys=None, train=True, base=None):
    c = lambda a: _cast(a, np.float64)
    return vjp(cfg, c(flat), c(xs), c(eps), c(cot), dts, c(ys), train, base)


def vjp32(cfg, flat, xs, eps, cot, dts, ys=None, train=True, base=None):
    c = lambda a: _cast(a, np.float32)
    return vjp(cfg, c(flat), c(xs), c(eps), c(cot), dts, c(ys), train, base)


def loss_cotangent(cfg, B, train=True):
    """The cotangent of the built-in loss: (-1/B, lam1/B, lam2/B, lam3/B) per sample."""
    l = (cfg.lam1, cfg.lam2, cfg.lam3 if cfg.naugs else 0.0) if train else (0.0, 0.0, 0.0)
    return np.stack([np.full(B, -1.0 / B)] + [np.full(B, v / B) for v in l])


def row_cotangents(rng, B, rows):
    """The five cotangents of the device tests: each output row of ``rows`` alone (N(0, 1)/B entries, zeros elsewhere), then
    all of them together.  name -> 4 x B float32."""
    names = ("logpx", "E", "n", "A")
    out = {}
    for r in rows:
        c = np.zeros((4, B), np.float32)
        c[r] = (rng.standard_normal(B) / B).astype(np.float32)
        out[names[r]] = c
    c = np.zeros((4, B), np.float32)
    for r in rows:
        c[r] = (rng.standard_normal(B) / B).astype(np.float32)
    out["all"] = c
    return out


def scale(a):
    a = np.asarray(a, np.float64)
    return float(np.abs(a).max() + np.sqrt(np.mean(a * a))) if a.size else 0.0


RTOL, FLOOR_FACTOR, RTOL_CAP = 1e-4, 8.0, 1e-3       # the bar of tests/grad_terms.py, taken over unchanged


def report(got, got_x, ref64, ref32, net):
    """Per parameter block and for grad_x: (name, err / scale, float32 floor, rtol, ok) with
    max|got - ref64| <= rtol (max|ref64| + rms ref64) over the block, rtol = max(1e-4, 8 floor) <= 1e-3, floor = the error of
    the float32 run of the SAME reference over that scale (never of the device).  ``ref64`` / ``ref32``: (grad, grad_x)."""
    recs = []

    def rec(name, g, r64, r32):
        s = scale(r64)
        floor = float(np.abs(np.asarray(r32, np.float64) - r64).max()) / s if s > 0 else np.inf
        err = float(np.abs(np.asarray(g, np.float64) - r64).max()) / s if s > 0 else np.inf
        rtol = max(RTOL, FLOOR_FACTOR * floor)
        recs.append((name, err, floor, rtol, s, bool(np.isfinite(err) and err <= rtol and rtol <= RTOL_CAP)))

    for name, sl in param_blocks(net).items():
        rec(name, np.asarray(got)[sl], ref64[0][sl], ref32[0][sl])
    if got_x is not None:
        rec("grad_x", got_x, ref64[1], ref32[1])
    return recs


def assert_vjp(got, got_x, ref64, ref32, net, what):
    recs = report(got, got_x, ref64, ref32, net)
    print(f"vjp | {what} | block err/scale floor rtol: " + "; ".join(f"{n} {e:.2e} {f:.2e} {r:.1e}" for n, e, f, r, _, _ in recs))
    for n, e, f, r, s, ok in recs:
        assert s > 0, f"{what} {n}: the reference is zero over this block (nothing to compare against)"
        assert r <= RTOL_CAP, f"{what} {n}: the float32 reference's own error {f:.3g} asks for rtol {r:.3g} > the cap {RTOL_CAP:g}"
    bad = [x for x in recs if not x[-1]]
    assert not bad, f"{what}: " + "; ".join(f"{n} off by {e:.3g} of its scale {s:.3g} (rtol {r:.3g}, float32 floor {f:.3g})"
                                           for n, e, f, r, s, _ in bad)
    return recs
