"""Float64 / float32 reference of differentiable sampling: ``generate`` with the log-density of the sample, and the
vector-Jacobian product of ``(z, logq)`` w.r.t. the parameters, the base draw ``z0`` and (conditional models) ``ys`` (helper
module; no GPU needed).

``generate`` integrates the augmented state over ``reverse(tspan)`` from ``u0 = [z0; 0]`` (src/base_icnf.jl:358-380).  The
dlogp row of that solve is the log-density the sample has gained on its way:

    z    = rows 1..n_in of the final state              (the sample is its first nvars rows)
    logq = logpdf(basedist, z0) + dlogp_end              (sign +; ``inference`` has logpz - dlogp)

Restated from the oracle's own pieces as tests/vjp_ref.py is -- ``G.forward_record``, ``G.rhs_vjp`` / ``G.rhs_vjp_test`` (their
restatements of tests/cond_grad_ref.py where d / d ys is wanted), ``vjp_ref._stages``, the Tsit5 tables -- with the terminal
cotangent

    lam_z(t_end) = cot_z,    lam_dlogp = +cot_logq,    lam_E = lam_n = 0

(the E and n rows are integrated when lam1, lam2 != 0 but are not outputs of sampling) and, once the sweep has reached
u(t_start) = [z0; 0],

    grad_z0 = lam_z(t_start) + cot_logq d logpdf(basedist, z0) / d z0            (N(0, I): -cot_logq z0)

tests/test_gen_vjp_ref_host.py pins it by torch float64 autograd and by central differences.  Nothing under oracle/ is changed.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import cnf_grad_oracle as G
from oracle import cnf_oracle as O
from tests import cond_grad_ref as CR
from tests import vjp_ref as V


def _span(cfg):
    """The span sampling integrates over: reverse(tspan)."""
    return cfg.tspan[1], cfg.tspan[0]


def base_logpdf(z0, base=None):
    z0 = np.asarray(z0)
    if base is None:
        return (-0.5 * (z0.shape[0] * math.log(2.0 * math.pi) + np.sum(z0 * z0, axis=0))).astype(z0.dtype)
    return base.logpdf(z0).astype(z0.dtype)


def forward(cfg, flat, z0, eps, dts, ys=None, train=True, base=None):
    """(z [n_in x B], logq [B], us, f) through the steps ``dts`` (absolute sizes), in the dtype of ``z0``."""
    z0 = np.asarray(z0)
    D = cfg.D(train)
    u0 = np.vstack([z0, np.zeros((D - cfg.n_in, z0.shape[1]), dtype=z0.dtype)])
    f = cfg.rhs(flat, eps if train else None, train, ys)
    t0, t1 = _span(cfg)
    us = G.forward_record(f, u0, t0, t1, [abs(float(d)) for d in dts])
    fsol = us[-1]
    logq = (base_logpdf(z0, base) + fsol[cfg.n_in]).astype(fsol.dtype)
    return fsol[:cfg.n_in].copy(), logq, us, f


def vjp(cfg, flat, z0, eps, cot_z, cot_logq, dts, ys=None, train=True, base=None):
    """(z, logq, grad, grad_z0, grad_ys): grad = sum_b <cot, d (z_b, logq_b) / d flat>, grad_z0 (n_in x B) and grad_ys
    (n_cond x B; None without ``ys``) likewise, through the fixed steps ``dts``, in the dtype of ``flat``.  ``cot_z``: n_in x B
    (or nvars x B: the rows beyond are zero), ``cot_logq``: B; None = zeros."""
    flat = np.asarray(flat)
    dts = [abs(float(d)) for d in dts]
    z, logq, us, f = forward(cfg, flat, z0, eps, dts, ys, train, base)
    fsol = us[-1]
    T = fsol.dtype.type
    n_in, B = cfg.n_in, fsol.shape[1]
    cz = np.zeros((n_in, B), dtype=fsol.dtype)
    if cot_z is not None:
        c = np.asarray(cot_z).astype(fsol.dtype)
        cz[:c.shape[0]] = c
    cl = np.zeros(B, dtype=fsol.dtype) if cot_logq is None else np.asarray(cot_logq).astype(fsol.dtype).reshape(B)
    lam = np.zeros_like(fsol)
    lam[:n_in] = cz
    lam[n_in] = cl                                      # rows E, n (TrainMode) stay zero
    grad = np.zeros(flat.size, dtype=flat.dtype)
    gy = None if ys is None else np.zeros_like(np.asarray(ys), dtype=fsol.dtype)
    A, Bc = O.TSIT5_A, O.TSIT5_B
    nz, nj = cfg.lam1 != 0, cfg.lam2 != 0
    t0, t1 = _span(cfg)
    tdir = 1.0 if t1 >= t0 else -1.0
    wl = lam[n_in][None, :]
    lz = lam[:n_in].copy()
    for n in reversed(range(len(dts))):
        h = T(tdir * dts[n])
        Us = V._stages(f, us[n], h, T)
        ws = [None] * 6
        for i in reversed(range(6)):
            if train:
                kbar = T(Bc[i]) * lam
                for m in range(i + 1, 6):
                    kbar[:n_in] += T(A[m][i]) * ws[m]
                if ys is None:
                    ws[i], g = G.rhs_vjp(cfg.net, flat, Us[i][:n_in], eps, h * kbar, nz, nj, cfg.use_jvp)
                else:
                    hbar, g = CR.rhs_vjp_full(cfg.net, flat, Us[i][:n_in], eps, h * kbar, nz, nj, cfg.use_jvp, ys)
            else:
                kb = T(Bc[i]) * lz
                for m in range(i + 1, 6):
                    kb = kb + T(A[m][i]) * ws[m]
                if ys is None:
                    ws[i], g = G.rhs_vjp_test(cfg.net, flat, Us[i][:n_in], h * kb, h * T(Bc[i]) * wl)
                else:
                    hbar, g = CR.rhs_vjp_test_full(cfg.net, flat, Us[i][:n_in], h * kb, h * T(Bc[i]) * wl, ys)
            if ys is not None:
                ws[i] = hbar[:n_in]
                gy += hbar[n_in:]
            grad += g
        if train:
            lam = lam.copy()
            for i in range(6):
                lam[:n_in] += ws[i]
        else:
            lz = lz + sum(ws)
    lam0 = (lam if train else lz)[:n_in]
    z0 = np.asarray(z0).astype(fsol.dtype)
    neg = z0 if base is None else base.neg_grad(z0).astype(fsol.dtype)          # -d logpdf / d z0
    gz0 = lam0 - cl[None, :] * neg
    return z, logq, grad, gz0, gy


def vjp64(cfg, flat, z0, eps, cot_z, cot_logq, dts, ys=None, train=True, base=None):
    c = lambda a: V._cast(a, np.float64)
    return vjp(cfg, c(flat), c(z0), c(eps), c(cot_z), c(cot_logq), dts, c(ys), train, base)


def vjp32(cfg, flat, z0, eps, cot_z, cot_logq, dts, ys=None, train=True, base=None):
    c = lambda a: V._cast(a, np.float32)
    return vjp(cfg, c(flat), c(z0), c(eps), c(cot_z), c(cot_logq), dts, c(ys), train, base)


def case_z0(case):
    """The base draw of a case of tests/grad_terms.py: n_in x B, seed + 11."""
    return np.random.default_rng(case.seed + 11).standard_normal((case.nvars + case.naugs, case.B)).astype(np.float32)


def cotangents(rng, n_in, nvars, B, aug_rows=False):
    """name -> (cot_z or None, cot_logq or None), entries N(0, 1)/B: the sample rows alone, logq alone, both; with ``aug_rows``
    one more with a cotangent on all n_in rows of the final state."""
    d = lambda *s: (rng.standard_normal(s) / B).astype(np.float32)
    out = {"x": (d(nvars, B), None), "logq": (None, d(B)), "both": (d(nvars, B), d(B))}
    if aug_rows:
        out["z-all-rows"] = (d(n_in, B), d(B))
    return out


def fixed_dts(case):
    return CR.case_dts(case)
