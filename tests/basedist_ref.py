"""Float64 restatement of the Gaussian base distribution and of the Rademacher contract, for the tests of
``basedist`` / ``epsdist`` (src/base_icnf.jl:16-25).  Independent of continuousnf.jl_amd/distributions.py: that module's
(mu, W, c) reduction is checked against this file and scipy, not against itself.

The float64 expectations of a model with a non-default base are built from the oracle's public pieces with two of them
supplied from here: ``inference_sol`` (the log-density of the final state) and ``final_cotangent`` (d loss / d u(t1))."""
import contextlib
import math

import numpy as np

from oracle import cnf_grad_oracle as G
from oracle import cnf_oracle as O
from tests import philox_ref as P


class Gauss:
    """N(mean, cov), ``cov`` a scalar, a vector (diagonal) or a full matrix; everything float64."""

    def __init__(self, mean, cov):
        self.mean = np.asarray(mean, dtype=np.float64)
        n = self.mean.size
        c = np.asarray(cov, dtype=np.float64)
        if c.ndim == 0:
            c = np.full(n, float(c))
        self.cov = np.diag(c) if c.ndim == 1 else c
        self.L = np.linalg.cholesky(self.cov)
        self.prec = np.linalg.inv(self.cov)
        self.logdet = 2.0 * float(np.sum(np.log(np.diag(self.L))))

    def logpdf(self, z):
        """z: (n, B)."""
        d = np.asarray(z, dtype=np.float64) - self.mean[:, None]
        q = np.sum(d * np.linalg.solve(self.cov, d), axis=0)
        return -0.5 * (self.mean.size * math.log(2.0 * math.pi) + self.logdet + q)

    def neg_grad(self, z):
        """-d logpdf / d z = inv(cov) (z - mean); z: (n, B)."""
        return np.linalg.solve(self.cov, np.asarray(z, dtype=np.float64) - self.mean[:, None])

    def sample_from(self, normals):
        return self.mean[:, None] + self.L @ np.asarray(normals, dtype=np.float64)


_O_INFERENCE_SOL, _G_FINAL_COTANGENT = O.inference_sol, G.final_cotangent      # the oracle's own, whatever is patched in later


def inference_sol(g: Gauss, cfg: O.Cfg, fsol, train: bool):
    """O.inference_sol (src/base_icnf.jl:167-189) with logpdf(basedist, z) in place of MvNormal(0, I)."""
    _, regs = _O_INFERENCE_SOL(cfg, fsol, train)
    return g.logpdf(fsol[:cfg.n_in]) - fsol[cfg.n_in], regs


def final_cotangent(g: Gauss, cfg: O.Cfg, fsol):
    """G.final_cotangent with -d logpdf(basedist, z) / d z = inv(cov) (z - mean) on the z rows in place of z."""
    lam = _G_FINAL_COTANGENT(cfg, fsol)
    n_in, B = cfg.n_in, fsol.shape[1]
    lam[:n_in] += (g.neg_grad(fsol[:n_in]) - fsol[:n_in]) / B
    return lam


@contextlib.contextmanager
def oracle_with(g: Gauss):
    """Inside the block the oracle's drivers (O.inference, G.loss_and_grad, G.loss_and_grad_test) evaluate the base
    distribution ``g``: the two pieces above take the place of their N(0, I) counterparts; nothing under oracle/ changes."""
    O.inference_sol = lambda cfg, fsol, train: inference_sol(g, cfg, fsol, train)
    G.final_cotangent = lambda cfg, fsol: final_cotangent(g, cfg, fsol)
    try:
        yield
    finally:
        O.inference_sol, G.final_cotangent = _O_INFERENCE_SOL, _G_FINAL_COTANGENT


def random_cov(rng, n, kind):
    """A covariance with eigenvalues drawn log-uniformly in [0.1, 10]: 'scalar', 'diag' or 'full'."""
    ev = np.exp(rng.uniform(np.log(0.1), np.log(10.0), size=n))
    if kind == "scalar":
        return float(ev[0])
    if kind == "diag":
        return ev
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    c = (q * ev) @ q.T
    return 0.5 * (c + c.T)


# ---- Rademacher contract: element e is +1 if bit 31 of word e is 0, -1 if it is 1 ----
def rademacher_of_words(words):
    w = np.asarray(words, dtype=np.uint32)
    return (1.0 - 2.0 * (w >> np.uint32(31)).astype(np.float64)).astype(np.float32)


def rademacher(seed, sub, offset, n):
    return rademacher_of_words(P.uint32(seed, sub, offset, n))


def loss_and_grad_test(g: Gauss, cfg: O.Cfg, flat, xs, dts, ys=None):
    """G.loss_and_grad_test on the replayed steps ``dts`` with the base distribution ``g``: the same discrete adjoint from the
    oracle's pieces (forward_record, rhs_vjp_test), started from d loss / d z(t1) = inv(cov) (z - mean) / B."""
    flat = np.asarray(flat)
    u0 = O.inference_u0(cfg, xs, False)
    f = cfg.rhs(flat, None, False, ys)
    st = O.SolveStats(naccept=len(dts), dts=[abs(float(d)) for d in dts])
    us = G.forward_record(f, u0, cfg.tspan[0], cfg.tspan[1], st.dts)
    fsol = us[-1]
    logpx, _ = inference_sol(g, cfg, fsol, False)
    val = float(-np.mean(logpx))
    T = u0.dtype.type
    tdir = 1.0 if cfg.tspan[1] >= cfg.tspan[0] else -1.0
    n_in, B = cfg.n_in, xs.shape[1]
    lam, lam_l = g.neg_grad(fsol[:n_in]) / B, 1.0 / B
    grad = np.zeros(flat.size, dtype=flat.dtype)
    A, Bc = O.TSIT5_A, O.TSIT5_B
    for n in reversed(range(len(st.dts))):
        h, u = T(tdir * st.dts[n]), us[n]
        ks, Us = [], []
        for s in range(6):
            acc = np.zeros_like(u)
            for j in range(s):
                acc = acc + T(A[s][j]) * ks[j]
            Us.append(u + h * acc)
            ks.append(f(Us[-1]))
        ws = [None] * 6
        for i in reversed(range(6)):
            kb = T(Bc[i]) * lam
            for m in range(i + 1, 6):
                kb = kb + T(A[m][i]) * ws[m]
            ws[i], gi = G.rhs_vjp_test(cfg.net, flat, Us[i][:n_in], h * kb, h * T(Bc[i]) * lam_l, ys)
            grad += gi
        lam = lam + sum(ws)
    st.grad_x = lam[:cfg.nvars].copy()
    return val, grad, st
