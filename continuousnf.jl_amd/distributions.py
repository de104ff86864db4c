"""``basedist`` / ``epsdist`` of ``construct`` (src/base_icnf.jl:16-25): the Gaussian base distributions whose log-density
``inference_sol`` evaluates at the final state (:155, :177) and ``generate_prob`` samples (:320-393), and the probe
distributions ``rand!(rng, icnf.epsdist, eps)`` draws from (:233-397).

Every Gaussian reduces to ``(mu, W, c)``, computed once here in float64 and rounded once to float32: ``W = inv(L)`` with
``Sigma = L L'`` (the vector ``1 / sigma`` in the diagonal case, a lower-triangular matrix otherwise) and
``c = sum(log W_ii) - n/2 log(2 pi)``, so that

    logpdf(z)      = c - 1/2 |W (z - mu)|^2
    d logpdf / d z = -W' W (z - mu)
    sample         = mu + L n,   n ~ N(0, I)

``MvNormal`` / ``DiagNormal`` are constants.  ``LearnableNormal(mean, scale_tril=... | std=...)`` is the same Gaussian held as
torch tensors ``mu`` and ``L`` (the lower-triangular factor, or the vector ``sigma``): every call that solves uploads their
current values (cnf_set_basedist) when a tensor's identity or in-place version changed, and the differentiable calls
(``differentiable_inference``, ``icnf(xs, ps, st)``, ``differentiable_generate``, ``reverse_kl``; ``with_base=True`` of the
pullbacks and of ``loss_and_grad``) return

    d/d mu sum_b w_b logpdf(z_b) = W' sum_b w_b n_b,                                         n_b = W (z_b - mu)
    d/d L  sum_b w_b logpdf(z_b) = tril(W' sum_b w_b n_b n_b') - (sum_b w_b) diag(1 / L_ii)

(cnf_base_logpdf_pullback) and, for samples drawn as ``mu + L n``, the pullback of that draw (cnf_base_sample_pullback).
Every upload is synchronous: one host wait per optimiser step on the base.  The built-in ``fit`` keeps the base constant and
optimises ``ps`` only -- training a base goes through a custom loss and a torch optimiser; the ``_host`` entry points, the
submitted gradients, the in-launch gradient of small networks and the Julia shims do not return the base's gradient."""
from __future__ import annotations

import numpy as np

KIND_DEFAULT, KIND_DIAG, KIND_DENSE = 0, 1, 2     # cnf_set_basedist's `kind`
_LOG2PI = float(np.log(2.0 * np.pi))


def _finite(a, name):
    a = np.asarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be finite")
    return a


class MvNormal:
    """``MvNormal(mean, cov)``: ``cov`` a scalar (sigma^2 I), a vector (the diagonal of Sigma) or a full symmetric
    positive-definite matrix.  ``len(mean)`` must be ``nvars + naugmented`` of the model it is given to."""

    def __init__(self, mean, cov):
        mu = self._mean(mean)
        n = mu.size
        c = _finite(cov, "cov")
        if c.ndim == 0:
            c = np.full(n, float(c))
        if c.ndim == 1:
            if c.size != n:
                raise ValueError(f"cov has {c.size} entries, mean has {n}")
            if not np.all(c > 0):
                raise ValueError("cov: every variance must be > 0")
            self._set(mu, KIND_DIAG, np.sqrt(c), 1.0 / np.sqrt(c))
        elif c.ndim == 2:
            if c.shape != (n, n):
                raise ValueError(f"cov is {c.shape[0]} x {c.shape[1]}, mean has {n} entries")
            if not np.allclose(c, c.T, rtol=1e-10, atol=1e-12 * float(np.max(np.abs(c)))):
                raise ValueError("cov must be symmetric")
            try:
                L = np.linalg.cholesky(0.5 * (c + c.T))
            except np.linalg.LinAlgError:
                raise ValueError("cov must be positive definite (its Cholesky factorisation failed)") from None
            W = np.tril(np.linalg.solve(L, np.eye(n)))       # inv(L): lower triangular, the upper part exactly 0
            self._set(mu, KIND_DENSE, L, W)
        else:
            raise ValueError("cov must be a scalar, a vector or a matrix")

    @staticmethod
    def _mean(mean):
        mu = _finite(mean, "mean")
        if mu.ndim != 1 or mu.size < 1:
            raise ValueError("mean must be a non-empty vector")
        return mu

    def _set(self, mu, kind, chol, whiten):
        n = mu.size
        self.kind = kind
        self.mean64, self.chol64, self.whiten64 = mu, chol, whiten
        d = whiten if kind == KIND_DIAG else np.diag(whiten)
        self.logconst64 = float(np.sum(np.log(d))) - 0.5 * n * _LOG2PI
        # what the device gets: rounded once (dense matrices row-major)
        self.mean = np.ascontiguousarray(mu, dtype=np.float32)
        self.whiten = np.ascontiguousarray(whiten, dtype=np.float32)
        self.chol = np.ascontiguousarray(chol, dtype=np.float32)
        self.logconst = float(np.float32(self.logconst64))
        dw = self.whiten if kind == KIND_DIAG else np.diag(self.whiten)
        dl = self.chol if kind == KIND_DIAG else np.diag(self.chol)
        if not (np.all(np.isfinite(self.whiten)) and np.all(np.isfinite(self.chol)) and np.isfinite(self.logconst)
                and np.all(dw > 0) and np.all(dl > 0)):
            raise ValueError("cov is outside what float32 holds")

    def __len__(self):
        return self.mean64.size

    def __repr__(self):
        return f"{type(self).__name__}(n={len(self)}, {'diagonal' if self.kind == KIND_DIAG else 'dense'})"

    def _cols(self, v, like):
        return v if like.ndim == 1 else v[:, None]

    def logpdf(self, z):
        """float64 on the host, in the (mu, W, c) form the device evaluates; ``z``: (n,) or (n, B)."""
        z = np.asarray(z, dtype=np.float64)
        d = z - self._cols(self.mean64, z)
        w = self._cols(self.whiten64, z) * d if self.kind == KIND_DIAG else self.whiten64 @ d
        return self.logconst64 - 0.5 * np.sum(w * w, axis=0)

    def sample_from(self, normals):
        """``mu + L n`` for standard normals ``n`` ((n,) or (n, B)), float64."""
        nrm = np.asarray(normals, dtype=np.float64)
        ln = self._cols(self.chol64, nrm) * nrm if self.kind == KIND_DIAG else self.chol64 @ nrm
        return self._cols(self.mean64, nrm) + ln


class DiagNormal(MvNormal):
    """``DiagNormal(mean, std)``: independent components; ``std`` a vector or a scalar, every entry > 0."""

    def __init__(self, mean, std):
        mu = self._mean(mean)
        s = _finite(std, "std")
        if s.ndim == 0:
            s = np.full(mu.size, float(s))
        if s.ndim != 1 or s.size != mu.size:
            raise ValueError(f"std must be a scalar or a vector of {mu.size} entries")
        if not np.all(s > 0):
            raise ValueError("std must be > 0")
        self._set(mu, KIND_DIAG, s.copy(), 1.0 / s)


class LearnableNormal(MvNormal):
    """``LearnableNormal(mean, scale_tril=None, std=None)``: N(mean, L L') with ``L = tril(scale_tril)`` (``n x n``, positive
    diagonal) or N(mean, diag(std)^2) (``std``: ``n`` entries > 0) -- exactly one of the two.  ``mean`` and the scale are torch
    tensors on any device, leaves or not: ``std = log_std.exp()`` keeps the positivity constraint in the caller's graph.  The
    model reads their current values before every call that solves; give a new pair with ``update`` (or a new
    ``LearnableNormal`` assigned to ``icnf.basedist``) when the tensors themselves are recomputed each step."""

    def __init__(self, mean, scale_tril=None, std=None):
        self._seen = None
        self.update(mean, scale_tril=scale_tril, std=std)

    def update(self, mean, scale_tril=None, std=None):
        """Replace the tensors (same length) and reduce their values; raises ``ValueError`` as ``MvNormal`` does."""
        if (scale_tril is None) == (std is None):
            raise ValueError("LearnableNormal takes exactly one of scale_tril and std")
        scale = scale_tril if std is None else std
        for name, t in (("mean", mean), ("scale_tril" if std is None else "std", scale)):
            if not (hasattr(t, "detach") and hasattr(t, "_version")):
                raise ValueError(f"LearnableNormal: {name} must be a torch tensor")
        if getattr(self, "mean64", None) is not None and int(mean.numel()) != len(self):
            raise ValueError(f"mean has {int(mean.numel())} entries, the distribution has {len(self)}")
        self.mean_t, self.scale_t = mean, scale
        self.kind = KIND_DIAG if scale_tril is None else KIND_DENSE
        self._seen = None
        self.refresh()

    @property
    def requires_grad(self):
        return bool(self.mean_t.requires_grad or self.scale_t.requires_grad)

    def refresh(self):
        """Reduce the tensors' current values on the host in float64 (``MvNormal._set``) if a tensor's identity or in-place
        version changed since the last time; returns whether it did."""
        m, sc_t, p = self.mean_t, self.scale_t, self._seen
        if p is not None and p[0] is m and p[1] == m._version and p[2] is sc_t and p[3] == sc_t._version:
            return False
        seen = (m, m._version, sc_t, sc_t._version)       # the caller's tensors, held: identity, not address (ICNF.set_cond)
        mu = self._mean(self.mean_t.detach().cpu().double().numpy())
        n = mu.size
        sc = _finite(self.scale_t.detach().cpu().double().numpy(), "std" if self.kind == KIND_DIAG else "scale_tril")
        if self.kind == KIND_DIAG:
            if sc.ndim != 1 or sc.size != n:
                raise ValueError(f"std must be a vector of {n} entries")
            if not np.all(sc > 0):
                raise ValueError("std must be > 0")
            self._set(mu, KIND_DIAG, sc.copy(), 1.0 / sc)
        else:
            if sc.shape != (n, n):
                raise ValueError(f"scale_tril must be {n} x {n}")
            L = np.tril(sc)
            if not np.all(np.diag(L) > 0):
                raise ValueError("scale_tril: the diagonal must be > 0")
            self._set(mu, KIND_DENSE, L, np.tril(np.linalg.solve(L, np.eye(n))))
        self._seen = seen
        self.generation = getattr(self, "generation", 0) + 1      # (what a model compares to know whether it holds these values)
        return True


def learnable(basedist):
    """The ``LearnableNormal`` of a model, or ``ValueError``: what ``with_base=True`` needs."""
    if not isinstance(basedist, LearnableNormal):
        raise ValueError("with_base: the model's basedist is not a LearnableNormal (a constant base has no gradient)")
    return basedist


class StdNormal:
    """``epsdist``: N(0, I) probes -- the default, spelled out."""

    def __repr__(self):
        return "StdNormal()"


class Rademacher:
    """``epsdist``: entries +1 / -1 with probability 1/2 each (Hutchinson's original probes).  E[eps eps'] = I, so the
    trace estimate and the E / n rows of src/icnf.jl:349 keep their meaning; the diagonal of the Jacobian enters exactly."""

    def __repr__(self):
        return "Rademacher()"


SUPPORTED = "basedist: MvNormal(mean, cov), DiagNormal(mean, std), LearnableNormal(mean, scale_tril | std) or None; epsdist: StdNormal(), Rademacher() or None"


def check_basedist(basedist, n_in):
    """What ``construct`` accepts as ``basedist``: None (the default N(0, I)) or an MvNormal over n_in rows."""
    if basedist is None:
        return None
    if not isinstance(basedist, MvNormal):
        raise NotImplementedError(f"basedist {basedist!r} is not built ({SUPPORTED})")
    if len(basedist) != n_in:
        raise ValueError(f"basedist has length {len(basedist)}, the model has nvars + naugmented = {n_in} rows")
    return basedist


def check_epsdist(epsdist):
    """What ``construct`` accepts as ``epsdist``: None / StdNormal() (N(0, I): returns None) or Rademacher()."""
    if epsdist is None or isinstance(epsdist, StdNormal):
        return None
    if isinstance(epsdist, Rademacher):
        return epsdist
    raise NotImplementedError(f"epsdist {epsdist!r} is not built ({SUPPORTED})")
