"""``EnsembleBases``: a Gaussian base distribution of its own for every member of an ensemble call, N(mean_m, L_m L_m') --
``basedist`` of ``construct`` (src/base_icnf.jl:16-21) per member (include/cnfhip_ensemble_base.h).  Each fold of a k-fold split
has the mean and scale of its own training rows; each restart of a variational fit its own learnable location-scale family; the
components of a mixture sit in different places.  The ensemble calls take it as ``bases=``; the values are reduced on the
device in stream order (cnf_ensemble_set_bases), so a learnable base costs no host wait per optimiser step."""
from __future__ import annotations

import numpy as np

from .distributions import KIND_DENSE, KIND_DIAG, DiagNormal, MvNormal


def _is_torch(x):
    return hasattr(x, "detach") and hasattr(x, "is_cuda")


class EnsembleBases:
    """``EnsembleBases(mean, std=... | scale_tril=...)``: ``mean`` is (M, n_in); ``std`` is (M, n_in), every entry > 0 (the
    diagonal kind), or ``scale_tril`` is (M, n_in, n_in), lower triangular with a positive diagonal (the dense kind; what lies
    above the diagonal is not read) -- exactly one of the two.  numpy arrays are constant bases: they are checked here and moved
    to the device once.  torch tensors are held as they are and may require grad (``std = log_std.exp()`` keeps the positivity
    constraint in the caller's graph): their current values are read by every call; values on the host are checked before the
    upload, values on the device by the device (a member whose scale is not positive or not finite fails its call, naming
    it).  ``bases[m]`` is the ``DiagNormal`` / ``MvNormal`` of member m; ``bases[lo:hi]`` the bases of those members.  Shape and
    dtype errors are ``ValueError``s."""

    def __init__(self, mean, std=None, scale_tril=None):
        if (std is None) == (scale_tril is None):
            raise ValueError("EnsembleBases takes exactly one of std and scale_tril")
        scale, name = (std, "std") if scale_tril is None else (scale_tril, "scale_tril")
        self.kind = KIND_DIAG if scale_tril is None else KIND_DENSE
        self.mean, self.scale = self._array(mean, "mean"), self._array(scale, name)
        if _is_torch(self.mean) != _is_torch(self.scale):
            raise ValueError(f"EnsembleBases: mean and {name} must both be numpy arrays or both be torch tensors")
        ms = tuple(self.mean.shape)
        if len(ms) != 2 or ms[0] < 1 or ms[1] < 1:
            raise ValueError(f"mean must be (M, n_in), got {ms}")
        want = ms if self.kind == KIND_DIAG else ms + (ms[1],)
        if tuple(self.scale.shape) != want:
            raise ValueError(f"{name} must be {want}, got {tuple(self.scale.shape)}")
        self._name, self._dev = name, {}
        self._check_host_values()

    @staticmethod
    def _array(a, name):
        if _is_torch(a):
            if not a.dtype.is_floating_point:
                raise ValueError(f"{name} must be a floating-point tensor, got {a.dtype}")
            return a
        a = np.asarray(a)
        if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)) or a.dtype == np.bool_:
            raise ValueError(f"{name} must be a real array, got dtype {a.dtype}")
        return np.ascontiguousarray(a, dtype=np.float64)

    def _host(self, a):
        """The values of ``a`` as float64 on the host, or None when reading them would wait for a device."""
        if _is_torch(a):
            return None if a.is_cuda else a.detach().double().numpy()
        return a

    def _check_host_values(self):
        mu, sc = self._host(self.mean), self._host(self.scale)
        if mu is not None and not np.isfinite(mu).all():
            raise ValueError("mean must be finite")
        if sc is None:
            return
        if self.kind == KIND_DENSE:
            sc = np.tril(sc)
        if not np.isfinite(sc).all():
            raise ValueError(f"{self._name} must be finite")
        d = sc if self.kind == KIND_DIAG else np.diagonal(sc, axis1=1, axis2=2)
        if not (d > 0).all():
            bad = int(np.argwhere(~(d > 0))[0][0])
            raise ValueError(f"{self._name}: member {bad} has a non-positive {'entry' if self.kind == KIND_DIAG else 'diagonal'}")

    def __len__(self):
        return int(self.mean.shape[0])

    @property
    def n_in(self):
        return int(self.mean.shape[1])

    @property
    def is_torch(self):
        return _is_torch(self.mean)

    @property
    def requires_grad(self):
        return bool(self.is_torch and (self.mean.requires_grad or self.scale.requires_grad))

    def __repr__(self):
        return f"EnsembleBases(M={len(self)}, n_in={self.n_in}, {'diagonal' if self.kind == KIND_DIAG else 'dense'})"

    def __getitem__(self, m):
        if isinstance(m, slice):
            return EnsembleBases(self.mean[m], **{self._name: self.scale[m]})
        m = int(m)
        if not -len(self) <= m < len(self):
            raise IndexError(f"member {m} of {len(self)}")
        host = lambda a: a[m].detach().cpu().double().numpy() if _is_torch(a) else a[m]
        mu, sc = host(self.mean), host(self.scale)
        if self.kind == KIND_DIAG:
            return DiagNormal(mu, sc)
        L = np.tril(sc)
        return MvNormal(mu, L @ L.T)

    def take(self, idx):
        """The bases of the members ``idx`` (a sequence of indices), in that order."""
        idx = [int(i) for i in idx]
        if _is_torch(self.mean):
            import torch
            ix = torch.as_tensor(idx, device=self.mean.device)
            return EnsembleBases(self.mean[ix], **{self._name: self.scale[ix]})
        return EnsembleBases(self.mean[idx], **{self._name: self.scale[idx]})

    def tensors(self, dev):
        """``(mean, scale)`` as torch tensors on ``dev``, attached to the caller's graph when they are tensors that require grad
        (numpy arrays: moved once per device and kept)."""
        import torch
        if not self.is_torch:
            key = str(dev)
            if key not in self._dev:
                self._dev[key] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (self.mean, self.scale))
            return self._dev[key]
        return self.mean.to(dev), self.scale.to(dev)

    def device_values(self, dev):
        """``(mean, scale)``: what the device reads -- detached float32 contiguous tensors on ``dev`` holding the current values
        (checked here when they live on the host)."""
        import torch
        if self.is_torch:
            self._check_host_values()
        return tuple(a.detach().to(torch.float32).contiguous() for a in self.tensors(dev))
