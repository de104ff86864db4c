"""The device generator: ``HIPRNG`` is this mirror's counterpart of the reference's
``rng_AT(::CUDALibs) = CURAND`` (ext/ContinuousNormalizingFlowsCUDAExt/ContinuousNormalizingFlowsCUDAExt.jl:5-7): with
``construct(..., rng=HIPRNG(seed))`` the Hutchinson probes eps (src/base_icnf.jl:277-278) and the base sample z0
(:367-370) are drawn on the GPU by ``cnf_draw_normal`` (Philox4x32-10 + Box-Muller, csrc/cnf_rand.hip) instead of on the
host by numpy.  Opt-in: ``rng=None``, an int or a numpy ``Generator`` keep the host draws.

Sharded runs: give every rank its own stream, ``HIPRNG(seed, subsequence=rank)``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

_U64 = (1 << 64) - 1


def _u64(v, name):
    v = int(v)
    if not 0 <= v <= _U64:
        raise ValueError(f"{name} must be in [0, 2**64)")
    return v


def _launch(fn, device, seed, subsequence, offset, out, n, stream):
    import torch
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    if out is None:
        out = torch.empty(n, dtype=torch.uint32 if fn == "cnf_draw_uint32" else torch.float32, device=dev)
    idx = out.device.index if out.device.index is not None else torch.cuda.current_device()
    if stream is None:
        stream = C.c_void_p(torch.cuda.current_stream(idx).cuda_stream)
    _lib.check(getattr(_lib.lib(), fn)(idx, _u64(seed, "seed"), _u64(subsequence, "subsequence"),
                                       _u64(offset, "offset"), out.data_ptr() if n else None, n, stream))
    return out


def draw_normal(n, seed, subsequence=0, offset=0, device=0, stream=None):
    """Elements ``offset .. offset + n - 1`` of stream ``(seed, subsequence)`` as N(0, 1) float32: a new CUDA tensor of n
    entries on ``device``, filled on ``stream`` (default: torch's current stream there).  Stateless."""
    return _launch("cnf_draw_normal", device, seed, subsequence, offset, None, int(n), stream)


def draw_rademacher(n, seed, subsequence=0, offset=0, device=0, stream=None):
    """The same elements as Rademacher values (float32): +1 where bit 31 of the element's word is 0, -1 where it is 1."""
    return _launch("cnf_draw_rademacher", device, seed, subsequence, offset, None, int(n), stream)


def draw_uint32(n, seed, subsequence=0, offset=0, device=0, stream=None):
    """The raw Philox4x32-10 words of the same elements (a torch.uint32 CUDA tensor)."""
    return _launch("cnf_draw_uint32", device, seed, subsequence, offset, None, int(n), stream)


class HIPRNG:
    """A seeded device stream.  ``offset`` is the index of the next element; every draw takes the next n elements and
    advances it by n on the host, when the draw is enqueued -- so a run is reproducible from ``(seed, subsequence)`` and
    can be resumed from ``get_state()``.  The few scalar and index draws of the API (``uniform`` for the steered end time,
    src/base_icnf.jl:108-121; ``permutation`` for ``fit``'s shuffle; the parameter initialisation of ``setup``) are not on
    the hot path and come from a host numpy generator seeded with ``seed``."""

    def __init__(self, seed, subsequence=0):
        self.seed = _u64(seed, "seed")
        self.subsequence = _u64(subsequence, "subsequence")
        self.offset = 0
        self._host = np.random.default_rng(self.seed)

    def __repr__(self):
        return f"HIPRNG(seed={self.seed}, subsequence={self.subsequence}, offset={self.offset})"

    def get_state(self):
        return {"seed": self.seed, "subsequence": self.subsequence, "offset": self.offset,
                "host": self._host.bit_generator.state}

    def set_state(self, state):
        self.seed = _u64(state["seed"], "seed")
        self.subsequence = _u64(state["subsequence"], "subsequence")
        self.offset = _u64(state["offset"], "offset")
        self._host = np.random.default_rng(self.seed)
        if "host" in state:
            self._host.bit_generator.state = state["host"]

    def take(self, n):
        """Reserve the next n elements: returns their first index and advances ``offset``."""
        n = int(n)
        if n < 0 or self.offset + n > _U64:
            raise ValueError("draw past the end of the stream")
        o = self.offset
        self.offset += n
        return o

    def normal(self, n, device, stream=None):
        """The next n N(0, 1) float32 values as a CUDA tensor on ``device``, drawn on ``stream``."""
        o = self.take(n)
        return draw_normal(n, self.seed, self.subsequence, o, device, stream)

    def rademacher(self, n, device, stream=None):
        """The next n Rademacher (+-1) float32 values as a CUDA tensor on ``device``; ``offset`` advances by n as for ``normal``."""
        o = self.take(n)
        return draw_rademacher(n, self.seed, self.subsequence, o, device, stream)

    # host draws (not on the hot path)
    def uniform(self, *args, **kwargs):
        return self._host.uniform(*args, **kwargs)

    def permutation(self, *args, **kwargs):
        return self._host.permutation(*args, **kwargs)
