"""Host-side mirror of src/base_icnf.jl for the batched (MatrixMode) hot path: ``construct``,
``inference_prob``, ``base_sol``, ``inference_sol``, ``inference`` and ``loss`` keep the
reference's names, argument meaning and error behaviour; every number is produced by
libcnfhip on the GPU.  Arrays follow the reference's shapes (``xs`` is ``nvars x B``, states
are ``D x B``) and may be numpy arrays (copied through the *_host entry points) or torch
CUDA tensors (used in place, on torch's current stream)."""
from __future__ import annotations

import atexit
import ctypes as C
import weakref
from dataclasses import dataclass, field
from typing import Any

import numpy as np

from . import _lib
from .distributions import LearnableNormal, Rademacher, check_basedist, check_epsdist, learnable
from .layers import Chain
from .rng import HIPRNG
from .types import (AbstractICNF, CondFFJORD, CondPlanar, CondRNODE, FFJORD, RNODE, HIPMatrixMode, HIPVecJacMatrixMode,
                    Mode, TestMode, TrainMode, _OutOfScope)

_KERNEL = {"auto": _lib.KERNEL_AUTO, "generic": _lib.KERNEL_GENERIC, "mfma": _lib.KERNEL_MFMA}


def _is_torch(x):
    return type(x).__module__.startswith("torch")


# Handles still open at interpreter exit are destroyed here, while the HIP runtime (and a profiler's
# tool library) are still alive: atexit hooks run before library destructors, and this one is
# registered after torch's, so it runs before torch tears its context down.  __del__ at interpreter
# teardown gives no such ordering.
_OPEN = {}


def _close_all():
    for ref in list(_OPEN.values()):
        ic = ref()
        if ic is not None:
            try:
                ic.close()
            except Exception:
                pass
    _OPEN.clear()


atexit.register(_close_all)


def _mode_id(mode) -> int:
    if isinstance(mode, type):
        mode = mode()
    if not isinstance(mode, Mode):
        raise TypeError("mode must be TrainMode() or TestMode()")
    return mode.cnf


# ---------------------------------------------------------------------------------------
# array plumbing: logical (rows, B) <-> Julia column-major bytes
# ---------------------------------------------------------------------------------------
class _Buf:
    """A float32 matrix with logical shape (rows, B) stored column-major (each column's
    rows contiguous), either host (numpy) or device (torch)."""

    def __init__(self, arr, rows, B, torch_mod=None):
        self.arr, self.rows, self.B, self.torch = arr, rows, B, torch_mod

    @property
    def ptr(self):
        if self.torch is not None:
            return self.arr.data_ptr()
        return self.arr.ctypes.data

    def flat2d(self):
        """(B, rows) row-major view of the storage (torch buffers)"""
        if self.arr.dim() == 2:
            return self.arr.t()
        return self.arr.view(self.B, self.rows)

    def view(self):
        """logical (rows, B) view without copying"""
        if self.torch is not None:
            if self.arr.dim() == 2:
                return self.arr                  # a column-major (rows, B) tensor taken as it came
            return self.arr.view(self.B, self.rows).t()
        return self.arr.reshape(self.B, self.rows).T


def _as_colmajor(x, rows=None, name="array"):
    """Return a _Buf over x's data laid out column-major (copying only if needed)."""
    if _is_torch(x):
        import torch
        if x.dim() != 2:
            raise ValueError(f"{name} must be a matrix")
        if rows is not None and x.shape[0] != rows:
            raise ValueError(f"{name} has {x.shape[0]} rows, expected {rows}")
        if not x.is_cuda:
            raise ValueError(f"{name}: torch tensors must live on the GPU (pass numpy for host data)")
        if x.dtype == torch.float32 and x.stride(0) == 1 and x.stride(1) == x.shape[0]:
            return _Buf(x, x.shape[0], x.shape[1], torch)    # already column-major: use the storage as it is
        t = x.t().contiguous().to(torch.float32).reshape(-1)   # (B, rows) row-major == col-major
        return _Buf(t, x.shape[0], x.shape[1], torch)
    a = np.asarray(x)
    if a.ndim != 2:
        raise ValueError(f"{name} must be a matrix")
    if rows is not None and a.shape[0] != rows:
        raise ValueError(f"{name} has {a.shape[0]} rows, expected {rows}")
    flat = np.ascontiguousarray(a.T, dtype=np.float32).reshape(-1)
    return _Buf(flat, a.shape[0], a.shape[1], None)


def _xs_colmajor(icnf, xs):
    """``_as_colmajor(xs, nvars)`` with the last device tensor's transposed copy kept (keyed on the tensor object and its
    in-place version counter, as the parameter cache is): a caller evaluating the same data again -- the reference's benchmark
    suite, a validation set per epoch -- pays for the transposition once."""
    if not _is_torch(xs):
        return _as_colmajor(xs, icnf.nvars, "xs")
    prev = getattr(icnf, "_xs_cache", None)
    if prev is not None and prev[0] is xs and prev[1] == xs._version:
        return prev[2]
    buf = _as_colmajor(xs, icnf.nvars, "xs")
    icnf._xs_cache = (xs, xs._version, buf)
    return buf


def _empty_like(ref: _Buf, rows, B):
    if ref.torch is not None:
        return _Buf(ref.torch.empty(rows * B, dtype=ref.torch.float32, device=ref.arr.device), rows, B, ref.torch)
    return _Buf(np.empty(rows * B, dtype=np.float32), rows, B, None)


def _stream(buf: _Buf):
    if buf.torch is not None:
        return C.c_void_p(buf.torch.cuda.current_stream(buf.arr.device).cuda_stream)
    return None


# ---------------------------------------------------------------------------------------
# ICNF (src/icnf.jl:69-104) + construct (src/base_icnf.jl:1-77)
# ---------------------------------------------------------------------------------------
@dataclass(eq=False)
class ICNF:
    tag: type
    nn: Chain
    nvars: int
    naugmented: int
    compute_mode: HIPMatrixMode
    inplace: bool
    tspan: tuple
    steer_rate: float
    sol_kwargs: dict
    rng: Any
    lambda1: float
    lambda2: float
    lambda3: float
    device: int = 0
    cond: bool = False          # COND type parameter (src/base_icnf.jl:44)
    n_cond: int = 0             # rows of ys = nn input size - (nvars + naugmented)
    basedist: Any = None        # src/base_icnf.jl:16-21; None: MvNormal(Zeros, Eye), else a distributions.MvNormal (a
                                # LearnableNormal is uploaded again whenever its tensors changed: set_basedist)
    epsdist: Any = None         # src/base_icnf.jl:22-25; None: N(0, I) probes, else distributions.Rademacher()
    _handle: Any = field(default=None, repr=False)
    _cond_id: Any = field(default=None, repr=False)
    _params_id: Any = field(default=None, repr=False)
    _base_id: Any = field(default=None, repr=False)

    # type parameters of the reference struct (src/base_icnf.jl:42-51)
    @property
    def AUGMENTED(self): return self.naugmented != 0
    @property
    def STEER(self): return self.steer_rate != 0
    @property
    def NORM_Z(self): return self.lambda1 != 0
    @property
    def NORM_J(self): return self.lambda2 != 0
    @property
    def NORM_Z_AUG(self): return self.lambda3 != 0

    def handle(self):
        if self._handle is None:
            l = _lib.lib()
            dims = (C.c_int32 * len(self.nn.dims))(*self.nn.dims)
            acts = (C.c_int32 * len(self.nn.acts))(*self.nn.acts)
            cfg = _lib.cnf_config(len(self.nn.layers), dims, acts, self.nvars, self.naugmented,
                                  self.compute_mode.ad, self.lambda1, self.lambda2, self.lambda3,
                                  self.device, self.n_cond)
            h = C.c_void_p()
            _lib.check(l.cnf_create(C.byref(h), C.byref(cfg)))
            self._handle = h
            _OPEN[id(self)] = weakref.ref(self)
            if self.basedist is not None:        # (the default never calls it: that handle launches what it always did)
                if isinstance(self.basedist, LearnableNormal):
                    self.basedist.refresh()
                self._upload_basedist()
        return self._handle

    def _upload_basedist(self):
        d = self.basedist
        _lib.check(_lib.lib().cnf_set_basedist(self._handle, d.kind, d.mean.ctypes.data, d.whiten.ctypes.data, d.chol.ctypes.data,
                                               d.logconst), self._handle)
        self._base_id = (d, getattr(d, "generation", 0))

    def set_basedist(self):
        """A ``LearnableNormal`` base: reduce and upload its current values (cnf_set_basedist, synchronous) if a tensor's
        identity or in-place version changed, or another ``LearnableNormal`` was assigned to ``basedist``, since the last
        upload.  Called by every call that solves (through ``set_params``); any other base was uploaded with the handle."""
        d = self.basedist
        if not isinstance(d, LearnableNormal):
            return
        if len(d) != self.nvars + self.naugmented:
            raise ValueError(f"basedist has length {len(d)}, the model has nvars + naugmented = {self.nvars + self.naugmented} rows")
        self.handle()
        d.refresh()
        if self._base_id is None or self._base_id[0] is not d or self._base_id[1] != d.generation:
            self._upload_basedist()

    def __call__(self, xs, ps, st, *, eps=None):
        """The Lux-layer form, src/base_icnf.jl:528-543: ``icnf(xs, ps, st)`` (conditional: ``icnf((xs, ys), ps, st)``)
        = ``(first(inference(icnf, TrainMode(), xs[, ys], ps, st)), st)``.  With a ``ps`` (or a ``ys``) that requires grad the
        call goes through ``vjp.differentiable_inference``: the result can be back-propagated to ``ps``, ``xs`` and ``ys``, and to
        the tensors of a ``LearnableNormal`` base (which triggers this route too when they require grad)."""
        from .types import TrainMode
        if (_is_torch(ps) and ps.requires_grad) or (self.cond and _is_torch(xs[1]) and xs[1].requires_grad) \
                or (isinstance(self.basedist, LearnableNormal) and self.basedist.requires_grad):
            from .vjp import differentiable_inference
            args = (xs[0], xs[1], ps, st) if self.cond else (xs, ps, st)
            return differentiable_inference(self, TrainMode(), *args, eps=eps)[0], st
        if self.cond:
            x, ys = xs
            return inference(self, TrainMode(), x, ys, ps, st, eps=eps)[0], st
        return inference(self, TrainMode(), xs, ps, st, eps=eps)[0], st

    def close(self):
        if self._handle is not None:
            _lib.lib().cnf_destroy(self._handle)
            self._handle = None
            self._params_id = None
            self._cond_id = None
            self._grad_ys_on = False
            _OPEN.pop(id(self), None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params_async(self, ps):
        """``set_params`` for a device tensor without host waits (cnf_set_params_async): the copy is enqueued on the current
        stream.  The parameter update between two submitted gradients (``loss_and_grad_submit``); every launch on this ICNF must
        go to that stream."""
        import torch
        if self.nn.planar is not None or not (_is_torch(ps) and ps.is_cuda):
            return self.set_params(ps)
        self.set_basedist()
        p = ps.detach().to(torch.float32).contiguous().reshape(-1)
        h = self.handle()
        st = C.c_void_p(torch.cuda.current_stream(p.device).cuda_stream)
        _lib.check(_lib.lib().cnf_set_params_async(h, p.data_ptr(), p.numel(), st), h)
        self._params_id = ("t", ps, ps._version)
        self._cond_id = None
        self._keep_ps = p                       # (the copy is in flight: keep its source)

    def set_params(self, ps):
        """Upload ``ps`` (the ``p`` of augmented_f) unless it is the vector already resident."""
        h = self.handle()
        l = _lib.lib()
        self.set_basedist()
        if self.nn.planar is not None:
            # (u, w, b) -> the MLP layout the kernels see (layers.Chain.to_internal); keyed on the caller's object below
            ps_ext = ps
            if _is_torch(ps):
                prev = self._params_id
                if prev is not None and prev[0] == "t" and prev[1] is ps_ext and prev[2] == ps_ext._version:
                    return
                import torch
                p = self.nn.to_internal(ps.detach().to(torch.float32)).contiguous()
                if p.is_cuda:
                    st = C.c_void_p(torch.cuda.current_stream(p.device).cuda_stream)
                    _lib.check(l.cnf_set_params(h, p.data_ptr(), p.numel(), st), h)
                    torch.cuda.current_stream(p.device).synchronize()
                else:
                    _lib.check(l.cnf_set_params_host(h, p.data_ptr(), p.numel()), h)
                self._params_id = ("t", ps_ext, ps_ext._version)
            else:
                p = np.ascontiguousarray(self.nn.to_internal(np.asarray(ps, dtype=np.float32)), dtype=np.float32)
                key = ("n", p.tobytes())
                if self._params_id is not None and self._params_id[0] == "n" and key == self._params_id:
                    return
                _lib.check(l.cnf_set_params_host(h, p.ctypes.data, p.size), h)
                self._params_id = key
            self._cond_id = None
            return
        if _is_torch(ps):
            # identity of a tensor this object keeps alive (+ its in-place version counter): an address
            # can be handed to a new tensor by the caching allocator, an object held here cannot
            prev = self._params_id
            if prev is not None and prev[0] == "t" and prev[1] is ps and prev[2] == ps._version:
                return
            key = ("t", ps, ps._version)
            import torch
            p = ps.detach().to(torch.float32).contiguous().reshape(-1)
            if p.is_cuda:
                st = C.c_void_p(torch.cuda.current_stream(p.device).cuda_stream)
                _lib.check(l.cnf_set_params(h, p.data_ptr(), p.numel(), st), h)
            else:
                _lib.check(l.cnf_set_params_host(h, p.data_ptr(), p.numel()), h)
        else:
            p = np.ascontiguousarray(np.asarray(ps), dtype=np.float32).reshape(-1)
            key = ("n", p.tobytes())
            if self._params_id is not None and self._params_id[0] == "n" and key == self._params_id:
                return
            _lib.check(l.cnf_set_params_host(h, p.ctypes.data, p.size), h)
        self._params_id = key
        self._cond_id = None        # the conditioning bias depends on the parameters

    def set_step_trace(self, cap_attempts: int):
        """Diagnostic (cnf_set_step_trace): what ``sol.stats`` / the integrator's step log would show if base_sol kept
        ``sol`` (src/base_icnf.jl:141-142).  Returns a (cap, 4) float32 CUDA tensor that every later one-launch solve on
        this handle fills with (t, signed h, EEst, accepted) per step attempt; ``0`` switches it off."""
        l, h = _lib.lib(), self.handle()
        if cap_attempts <= 0:
            _lib.check(l.cnf_set_step_trace(h, None, 0), h)
            self._trace = None
            return None
        import torch
        self._trace = torch.zeros(cap_attempts, 4, dtype=torch.float32, device=torch.device("cuda", self.device))
        _lib.check(l.cnf_set_step_trace(h, self._trace.data_ptr(), cap_attempts), h)
        return self._trace

    def solve_fallbacks(self) -> int:
        """One-launch solves of this handle that ran out of a wait and were run again on the streamed driver."""
        return int(_lib.lib().cnf_solve_fallbacks(self.handle()))

    def set_solve_wait(self, wait_us: int = 0, poll_limit: int = 0):
        """cnf_set_solve_wait: how long a wait inside a one-launch solve lasts (microseconds per tile a workgroup carries;
        default 2000) and / or how many polls it makes (1: every wait runs out at once) before the call falls back to the
        streamed driver.  0 keeps a value."""
        _lib.check(_lib.lib().cnf_set_solve_wait(self.handle(), int(wait_us), int(poll_limit)), self.handle())

    def set_shard_reduce(self, fn):
        """Lock-step sharded solves (cnf_set_shard_reduce): ``fn(values)`` receives a
        writable float32 numpy view of the local sums and must replace it IN PLACE by the sum over
        all shards (``parallel.make_shard_reduce`` builds one from a torch.distributed group).
        ``None`` switches back to independent per-shard solves."""
        l, h = _lib.lib(), self.handle()
        if fn is None:
            cb = _lib.shard_reduce_fn()          # NULL function pointer
        else:
            def _cb(ptr, n, _user):
                try:
                    fn(np.ctypeslib.as_array(ptr, shape=(n,)))
                    return 0
                except Exception:                # never unwind through the C frames
                    import traceback
                    traceback.print_exc()
                    return 1
            cb = _lib.shard_reduce_fn(_cb)
        _lib.check(l.cnf_set_shard_reduce(h, cb, None), h)
        self._shard_cb = cb                      # keep the trampoline alive as long as the handle uses it

    def set_cond(self, ys, B):
        """Hand ``ys`` (n_cond x B) to the device (cnf_set_cond) unless it is already resident."""
        if not self.cond:
            if ys is not None:
                raise ValueError("ys given to an unconditional model")
            return
        if ys is None:
            raise ValueError("conditional model: ys is required")
        yb = _as_colmajor(ys, self.n_cond, "ys")
        if yb.B != B:
            raise ValueError("ys must have one column per sample")
        if yb.torch is not None:
            prev = self._cond_id
            if prev is not None and prev[0] == "t" and prev[1] is ys and prev[2] == ys._version and prev[3] == B:
                return
            key = ("t", ys, ys._version, B)          # the caller's tensor, held: identity, not address
        else:
            key = ("n", yb.arr.tobytes(), B)
            if self._cond_id is not None and self._cond_id[0] == "n" and key == self._cond_id:
                return
        l, h = _lib.lib(), self.handle()
        if yb.torch is not None:
            _lib.check(l.cnf_set_cond(h, yb.ptr, B, _stream(yb)), h)
            self._keep_ys = yb.arr
        else:
            _lib.check(l.cnf_set_cond_host(h, yb.ptr, B), h)
        self._cond_id = key


def n_augment(icnf: ICNF, mode) -> int:
    """src/icnf.jl:106-108 (TrainMode -> 2), src/base_icnf.jl:79-81 (otherwise 0)."""
    return 2 if _mode_id(mode) == _lib.MODE_TRAIN else 0


def n_augment_input(icnf: ICNF) -> int:
    """src/base_icnf.jl:98-106."""
    return icnf.naugmented if icnf.AUGMENTED else 0


def construct(aicnf, nn: Chain, nvars: int, naugmented: int = 0, *, data_type=np.float32,
              compute_mode=None, inplace: bool = False, cond=None, resource=None,
              tspan=(0.0, 1.0), steer_rate: float = 0.0, sol_kwargs=None, rng=None,
              lambda1=None, lambda2=None, lambda3=0.0, device: int = 0, basedist=None, epsdist=None, **kw) -> ICNF:
    """src/base_icnf.jl:1-77.  Keyword names follow the reference; the lambdas may also be
    given under their Julia names via ``**{"λ₁": ...}``.  RNODE defaults lambda1 = lambda2 = 1e-2
    (src/base_icnf.jl:28-37), everything else 0."""
    for jl, py in (("λ₁", "lambda1"), ("λ₂", "lambda2"), ("λ₃", "lambda3")):
        if jl in kw:
            v = kw.pop(jl)
            if py == "lambda1": lambda1 = v
            elif py == "lambda2": lambda2 = v
            else: lambda3 = v
    if kw:
        raise TypeError(f"unknown keyword(s) {sorted(kw)}")
    # src/base_icnf.jl:16-25: both default to MvNormal(0, I) over the nvars + naugmented rows; a Gaussian base
    # (distributions.MvNormal / DiagNormal) and Rademacher probes are built, anything else is refused
    basedist = check_basedist(basedist, int(nvars) + int(naugmented))
    epsdist = check_epsdist(epsdist)
    if not (isinstance(aicnf, type) and issubclass(aicnf, AbstractICNF)):
        raise TypeError("first argument must be a model tag such as RNODE or FFJORD")
    if issubclass(aicnf, _OutOfScope):
        raise NotImplementedError(f"{aicnf.__name__}: not built")
    if cond is None:
        cond = issubclass(aicnf, (CondRNODE, CondFFJORD, CondPlanar))          # src/base_icnf.jl:14
    if np.dtype(data_type) != np.float32:
        raise NotImplementedError("the HIP backend computes in Float32 (the reference default, base_icnf.jl:6)")
    if compute_mode is None:
        compute_mode = HIPVecJacMatrixMode()
    if not isinstance(compute_mode, HIPMatrixMode):
        raise TypeError("compute_mode must be HIPVecJacMatrixMode() or HIPJacVecMatrixMode()")
    n_in = nvars + naugmented
    n_cond = nn.dims[0] - n_in if cond else 0
    if nn.dims[-1] != n_in or (not cond and nn.dims[0] != n_in) or (cond and n_cond < 1):
        raise ValueError(f"nn must map {n_in}{' + n_cond' if cond else ''} -> {n_in} (nvars + naugmented)")
    rn = issubclass(aicnf, (RNODE, CondRNODE))
    if lambda1 is None: lambda1 = 1e-2 if rn else 0.0
    if lambda2 is None: lambda2 = 1e-2 if rn else 0.0
    # rng: None (fresh host generator), an int seed, a numpy Generator, or a HIPRNG (eps and z0 drawn on the device)
    if rng is None:
        rng = np.random.default_rng()
    elif isinstance(rng, (int, np.integer)):
        rng = np.random.default_rng(int(rng))
    return ICNF(aicnf, nn, int(nvars), int(naugmented), compute_mode, bool(inplace),
                (float(tspan[0]), float(tspan[1])), float(steer_rate), dict(sol_kwargs or {}), rng,
                float(np.float32(lambda1)), float(np.float32(lambda2)), float(np.float32(lambda3)),
                int(device), bool(cond), int(n_cond), basedist, epsdist)


def steer_tspan(icnf: ICNF, mode):
    """src/base_icnf.jl:108-121: TrainMode + STEER -> t1' = t1 + |t1 - t0| * r, r ~ U(-s, s)."""
    t0, t1 = icnf.tspan
    if icnf.STEER and _mode_id(mode) == _lib.MODE_TRAIN:
        r = np.float32(icnf.rng.uniform(-icnf.steer_rate, icnf.steer_rate))
        return (t0, float(np.float32(abs(t1 - t0)) * r + np.float32(t1)))
    return (t0, t1)


# ---------------------------------------------------------------------------------------
# problem assembly, solve, post-processing
# ---------------------------------------------------------------------------------------
@dataclass
class ODEProblem:
    """What inference_prob returns in the reference (an SciMLBase.ODEProblem): here the
    pieces libcnfhip needs."""
    icnf: ICNF
    mode: Any
    u0: _Buf
    eps: Any          # _Buf or None
    tspan: tuple
    ps: Any
    stats: dict = field(default_factory=dict)


def draw_eps(icnf: ICNF, like: _Buf, B: int):
    """``rand!(icnf.rng, icnf.epsdist, eps)`` (src/base_icnf.jl:277-278): N(0, I) probes, or +-1 with
    ``epsdist=Rademacher()``.  With a ``HIPRNG`` they are drawn on the device (cnf_draw_normal / cnf_draw_rademacher) where
    ``like`` lives -- on ``icnf.device`` and copied back for host arrays, so that one seed gives one eps wherever the data are."""
    n_in = icnf.nvars + n_augment_input(icnf)
    rad = isinstance(icnf.epsdist, Rademacher)
    if isinstance(icnf.rng, HIPRNG):
        draw = icnf.rng.rademacher if rad else icnf.rng.normal
        if like.torch is not None:
            return _Buf(draw(n_in * B, like.arr.device, _stream(like)), n_in, B, like.torch)
        return _Buf(draw(n_in * B, icnf.device).cpu().numpy(), n_in, B, None)
    if rad:
        e = (1.0 - 2.0 * icnf.rng.integers(0, 2, size=(B, n_in))).astype(np.float32).reshape(-1)
    else:
        e = icnf.rng.standard_normal((B, n_in)).astype(np.float32).reshape(-1)
    if like.torch is not None:
        # through a small ring of PINNED staging buffers: the copy is enqueued (a pageable source makes the host wait for the
        # stream, which would put a bubble between two submitted gradients); a buffer is reused four draws later, long after
        # its copy (at most three launches are ever in flight)
        t = like.torch
        ring = getattr(icnf, "_eps_pin", None)
        if ring is None or ring[0].numel() < e.size:
            ring = icnf._eps_pin = [t.empty(max(e.size, 1024), dtype=t.float32).pin_memory() for _ in range(4)]
            icnf._eps_pin_i = 0
        buf = ring[icnf._eps_pin_i % 4]
        icnf._eps_pin_i += 1
        buf[:e.size].copy_(t.from_numpy(e))
        return _Buf(buf[:e.size].to(like.arr.device, non_blocking=True), n_in, B, t)
    return _Buf(e, n_in, B, None)


def _split_cond_args(icnf: ICNF, args):
    """Unconditional: (ps, st);  conditional: (ys, ps, st)  -- the reference's two method
    families (src/base_icnf.jl:266-286 vs :288-309)."""
    if icnf.cond:
        if len(args) < 2:
            raise TypeError("conditional model: call with (xs, ys, ps, st)")
        return args[0], args[1], (args[2] if len(args) > 2 else None)
    if len(args) < 1:
        raise TypeError("call with (xs, ps, st)")
    return None, args[0], (args[1] if len(args) > 1 else None)


def inference_prob(icnf: ICNF, mode, xs, *args, eps=None, tspan=None) -> ODEProblem:
    """src/base_icnf.jl:266-286 (``(xs, ps, st)``) and :288-309 (conditional: ``(xs, ys, ps, st)``).
    ``eps`` may be supplied (n_in x B) to make the call deterministic; by default it is drawn
    from icnf.rng as the reference does.  ``tspan``: the span to integrate instead of ``steer_tspan(icnf, mode)`` (no steer
    variate is drawn then)."""
    ys, ps, st = _split_cond_args(icnf, args)
    m = _mode_id(mode)
    xb = _xs_colmajor(icnf, xs)
    B = xb.B
    D = icnf.nvars + n_augment_input(icnf) + 1 + n_augment(icnf, mode)
    icnf.set_params(ps)
    icnf.set_cond(ys, B)
    u0 = _empty_like(xb, D, B)
    if xb.torch is not None:
        _lib.check(_lib.lib().cnf_build_u0(icnf.handle(), m, xb.ptr, u0.ptr, B, _stream(xb)), icnf.handle())
    else:
        v = u0.arr.reshape(B, D)
        v[:, :icnf.nvars] = xb.arr.reshape(B, icnf.nvars)
        v[:, icnf.nvars:] = 0.0
    if eps is not None:
        eb = _as_colmajor(eps, icnf.nvars + n_augment_input(icnf), "eps")
        if eb.B != B:
            raise ValueError("eps must have one column per sample")
    else:
        eb = draw_eps(icnf, xb, B)
    return ODEProblem(icnf, mode, u0, eb, tuple(tspan) if tspan is not None else steer_tspan(icnf, mode), ps)


def _solve_opts(icnf: ICNF, tspan):
    key = (tspan, tuple(sorted(icnf.sol_kwargs.items())), icnf.compute_mode.kernel)
    hit = getattr(icnf, "_opts_cache", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    opts = _solve_opts_build(icnf, tspan)
    icnf._opts_cache = (key, opts)
    return opts


def _solve_opts_build(icnf: ICNF, tspan):
    kw = dict(icnf.sol_kwargs)
    kernel = _KERNEL[icnf.compute_mode.kernel]
    adaptive = bool(kw.pop("adaptive", True))
    dt = float(kw.pop("dt", 0.0))
    if not adaptive and dt <= 0:
        raise ValueError("sol_kwargs: adaptive=false needs dt > 0")
    opts = _lib.cnf_solve_opts(
        tspan[0], tspan[1],
        float(kw.pop("abstol", 1e-6)), float(kw.pop("reltol", 1e-3)),   # OrdinaryDiffEq defaults
        dt, int(adaptive), int(min(kw.pop("maxiters", 100000), 2**31 - 1)), kernel)
    for ignored in ("progress", "save_everystep", "alg", "save_start", "save_end", "dense"):
        kw.pop(ignored, None)
    if kw:
        raise TypeError(f"unsupported sol_kwargs {sorted(kw)} (Tsit5 is fixed as the algorithm)")
    return opts


def base_sol(icnf: ICNF, prob: ODEProblem):
    """src/base_icnf.jl:137-143: solve and return the final ``D x B`` state (what
    ``get_fsol`` extracts).  The whole Tsit5 solve runs on the device in one C call."""
    l, h = _lib.lib(), icnf.handle()
    m = _mode_id(prob.mode)
    u0 = prob.u0
    out = _empty_like(u0, u0.rows, u0.B)
    opts = _solve_opts(icnf, prob.tspan)
    stats = _lib.cnf_solve_stats()
    if u0.torch is not None:
        _lib.check(l.cnf_solve_tsit5(h, m, u0.ptr, prob.eps.ptr if prob.eps else None, out.ptr,
                                     u0.B, C.byref(opts), C.byref(stats), _stream(u0)), h)
    else:
        _lib.check(l.cnf_solve_tsit5_host(h, m, u0.ptr, prob.eps.ptr if prob.eps else None, out.ptr,
                                          u0.B, C.byref(opts), C.byref(stats)), h)
    prob.stats = stats.as_dict()
    return out


def raise_if_no_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: the HIP backend has no CPU fallback")


def inference_sol(icnf: ICNF, mode, prob: ODEProblem):
    """src/base_icnf.jl:167-189: returns ``(logp_x, (E, n, A))``; each entry has B elements."""
    fsol = base_sol(icnf, prob)
    return _post(icnf, mode, fsol)


def _post(icnf, mode, fsol: _Buf):
    l, h = _lib.lib(), icnf.handle()
    m = _mode_id(mode)
    B = fsol.B
    if fsol.torch is not None:
        t = fsol.torch
        logpx = t.empty(B, dtype=t.float32, device=fsol.arr.device)
        regs = t.empty(3 * B, dtype=t.float32, device=fsol.arr.device)
        _lib.check(l.cnf_inference_post(h, m, fsol.ptr, logpx.data_ptr(), regs.data_ptr(), B, _stream(fsol)), h)
        r = regs.view(3, B)
    else:
        import torch
        raise_if_no_gpu()
        dev = torch.device("cuda", icnf.device)
        df = torch.from_numpy(fsol.arr).to(dev)
        dl = torch.empty(B, dtype=torch.float32, device=dev)
        dr = torch.empty(3 * B, dtype=torch.float32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(l.cnf_inference_post(h, m, df.data_ptr(), dl.data_ptr(), dr.data_ptr(), B, st), h)
        logpx = dl.cpu().numpy()
        r = dr.cpu().numpy().reshape(3, B)
    return logpx, (r[0], r[1], r[2])


def generate_prob(icnf: ICNF, mode, ps, st, n: int, *, ys=None, z0=None, eps=None, tspan=None) -> ODEProblem:
    """src/base_icnf.jl:358-380 (first row of SURVEY.md 8f): the sampling problem -- the same
    right-hand side integrated over ``reverse(tspan)`` from a draw of the base distribution.
    ``z0`` ((nvars+naugs) x n) and ``eps`` may be supplied to make the call deterministic;
    by default both are drawn from icnf.rng (``rand!(rng, icnf.basedist, new_xs)``, ``rand!(rng, icnf.epsdist, eps)``); with a
    ``HIPRNG`` on the device, z0 first and eps from the elements after it, and the sample comes back as a device tensor.  A
    non-default ``basedist`` takes the standard normals the default would have drawn through ``mu + L n`` on the device
    (cnf_base_sample), wherever they were drawn; a ``z0`` given by the caller is used as it is.  ``tspan``: the span whose
    reverse is integrated instead of ``steer_tspan(icnf, mode)`` (no steer variate is drawn then)."""
    n_in = icnf.nvars + n_augment_input(icnf)
    D = n_in + 1 + n_augment(icnf, mode)
    zb, eb = _generate_inputs(icnf, mode, ps, n, ys, z0, eps)
    u0 = _empty_like(zb, D, n)
    v = u0.arr.view(n, D) if u0.torch is not None else u0.arr.reshape(n, D)
    src = zb.flat2d() if zb.torch is not None else zb.arr.reshape(n, n_in)
    v[:, :n_in] = src
    v[:, n_in:] = 0.0                                   # zrs = zeros(n_aug + 1, n)  (:367-368)
    t0, t1 = tspan if tspan is not None else steer_tspan(icnf, mode)
    return ODEProblem(icnf, mode, u0, eb, (t1, t0), ps)  # reverse(tspan)  (:377)


def _generate_inputs(icnf: ICNF, mode, ps, n: int, ys=None, z0=None, eps=None, normals_out=None):
    """What ``generate_prob`` uploads and draws, in its order: parameters, conditioning, the base draw ``z0`` and the probes
    ``eps`` (n_in x n each, as _Buf).  ``normals_out``: a list that receives the standard normals a non-default base turned
    into ``z0`` here (a flat device tensor, column by column) -- what ``differentiable_generate`` keeps for the pullback of the
    draw; nothing is appended when the caller gave ``z0``."""
    _mode_id(mode)
    n_in = icnf.nvars + n_augment_input(icnf)
    icnf.set_params(ps)
    icnf.set_cond(ys, n)
    if z0 is None and isinstance(icnf.rng, HIPRNG):
        import torch                                    # drawn on the device, before eps: the sample is a device tensor
        zb = _Buf(icnf.rng.normal(n_in * n, icnf.device), n_in, n, torch)
        if icnf.basedist is not None:
            if normals_out is not None:
                normals_out.append(zb.arr)
            zb = _Buf(base_sample(icnf, zb.arr, n), n_in, n, torch)
    else:
        drawn = z0 is None
        if drawn:
            z0 = icnf.rng.standard_normal((n, n_in)).astype(np.float32).T
        zb = _as_colmajor(z0, n_in, "z0")
        if drawn and icnf.basedist is not None:
            import torch
            raise_if_no_gpu()
            nd = torch.from_numpy(zb.arr).to(torch.device("cuda", icnf.device))
            if normals_out is not None:
                normals_out.append(nd.reshape(-1))
            zb = _Buf(base_sample(icnf, nd, n).cpu().numpy(), n_in, n, None)
    if zb.B != n:
        raise ValueError("z0 must have n columns")
    if eps is None:
        eb = draw_eps(icnf, zb, n)
    else:
        eb = _as_colmajor(eps, n_in, "eps")
    return zb, eb


def base_sample(icnf: ICNF, normals, n: int):
    """``mu + L n`` on the device (cnf_base_sample) for the ``n_in * n`` standard normals of a flat float32 CUDA tensor laid
    out column by column; returns a new tensor of the same layout (a copy for the default base)."""
    import torch
    nrm = normals.contiguous().reshape(-1)
    n_in = icnf.nvars + n_augment_input(icnf)
    if nrm.numel() != n_in * n or nrm.dtype != torch.float32 or not nrm.is_cuda:
        raise ValueError("normals must be n_in * n float32 values on the GPU")
    out = torch.empty_like(nrm)
    h = icnf.handle()
    st = C.c_void_p(torch.cuda.current_stream(nrm.device).cuda_stream)
    _lib.check(_lib.lib().cnf_base_sample(h, nrm.data_ptr(), out.data_ptr(), n, st), h)
    return out


def base_logpdf_pullback(icnf: ICNF, w):
    """``sum_b w[b] d logpdf(basedist; s_b) / d (mean, scale)`` (cnf_base_logpdf_pullback) for a ``LearnableNormal`` base, where
    ``s_b`` is the final state of the current inference record (or of the last ``loss_and_grad``), or the base draw ``z0`` of
    the current sampling record.  ``w``: ``B`` float32 values on the GPU.  Returns device tensors ``(g_mean [n_in], g_scale)``,
    ``g_scale`` shaped like the distribution's scale (``n_in``, or ``n_in x n_in`` with zeros above the diagonal)."""
    import torch
    d = learnable(icnf.basedist)
    n_in = icnf.nvars + n_augment_input(icnf)
    w = w.detach().to(torch.float32).contiguous().reshape(-1)
    if not w.is_cuda:
        raise ValueError("w must live on the GPU")
    out = torch.empty(n_in + (n_in if d.kind == 1 else n_in * n_in), dtype=torch.float32, device=w.device)
    h = icnf.handle()
    st = C.c_void_p(torch.cuda.current_stream(w.device).cuda_stream)
    _lib.check(_lib.lib().cnf_base_logpdf_pullback(h, w.data_ptr(), w.numel(), out.data_ptr(), out[n_in:].data_ptr(), st), h)
    return out[:n_in], (out[n_in:] if d.kind == 1 else out[n_in:].view(n_in, n_in))


def base_sample_pullback(icnf: ICNF, normals, g_z0):
    """The vector-Jacobian product of ``base_sample`` (cnf_base_sample_pullback) for a ``LearnableNormal`` base: ``normals`` and
    ``g_z0`` are ``n_in x n`` on the GPU (any strides); returns ``(sum_b g_z0[:, b], tril(sum_b g_z0[:, b] normals[:, b]'))``
    -- the diagonal of the latter for a ``std`` base -- as device tensors."""
    import torch
    d = learnable(icnf.basedist)
    n_in = icnf.nvars + n_augment_input(icnf)
    if normals.dim() != 2 or normals.shape[0] != n_in or tuple(g_z0.shape) != tuple(normals.shape) or not normals.is_cuda:
        raise ValueError("normals and g_z0 must be n_in x n on the GPU")
    n = int(normals.shape[1])
    nb = normals.detach().to(torch.float32).t().contiguous()          # [n][n_in]: sample b contiguous
    gb = g_z0.detach().to(device=nb.device, dtype=torch.float32).t().contiguous()
    out = torch.empty(n_in + (n_in if d.kind == 1 else n_in * n_in), dtype=torch.float32, device=nb.device)
    h = icnf.handle()
    st = C.c_void_p(torch.cuda.current_stream(nb.device).cuda_stream)
    _lib.check(_lib.lib().cnf_base_sample_pullback(h, nb.data_ptr(), gb.data_ptr(), n, out.data_ptr(), out[n_in:].data_ptr(), st), h)
    return out[:n_in], (out[n_in:] if d.kind == 1 else out[n_in:].view(n_in, n_in))


def generate_sol(icnf: ICNF, mode, prob: ODEProblem):
    """src/base_icnf.jl:202-211: rows 1..nvars of the final state."""
    fsol = base_sol(icnf, prob)
    return fsol.view()[: icnf.nvars, :]


def generate(icnf: ICNF, mode, ps, st=None, n: int = 1, *, ys=None, z0=None, eps=None, with_logp=False):
    """src/base_icnf.jl:447-455 (conditional: :457-466, ``ys`` as keyword here).  ``with_logp``: return ``(xs, logq)``, the
    samples and their log-density under the flow from the one solve (``gen_vjp.generate_record``: with ``naugmented > 0`` the
    density of the whole n_in-dimensional final state; TestMode exact, TrainMode the Hutchinson estimate for the ``eps``
    used).  Without it the call launches exactly what it always has."""
    if with_logp:
        from .gen_vjp import generate_record
        return generate_record(icnf, mode, ps, st, n, ys=ys, z0=z0, eps=eps)
    return generate_sol(icnf, mode, generate_prob(icnf, mode, ps, st, n, ys=ys, z0=z0, eps=eps))


def inference(icnf: ICNF, mode, xs, *args, eps=None, with_sums=False):
    """src/base_icnf.jl:407-415 / :417-426 (conditional: ``inference(icnf, mode, xs, ys, ps, st)``).
    ``with_sums`` (device tensors only): also return the 5 local loss sums of ``loss_sums``, computed in
    the same C call (cnf_inference_sums) -- what a rank needs before its all-reduce."""
    if with_sums and not _is_torch(xs):
        raise ValueError("with_sums needs device tensors")
    if _is_torch(xs):
        # device tensors: the whole of inference_prob -> base_sol -> inference_sol in ONE C call (cnf_inference)
        ys, ps, st = _split_cond_args(icnf, args)
        m = _mode_id(mode)
        xb = _xs_colmajor(icnf, xs)
        B = xb.B
        icnf.set_params(ps)
        icnf.set_cond(ys, B)
        if eps is not None:
            eb = _as_colmajor(eps, icnf.nvars + n_augment_input(icnf), "eps")
            if eb.B != B:
                raise ValueError("eps must have one column per sample")
        elif m == _lib.MODE_TRAIN:
            eb = draw_eps(icnf, xb, B)
        else:
            eb = None                           # TestMode: exact trace, no probes
        t = xb.torch
        # one allocation for the three outputs (logpx | regs | sums): the allocator call is the slowest line of this path
        buf = t.empty(4 * B + 8, dtype=t.float32, device=xb.arr.device)
        logpx, regs = buf[:B], buf[B:4 * B]
        opts = _solve_opts(icnf, steer_tspan(icnf, mode))
        stats = _lib.cnf_solve_stats()
        l, h = _lib.lib(), icnf.handle()
        ep = eb.ptr if eb is not None else None
        if with_sums:
            sums = buf[4 * B:4 * B + 5]
            _lib.check(l.cnf_inference_sums(h, m, xb.ptr, ep, logpx.data_ptr(), regs.data_ptr(), sums.data_ptr(), B,
                                            C.byref(opts), C.byref(stats), _stream(xb)), h)
        else:
            _lib.check(l.cnf_inference(h, m, xb.ptr, ep, logpx.data_ptr(), regs.data_ptr(), None, B,
                                       C.byref(opts), C.byref(stats), _stream(xb)), h)
        icnf.last_stats = stats.as_dict()
        r = regs.view(3, B)
        if with_sums:
            return logpx, (r[0], r[1], r[2]), sums
        return logpx, (r[0], r[1], r[2])
    prob = inference_prob(icnf, mode, xs, *args, eps=eps)
    res = inference_sol(icnf, mode, prob)
    icnf.last_stats = prob.stats
    return res


def inference_submit(icnf: ICNF, mode, xs, *args, eps=None, with_sums=False):
    """``inference`` on device tensors, submitted: the solve is enqueued and the call returns (cnf_inference_submit) --
    a loop over column blocks or mini-batches keeps the GPU going from one solve straight into the next.  Returns the
    output tensors ``(logpx, (E, n, A)[, sums])``; they are valid once ``inference_collect(icnf)`` has returned for this
    submission (oldest first; up to three outstanding per ICNF, all on one stream)."""
    if not _is_torch(xs):
        raise ValueError("inference_submit needs device tensors")
    ys, ps, st = _split_cond_args(icnf, args)
    m = _mode_id(mode)
    xb = _xs_colmajor(icnf, xs)
    B = xb.B
    l, h = _lib.lib(), icnf.handle()
    _trim_submitted(icnf)
    # Every submission runs with ITS parameters and conditioning: the upload caches make these two calls free when nothing
    # changed (the mini-batches of an epoch); when something did, the library first brings the inferences already submitted
    # to their end (cnf_set_params / cnf_set_cond settle the queue: they stay collectable) and only then changes its state.
    icnf.set_params(ps)
    icnf.set_cond(ys, B)
    if eps is not None:
        eb = _as_colmajor(eps, icnf.nvars + n_augment_input(icnf), "eps")
        if eb.B != B:
            raise ValueError("eps must have one column per sample")
    elif m == _lib.MODE_TRAIN:
        eb = draw_eps(icnf, xb, B)
    else:
        eb = None
    t = xb.torch
    buf = t.empty(4 * B + 8, dtype=t.float32, device=xb.arr.device)
    logpx, regs = buf[:B], buf[B:4 * B]
    opts = _solve_opts(icnf, steer_tspan(icnf, mode))
    sums = buf[4 * B:4 * B + 5] if with_sums else None
    _lib.check(l.cnf_inference_submit(h, m, xb.ptr, eb.ptr if eb is not None else None, logpx.data_ptr(), regs.data_ptr(),
                                      sums.data_ptr() if with_sums else None, B, C.byref(opts), _stream(xb)), h)
    # (the inputs must outlive the launch: the submission keeps them)
    icnf._submitted = getattr(icnf, "_submitted", [])
    icnf._submitted.append((xb, eb, buf))
    r = regs.view(3, B)
    return (logpx, (r[0], r[1], r[2]), sums) if with_sums else (logpx, (r[0], r[1], r[2]))


def _trim_submitted(icnf: ICNF):
    """The buffers kept alive for submitted launches follow the library's queue: a synchronous call on the handle completes
    (and drops) what was submitted before it, so entries beyond ``cnf_inference_pending`` are released oldest first."""
    sub = getattr(icnf, "_submitted", None)
    if sub:
        n = max(0, int(_lib.lib().cnf_inference_pending(icnf.handle())))
        if len(sub) > n:
            del sub[:len(sub) - n]


def inference_collect(icnf: ICNF):
    """Completes the oldest submitted inference (cnf_inference_collect); its statistics become ``icnf.last_stats``."""
    l, h = _lib.lib(), icnf.handle()
    _trim_submitted(icnf)
    stats = _lib.cnf_solve_stats()
    _lib.check(l.cnf_inference_collect(h, C.byref(stats)), h)
    if getattr(icnf, "_submitted", None):
        icnf._submitted.pop(0)
    icnf.last_stats = stats.as_dict()
    return icnf.last_stats


def loss(icnf: ICNF, mode, xs, *args, eps=None):
    """TrainMode: mean(-logpx + l1 E + l2 n + l3 A) (src/icnf.jl:481-490); otherwise
    -mean(logpx) (src/base_icnf.jl:489-497).  Single process; the sharded form is
    ``parallel.distributed_loss``."""
    if _is_torch(xs):                 # the five sums come out of the launch of the solve (cnf_inference_sums): no second kernel
        _, _, sums = inference(icnf, mode, xs, *args, eps=eps, with_sums=True)
        return loss_from_sums(icnf, mode, sums)
    logpx, (E, n, A) = inference(icnf, mode, xs, *args, eps=eps)
    sums = loss_sums(icnf, logpx, (E, n, A))
    return loss_from_sums(icnf, mode, sums)


def set_grad_ys(icnf: ICNF, with_ys):
    """The per-handle switch of the gradient w.r.t. ``ys`` (cnf_set_grad_ys), set from ``with_ys`` by every call that takes a
    gradient.  ``ValueError`` when it is asked of an unconditional model (which has no switch to set)."""
    if not icnf.cond:
        if with_ys:
            raise ValueError("with_ys: the model has no conditioning inputs")
        return
    on = bool(with_ys)
    if on != getattr(icnf, "_grad_ys_on", False):      # (off on a fresh handle: calls that never ask make no call of it)
        l, h = _lib.lib(), icnf.handle()
        _lib.check(l.cnf_set_grad_ys(h, 1 if on else 0), h)
        icnf._grad_ys_on = on


def grad_ys(icnf: ICNF, B, dev, stream, host=False):
    """d / d ys of the last gradient call (cnf_grad_ys): ``n_cond x B``, where ys lives -- a device tensor, or a numpy array
    for host inputs."""
    import torch
    l, h = _lib.lib(), icnf.handle()
    gy = torch.empty(B * icnf.n_cond, dtype=torch.float32, device=dev)
    _lib.check(l.cnf_grad_ys(h, gy.data_ptr(), B, stream), h)
    gy = gy.view(B, icnf.n_cond).t()
    return gy.cpu().numpy() if host else gy


def grad_x(icnf: ICNF, B, dev, stream, host=False):
    """d / d xs of the last gradient call (the reference's call tests differentiate the loss w.r.t. the data too:
    test/call_tests.jl, `diff2_loss`): the adjoint state at t0, left behind by the backward sweep (cnf_grad_x) -- ``nvars x B``,
    where xs lives."""
    import torch
    l, h = _lib.lib(), icnf.handle()
    gx = torch.empty(B * icnf.nvars, dtype=torch.float32, device=dev)
    _lib.check(l.cnf_grad_x(h, gx.data_ptr(), B, stream), h)
    gx = gx.view(B, icnf.nvars).t()
    return gx.cpu().numpy() if host else gx


def grad_steps(icnf: ICNF):
    """``icnf.last_steps``: the signed step sizes the last gradient or recorded solve went through (cnf_grad_steps)."""
    l, h = _lib.lib(), icnf.handle()
    n = l.cnf_grad_steps(h, None, 0)
    hs = np.empty(max(n, 1), dtype=np.float32)
    l.cnf_grad_steps(h, hs.ctypes.data, n)
    icnf.last_steps = hs[:n]


def resolve_eps(icnf: ICNF, m, eps, xb: _Buf, B):
    """The probes of a gradient or recording call in mode ``m``: none in TestMode, the caller's (one column per sample), or
    drawn as ``inference`` draws them."""
    if m != _lib.MODE_TRAIN:
        return None
    if eps is None:
        return draw_eps(icnf, xb, B)
    eb = _as_colmajor(eps, icnf.nvars + n_augment_input(icnf), "eps")
    if eb.B != B:
        raise ValueError("eps must have one column per sample")
    return eb


def to_device(icnf: ICNF, a, dev=None):
    """A host array as a float32 tensor on ``dev`` (the model's device); a host ``_Buf`` as a device ``_Buf`` over the same
    column-major storage.  None and what is on a device already pass through."""
    import torch
    if a is None or (isinstance(a, _Buf) and a.torch is not None):
        return a
    if isinstance(a, _Buf):
        return _Buf(to_device(icnf, a.arr, dev), a.rows, a.B, torch)
    raise_if_no_gpu()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(dev or torch.device("cuda", icnf.device))


def device_and_stream(icnf: ICNF, buf: _Buf):
    """Where the device side of a call on ``buf`` runs: the tensor's device (the model's for host arrays) and its current stream."""
    import torch
    dev = buf.arr.device if buf.torch is not None else torch.device("cuda", icnf.device)
    return dev, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def grad_result(head, host, *optional):
    """The result of a gradient call: ``head`` and then those of the optional results that were asked for -- ``(asked, value)``
    in their one order: d / d xs (or z0), d / d ys, the base's pair -- as numpy arrays for a call on host arrays.  A lone
    gradient is returned bare."""
    def where(v):
        if isinstance(v, tuple):
            return tuple(where(a) for a in v)
        return v.cpu().numpy() if host and _is_torch(v) else v
    out = tuple(where(v) for v in head) + tuple(where(v) for asked, v in optional if asked)
    return out[0] if len(out) == 1 else out


def loss_and_grad(icnf: ICNF, mode, xs, *args, eps=None, with_x=False, with_ys=False, with_base=False):
    """``(loss, d loss / d ps)``: the pair ``MLJModelInterface.fit`` gets from Enzyme on
    ``loss(icnf, TrainMode(), xs, ps, st)`` (src/exts/mlj_ext/core_icnf.jl:59-73, src/icnf.jl:481-490),
    here from the discrete adjoint of the solve (cnf_loss_grad).  The gradient has the layout of
    ``ps`` and lives where ``xs`` lives (torch.cuda tensor or numpy array).  Conditional models:
    ``(xs, ys, ps, st)`` as everywhere else.  Steering draws t1 exactly as ``loss`` does.  ``with_x`` / ``with_ys`` append
    d loss / d xs (``nvars x B``) and, for a conditional model, d loss / d ys (``n_cond x B``) to the result; with
    ``with_ys`` the gradient always takes the recorded solve.  ``with_base`` (a ``LearnableNormal`` base, device tensors)
    appends ``(d loss / d mean, d loss / d scale)`` last: the log-density of the final state pulled back with the loss's
    cotangent ``-1/B`` (cnf_base_logpdf_pullback); ``ValueError`` with any other base.

    TestMode: ``loss(icnf, TestMode(), xs, ps, st)`` and its gradient through the exact-trace solve (cnf_loss_grad_test): what the
    reference's call tests and benchmark suite differentiate besides the TrainMode loss (test/call_tests.jl ``diff_loss``,
    benchmark/benchmarks.jl:60-99).  Small two-layer (or one-layer) tanh networks in the launch of the solve; every other Dense
    chain through the recorded solve and the generic adjoint kernel (cnf_gradt.hip); ``NotImplementedError`` only where that
    kernel's LDS budget is exceeded."""
    if with_base:
        learnable(icnf.basedist)
        if not _is_torch(xs):
            raise ValueError("with_base needs device tensors")
    m = _mode_id(mode)
    ys, ps, st = _split_cond_args(icnf, args)
    xb = _xs_colmajor(icnf, xs)
    B = xb.B
    icnf.set_params(ps)
    icnf.set_cond(ys, B)
    set_grad_ys(icnf, with_ys)
    eb = resolve_eps(icnf, m, eps, xb, B)
    opts = _solve_opts(icnf, steer_tspan(icnf, mode))
    stats = _lib.cnf_solve_stats()
    val = C.c_float()
    l, h = _lib.lib(), icnf.handle()
    host = xb.torch is None                                # host arrays in, host gradient out
    dev, stream = device_and_stream(icnf, xb)
    # the two modes differ in the pair of entry points (TrainMode's take eps) ...
    if m == _lib.MODE_TRAIN:
        fn, lead = (l.cnf_loss_grad_host if host else l.cnf_loss_grad), (h, xb.ptr, eb.ptr, B)
    else:
        fn, lead = (l.cnf_loss_grad_test_host if host else l.cnf_loss_grad_test), (h, xb.ptr, B)
    if host:
        grad = np.empty(icnf.nn.n_params_internal, dtype=np.float32)
        rc = fn(*lead, C.byref(opts), C.byref(val), grad.ctypes.data, C.byref(stats))
    else:
        grad = xb.torch.empty(icnf.nn.n_params_internal, dtype=xb.torch.float32, device=dev)
        rc = fn(*lead, C.byref(opts), C.byref(val), grad.data_ptr(), C.byref(stats), stream)
    # ... and in that TestMode has networks without a gradient
    if m != _lib.MODE_TRAIN and rc == _lib.ERR_UNSUPPORTED:
        raise NotImplementedError("TestMode gradient: network too wide for the adjoint kernels: " + l.cnf_last_error(h).decode())
    _lib.check(rc, h)
    icnf.last_stats = stats.as_dict()
    grad_steps(icnf)                     # signed step sizes the gradient was taken through
    grad = icnf.nn.grad_to_external(grad)  # (PlanarLayer: back to the (u, w, b) order; identity for Dense chains)
    return grad_result((float(val.value), grad), host,
                       (with_x, grad_x(icnf, B, dev, stream, host) if with_x else None),
                       (with_ys, grad_ys(icnf, B, dev, stream, host) if with_ys else None),
                       (with_base, _loss_base_grad(icnf, xs) if with_base else None))


def _loss_base_grad(icnf: ICNF, xs):
    """(d loss / d mean, d loss / d scale) of the ``loss_and_grad`` call that has just returned: the loss is ``-mean(logpx)``
    plus terms that do not depend on the base, so every sample carries ``-1/B``."""
    import torch
    B = xs.shape[1]
    return base_logpdf_pullback(icnf, torch.full((B,), -1.0 / B, dtype=torch.float32, device=xs.device))


def loss_and_grad_submit(icnf: ICNF, mode, xs, *args, eps=None):
    """``loss_and_grad`` on device tensors, SUBMITTED (cnf_loss_grad_submit): solve, loss, adjoint and the sum of the partials are
    enqueued and the call returns ``(loss, grad)`` as device tensors (one float; ``n_params`` floats) that are valid in stream
    order -- an optimiser update enqueued next on the same stream consumes the gradient without the host ever waiting.
    ``loss_and_grad_collect(icnf)`` completes the oldest submission (at most three in flight).  ``ps`` must be a device tensor;
    it is uploaded with ``set_params_async``.  ``NotImplementedError`` where the gradient does not run in the launch of the
    solve, or the model has a non-default ``basedist`` (use ``loss_and_grad``)."""
    import torch
    if not _is_torch(xs):
        raise ValueError("loss_and_grad_submit needs device tensors")
    if icnf.basedist is not None:       # (refused before anything is drawn or uploaded, as cnf_loss_grad_submit itself would)
        raise NotImplementedError("no in-launch gradient with a non-default basedist: use loss_and_grad")
    ys, ps, st = _split_cond_args(icnf, args)
    m = _mode_id(mode)
    xb = _xs_colmajor(icnf, xs)
    B = xb.B
    _trim_submitted(icnf)
    icnf.set_params_async(ps)
    icnf.set_cond(ys, B)
    set_grad_ys(icnf, False)            # (a submitted gradient carries no d / d ys: the switch would refuse it)
    eb = resolve_eps(icnf, m, eps, xb, B)
    opts = _solve_opts(icnf, steer_tspan(icnf, mode))
    l, h = _lib.lib(), icnf.handle()
    out = torch.empty(icnf.nn.n_params_internal + 1, dtype=torch.float32, device=xb.arr.device)
    grad, lossd = out[:-1], out[-1:]
    rc = l.cnf_loss_grad_submit(h, m, xb.ptr, eb.ptr if eb is not None else None, B, C.byref(opts), lossd.data_ptr(), grad.data_ptr(),
                                _stream(xb))
    if rc == _lib.ERR_UNSUPPORTED:
        raise NotImplementedError("no in-launch gradient for this network / batch: use loss_and_grad")
    _lib.check(rc, h)
    icnf._submitted = getattr(icnf, "_submitted", [])
    icnf._submitted.append((xb, eb, out))
    return lossd, icnf.nn.grad_to_external(grad)


def loss_and_grad_collect(icnf: ICNF):
    """Completes the oldest submitted gradient (cnf_loss_grad_collect); returns its statistics.  Raises ``RuntimeError`` if that
    launch gave up (it delivered zeros and a NaN loss): run the batch again with ``loss_and_grad``."""
    return inference_collect(icnf)


def loss_sums(icnf: ICNF, logpx, regs):
    """(sum logpx, sum E, sum n, sum A, B) -- the only cross-shard quantity.  Device
    inputs are reduced on the device (cnf_loss_sums) and stay there."""
    E, n, A = regs
    if _is_torch(logpx):
        import torch
        B = logpx.numel()
        if (E.data_ptr() + 4 * B == n.data_ptr() and n.data_ptr() + 4 * B == A.data_ptr()
                and E.is_contiguous() and n.is_contiguous() and A.is_contiguous()):
            r = E                  # the three rows are already one 3 x B buffer (as _post returns them)
        else:
            r = torch.stack([E, n, A]).contiguous().reshape(-1)
        out = torch.empty(5, dtype=torch.float32, device=logpx.device)
        st = C.c_void_p(torch.cuda.current_stream(logpx.device).cuda_stream)
        _lib.check(_lib.lib().cnf_loss_sums(icnf.handle(), logpx.contiguous().data_ptr(), r.data_ptr(), B,
                                            out.data_ptr(), st), icnf.handle())
        return out
    return np.array([np.sum(logpx, dtype=np.float64), np.sum(E, dtype=np.float64),
                     np.sum(n, dtype=np.float64), np.sum(A, dtype=np.float64), len(logpx)], dtype=np.float32)


def loss_from_sums(icnf: ICNF, mode, sums) -> float:
    s = sums.detach().cpu().numpy() if _is_torch(sums) else np.asarray(sums)
    s = np.ascontiguousarray(s, dtype=np.float32)
    out = C.c_float()
    _lib.check(_lib.lib().cnf_loss_from_sums(icnf.handle(), _mode_id(mode), s.ctypes.data, C.byref(out)),
               icnf.handle())
    return float(out.value)
