"""Ensembles: M independent models of one architecture -- cross-validation folds, bootstrap replicas, seeds, sweeps -- whose
losses and gradients come out of ONE launch (cnf_loss_grad_many, include/cnfhip_ensemble.h).  The reference trains its README /
regression networks at ``batch_size = 32`` (src/exts/mlj_ext/core_icnf.jl:59-73); a gradient of one such model occupies two
workgroups of the device; here M of them run side by side on M times as many (measured: tools/prof_ensemble.py).

``loss_and_grad_many`` is ``loss_and_grad`` for M members with their own parameters, data, probes and end times;
``fit_many`` is ``mlj.fit`` for M data sets trained side by side.

The other half of that workflow (include/cnfhip_ensemble_eval.h): ``inference_many`` / ``loss_many`` score the M members --
each on its own held-out data, or all on one data set -- and ``generate_many`` samples them, each in ONE launch of the plain
ensemble form of the same kernel; ``EnsembleDist`` is the bagged density: a weighted mixture of the members with ``logpdf``,
``pdf`` and ``rand``."""
from __future__ import annotations

import ctypes as C
import functools
import time
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np

from . import _lib
from .base_icnf import ICNF, _Buf, _is_torch, _mode_id, _solve_opts, _stream, draw_eps, generate, inference, loss_and_grad, \
    n_augment_input, steer_tspan
from .distributions import LearnableNormal
from .ensemble_base import EnsembleBases
from .gen_vjp import _cot_two
from .layers import setup
from .rng import HIPRNG
from .types import TrainMode
from .vjp import _cot_rows


def _refusal(icnf: ICNF):
    """Why this model has no ensemble form, or None.  Host logic only: nothing is drawn, no handle is made.  The network
    envelope restates `ens_fn` of csrc/cnf_wave.hip and the WF_ENS_GRAD form of csrc/cnf_wave_variants.h (which decide for the
    C ABI): change both together."""
    if icnf.cond:
        return "conditional models are evaluated one member at a time"
    if icnf.basedist is not None:
        return "a non-default basedist is evaluated one member at a time"
    if icnf.compute_mode.kernel == "generic":
        return "the ensemble form exists on the wave kernels only (kernel = 'generic' was asked for)"
    if icnf.nn.planar is not None:
        return "PlanarLayer chains keep (u, w, b) vectors: one member at a time"
    dims, acts = icnf.nn.dims, icnf.nn.acts
    tanh, ident = _lib.ACT["tanh"], _lib.ACT["identity"]
    if len(acts) != 2 or acts[0] != tanh or acts[1] not in (tanh, ident) or dims[0] > 16 or dims[1] > 64 or \
            (acts[1] == ident and dims[1] > 16):
        return (f"no ensemble form for the network {dims}: two layers, tanh then tanh (or identity, up to 16 hidden units), "
                "n_in <= 16 and at most 64 hidden units")
    return None


def _capacity(icnf: ICNF, mode, capacity_fn, *size) -> int:
    """What ``capacity_fn`` of the C ABI answers for this model, mode and size; 0, without making a handle, for a model
    ``_refusal`` turns away."""
    m = _mode_id(mode)
    if _refusal(icnf) is not None:
        return 0
    return int(getattr(_lib.lib(), capacity_fn)(icnf.handle(), m, *(int(s) for s in size)))


def ensemble_capacity(icnf: ICNF, mode, B: int) -> int:
    """The largest M one launch takes for this model, mode and batch size (cnf_ensemble_capacity); 0: no ensemble form."""
    return _capacity(icnf, mode, "cnf_ensemble_capacity", B)


def _check_inputs(icnf: ICNF, mode, xs, ps, eps, t1, who="loss_and_grad_many", single="loss_and_grad"):
    m = _mode_id(mode)
    why = _refusal(icnf)
    if why is not None:
        raise NotImplementedError(f"{who}: " + why)
    if not (_is_torch(xs) and _is_torch(ps)):
        raise NotImplementedError(f"{who} takes device tensors (host arrays: {single}, one member at a time)")
    if xs.dim() != 3 or xs.shape[1] != icnf.nvars or xs.shape[0] < 1 or xs.shape[2] < 1:
        raise ValueError(f"xs must be (M, nvars = {icnf.nvars}, B), got {tuple(xs.shape)}")
    M, _, B = xs.shape
    n_params = icnf.nn.n_params_internal
    if ps.dim() != 2 or tuple(ps.shape) != (M, n_params):
        raise ValueError(f"ps must be (M = {M}, n_params = {n_params}), got {tuple(ps.shape)}")
    n_in = icnf.nvars + n_augment_input(icnf)
    if eps is not None:
        if m != _lib.MODE_TRAIN:
            raise ValueError("eps has no meaning in TestMode (exact trace)")
        if not _is_torch(eps) or tuple(eps.shape) != (M, n_in, B):
            raise ValueError(f"eps must be a device tensor (M = {M}, n_in = {n_in}, B = {B})")
    if t1 is not None:
        t1 = np.asarray(t1, dtype=np.float32).reshape(-1)
        if t1.shape[0] != M:
            raise ValueError(f"t1 must have one end time per member (M = {M}), got {t1.shape[0]}")
        if not np.isfinite(t1).all() or (t1 == np.float32(icnf.tspan[0])).any():
            raise ValueError("t1: every member needs a finite end time different from tspan[0]")
    return m, M, B, n_in, t1


def _probes_and_ends(icnf: ICNF, mode, train, M, B, n_in, xr, eps, t1, steer=True, counts=None):
    """The members' probes ([M][B][n_in] on the device of ``xr``; None in TestMode) and end times (None: ``tspan[1]`` for all),
    given or drawn in the order ``loss_and_grad_many`` documents.  ``steer=False``: no steer variate is drawn (the path calls,
    which are this draw with one member).  ``counts``: on a host generator member m draws ``counts[m]`` columns -- what a loop of
    the single-model call at that batch size draws -- and the columns behind them are zeros."""
    import torch
    steer = steer and train and t1 is None and icnf.STEER      # (given end times and TestMode never steer)
    if not train:
        er = None
    elif eps is not None:
        er = _rows(eps)
    elif isinstance(icnf.rng, HIPRNG):                     # one draw of M B columns
        er = draw_eps(icnf, _Buf(xr.view(-1), icnf.nvars, M * B, torch), M * B).arr.view(M, B, n_in)
    else:
        # the host generator, member by member in the order a loop of ``loss_and_grad`` consumes it (the member's probes, then
        # its end time: base_icnf.loss_and_grad), so that one seed gives the members the draws that loop would; one upload
        host, draws, ends = _Buf(None, icnf.nvars, B, None), [], []
        for i in range(M):
            if counts is None:
                draws.append(draw_eps(icnf, host, B).arr.reshape(B, n_in))
            else:
                k = int(counts[i])
                draws.append(np.zeros((B, n_in), dtype=np.float32))
                draws[-1][:k] = draw_eps(icnf, _Buf(None, icnf.nvars, k, None), k).arr.reshape(k, n_in)
            if steer:
                ends.append(steer_tspan(icnf, mode)[1])
        er = torch.from_numpy(np.stack(draws)).to(xr.device)
        if steer:
            t1 = np.asarray(ends, dtype=np.float32)
    if steer and t1 is None:                               # (given probes, or a device generator: M draws)
        t1 = np.asarray([steer_tspan(icnf, mode)[1] for _ in range(M)], dtype=np.float32)
    return er, t1


def _rows(x):
    """(M, rows, B) -> the bytes the C ABI reads: [M][B][rows]."""
    import torch
    return x.detach().to(torch.float32).permute(0, 2, 1).contiguous()


# ---- heterogeneous members (include/cnfhip_ensemble_hetero.h): per-member batch size, lambdas and tolerances ----
def _default_tols(icnf: ICNF):
    """(abstol, reltol) of the model's ``sol_kwargs`` (OrdinaryDiffEq's defaults where it has none: ``_solve_opts_build``)."""
    return float(icnf.sol_kwargs.get("abstol", 1e-6)), float(icnf.sol_kwargs.get("reltol", 1e-3))


def _members(icnf: ICNF, M, B, counts=None, lambdas=None, reltol=None, abstol=None, who="loss_and_grad_many"):
    """The per-member arguments of an ensemble call, checked.  Host logic only: nothing is drawn, no handle is made.  ``counts``:
    M batch sizes within [1, B]; ``lambdas``: (M, 3) finite values, zero exactly where the model's are (that decides the rows of
    the state); ``reltol`` / ``abstol``: a positive finite scalar or M of them (one given: the other is the model's).  Returns
    None when none is given (the call is then today's), else a namespace ``counts`` (int32 (M,) or None), ``lambdas`` (float32
    (M, 3) or None), ``tols`` (float32 (M, 2): abstol, reltol; or None)."""
    if counts is None and lambdas is None and reltol is None and abstol is None:
        return None
    c = lam = tols = None
    if counts is not None:
        c = np.asarray(counts)
        if c.ndim != 1 or c.shape[0] != M or not np.issubdtype(c.dtype, np.integer):
            raise ValueError(f"{who}: counts must be M = {M} integers, got {np.asarray(counts).shape}")
        if (c < 1).any() or (c > B).any():
            raise ValueError(f"{who}: every count must be within [1, B = {B}], got {c.tolist()}")
        c = np.ascontiguousarray(c, dtype=np.int32)
    if lambdas is not None:
        lam = np.asarray(lambdas, dtype=np.float32)
        if lam.shape != (M, 3):
            raise ValueError(f"{who}: lambdas must be (M = {M}, 3), got {lam.shape}")
        own = np.asarray([icnf.lambda1, icnf.lambda2, icnf.lambda3], dtype=np.float32)
        if not np.isfinite(lam).all() or ((lam == 0) != (own == 0)[None, :]).any():
            raise ValueError(f"{who}: every lambda must be finite, and zero exactly where the model's is (they decide the rows of "
                             f"the state): the model has {own.tolist()}")
        lam = np.ascontiguousarray(lam)
    if reltol is not None or abstol is not None:
        a0, r0 = _default_tols(icnf)
        cols = []
        for name, v, dflt in (("abstol", abstol, a0), ("reltol", reltol, r0)):
            v = np.asarray(dflt if v is None else v, dtype=np.float32)
            if v.ndim == 0:
                v = np.full(M, v, dtype=np.float32)
            if v.shape != (M,):
                raise ValueError(f"{who}: {name} must be a scalar or M = {M} values, got {v.shape}")
            if not np.isfinite(v).all() or (v <= 0).any():
                raise ValueError(f"{who}: every {name} must be finite and positive")
            cols.append(v)
        tols = np.ascontiguousarray(np.stack(cols, axis=1), dtype=np.float32)
    return SimpleNamespace(counts=c, lambdas=lam, tols=tols)


@functools.lru_cache(maxsize=64)
def _call_values(M, B, lams, tols):
    """(counts, lambdas, tols) of a call whose members are all the call's own: read-only arrays, made once per shape."""
    out = (np.full(M, B, dtype=np.int32), np.tile(np.asarray(lams, dtype=np.float32), (M, 1)), np.tile(np.asarray(tols, dtype=np.float32), (M, 1)))
    for a in out:
        a.flags.writeable = False
    return out


def _members_used(icnf: ICNF, het, M, B):
    """What a call reports as ``info["counts"]``, ``info["lambdas"]`` and ``info["tols"]``: the members' own, or the call's."""
    c, lam, tols = _call_values(int(M), int(B), (icnf.lambda1, icnf.lambda2, icnf.lambda3), _default_tols(icnf))
    if het is None:
        return dict(counts=c, lambdas=lam, tols=tols)
    return dict(counts=het.counts.copy() if het.counts is not None else c, lambdas=het.lambdas.copy() if het.lambdas is not None else lam,
                tols=het.tols.copy() if het.tols is not None else tols)


def _set_members(h, het, lo, n):
    """cnf_ensemble_set_members for the members ``lo .. lo + n - 1``: the next ensemble call on the handle takes them away."""
    part = [a[lo:lo + n] if a is not None else None for a in (het.counts, het.lambdas, het.tols)]
    _lib.check(_lib.lib().cnf_ensemble_set_members(
        h, n, part[0].ctypes.data_as(C.POINTER(C.c_int)) if part[0] is not None else None,
        part[1].ctypes.data if part[1] is not None else None, part[2].ctypes.data if part[2] is not None else None), h)


# ---- a base per member (include/cnfhip_ensemble_base.h) ----
def _check_bases(icnf: ICNF, bases, M, who):
    """``bases=`` of an ensemble call, checked.  Host logic only: nothing is drawn, no handle is made."""
    if bases is None:
        return None
    if not isinstance(bases, EnsembleBases):
        raise ValueError(f"{who}: bases must be an EnsembleBases, got {type(bases).__name__}")
    n_in = icnf.nvars + n_augment_input(icnf)
    if len(bases) != M or bases.n_in != n_in:
        raise ValueError(f"{who}: bases must have M = {M} members of nvars + naugmented = {n_in} rows, got ({len(bases)}, {bases.n_in})")
    return bases


def _bases_on(bases, dev):
    """The members' bases as the device reads them: a namespace ``src`` (the ``EnsembleBases``), ``kind``, ``mean`` (M, n_in) and
    ``scale`` -- detached float32 tensors on ``dev`` holding the current values; None for None."""
    if bases is None:
        return None
    mean, scale = bases.device_values(dev)
    return SimpleNamespace(src=bases, kind=bases.kind, mean=mean, scale=scale)


def _set_bases(h, b, lo, n, stream):
    """cnf_ensemble_set_bases for the members ``lo .. lo + n - 1`` (stream-ordered: one small kernel, no host wait): the next
    ensemble call on the handle takes them away."""
    _lib.check(_lib.lib().cnf_ensemble_set_bases(h, n, b.kind, b.mean[lo].data_ptr(), b.scale[lo].data_ptr(), stream), h)


def _base_grads(b, M, dev):
    """Where the base pullbacks leave ``(g_mean (M, n_in), g_scale)``: zeros, so that a member that contributes nothing has none."""
    import torch
    return torch.zeros(tuple(b.mean.shape), dtype=torch.float32, device=dev), torch.zeros(tuple(b.scale.shape), dtype=torch.float32, device=dev)


def _logpdf_pullback(h, b, lo, n, w, B, out, stream):
    """cnf_ensemble_base_logpdf_pullback of the ensemble call just made for the members ``lo .. lo + n - 1``: ``w`` (n, B)
    weights of the log-density of each column that call left in the column store; into ``out = (g_mean, g_scale)``."""
    w = w.contiguous()
    _lib.check(_lib.lib().cnf_ensemble_base_logpdf_pullback(h, n, w.data_ptr(), B, out[0][lo].data_ptr(), out[1][lo].data_ptr(), stream), h)


def _member_base(b, i, learn=False):
    """Member i's base as a single model's ``basedist``: the constant ``bases[i]``, or -- ``learn`` -- a ``LearnableNormal`` over
    its current values, which the single-model calls return the base's gradient for."""
    if not learn:
        return b.src[i]
    return LearnableNormal(b.mean[i].clone(), **{"std" if b.kind == 1 else "scale_tril": b.scale[i].clone()})


def member_twin(icnf: ICNF, lambdas=None, tols=None, basedist=None):
    """A model of its own handle that is ``icnf`` with one member's regularisers (``lambdas``: three values) and tolerances
    (``tols``: abstol, reltol) -- what the member of a heterogeneous call is compared with and, when its part of a launch gave
    up, run again on.  It shares ``icnf``'s generator and network; the caller closes it."""
    import dataclasses
    kw = dict(icnf.sol_kwargs)
    if tols is not None:
        kw["abstol"], kw["reltol"] = float(np.float32(tols[0])), float(np.float32(tols[1]))
    lam = (icnf.lambda1, icnf.lambda2, icnf.lambda3) if lambdas is None else tuple(float(np.float32(v)) for v in lambdas)
    return dataclasses.replace(icnf, sol_kwargs=kw, lambda1=lam[0], lambda2=lam[1], lambda3=lam[2], _handle=None, _cond_id=None,
                               _params_id=None, _base_id=None, basedist=basedist if basedist is not None else icnf.basedist)


def pad_columns(parts, B, fill=0.0):
    """Ragged members -> one rectangular array: ``parts[m]`` is (rows, counts[m]); the result is (M, rows, B) with ``fill`` in
    the columns at and behind a member's count (numpy arrays or torch tensors; the result is of the same kind)."""
    if _is_torch(parts[0]):
        import torch
        out = torch.full((len(parts), parts[0].shape[0], B), fill, dtype=parts[0].dtype, device=parts[0].device)
    else:
        out = np.full((len(parts), parts[0].shape[0], B), fill, dtype=parts[0].dtype)
    for m, p in enumerate(parts):
        if p.shape[1] > B:
            raise ValueError(f"member {m} has {p.shape[1]} columns, more than B = {B}")
        out[m, :, :p.shape[1]] = p
    return out


def member_loss_from_sums(mode, sums5, lambdas):
    """A member's loss from its five sums (logpx, E, n, A, count) with its own regularisers: ``(-S_logpx + l1 S_E + l2 S_n + l3
    S_A) / count`` in TrainMode (src/icnf.jl:489), ``-S_logpx / count`` in TestMode (src/base_icnf.jl:496), formed in float64 and
    rounded once -- the arithmetic of the library's per-member loss; ``inference_many`` forms the loss of a member that was run
    again with it."""
    s = np.asarray(sums5.detach().cpu() if _is_torch(sums5) else sums5, dtype=np.float32).astype(np.float64)
    lam = np.asarray(lambdas, dtype=np.float32).astype(np.float64)
    if not s[4] > 0:
        raise ValueError("empty batch")
    if _mode_id(mode) == _lib.MODE_TRAIN:
        return np.float32((-s[0] + lam[0] * s[1] + lam[1] * s[2] + lam[2] * s[3]) / s[4])
    return np.float32(-s[0] / s[4])


_BASE_CAPACITY = {"cnf_ensemble_capacity": 0, "cnf_ensemble_vjp_capacity": 1}     # -> cnf_ensemble_base_capacity's `per_sample`


def _device_capacity(who, capacity_fn, h, m, B, *more):
    """The members one launch takes on this device (``capacity_fn`` of the C ABI), or ``NotImplementedError``."""
    cap = int(getattr(_lib.lib(), capacity_fn)(h, m, B, *more))
    if cap < 1:
        raise NotImplementedError(f"{who}: no ensemble form for this model, mode or batch on this device ({capacity_fn} is 0)")
    return cap


def _settle_density(icnf: ICNF, mode, xs, ps, eps, t1, who, single, capacity_fn=None, cot_rows=None, shared=True, members=None,
                    steer=True, bases=None):
    """The inputs of a density-direction ensemble call, checked, placed and drawn, in the one order the callers promise: the
    host-side refusals and shape checks (``_check_inputs``, then ``cot_rows(M, B)``: the call's cotangent tensors) -- nothing is
    drawn, no handle is made --; the handle (no device: cnf_create's error, as everywhere); the device check; the capacity
    (``capacity_fn`` of the C ABI; None: not asked, for the ``differentiable_*`` entries, whose forward asks); the probes and
    end times (``_probes_and_ends``).  ``shared``: ``xs`` may be one (nvars, B) data set for all members.  ``members``: the
    keywords ``counts``, ``lambdas``, ``reltol``, ``abstol`` of the call (``_members`` checks them with the shapes).
    ``steer=False``: no steer variate is drawn (the path calls).  Returns a
    namespace: ``m, M, B, n_in, train, cot, cap, dev, stream, xr, pr, er, t1, het``."""
    import torch
    if shared and _is_torch(xs) and _is_torch(ps) and xs.dim() == 2 and ps.dim() == 2 and _refusal(icnf) is None:
        xs = xs.unsqueeze(0).expand(ps.shape[0], *xs.shape)                # shared data: every member reads its own copy
    m, M, B, n_in, t1 = _check_inputs(icnf, mode, xs, ps, eps, t1, who, single)
    cot = cot_rows(M, B) if cot_rows is not None else ()
    het = _members(icnf, M, B, who=who, **members) if members else None
    bases = _check_bases(icnf, bases, M, who)
    h = icnf.handle() if capacity_fn is not None else None
    if not (xs.is_cuda and ps.is_cuda and all(a is None or a.is_cuda for a in (eps, *cot))):
        raise ValueError(f"{who}: torch tensors must live on the GPU")
    cap = _device_capacity(who, capacity_fn, h, m, B) if capacity_fn is not None else None
    if cap is not None and bases is not None and capacity_fn in _BASE_CAPACITY:      # (the gradient launch with bases: kernels of its own)
        cap = min(cap, _device_capacity(who, "cnf_ensemble_base_capacity", h, m, B, _BASE_CAPACITY[capacity_fn]))
    train, dev = m == _lib.MODE_TRAIN, xs.device
    xr = _rows(xs)
    pr = ps.detach().to(torch.float32).contiguous()
    er, t1 = _probes_and_ends(icnf, mode, train, M, B, n_in, xr, eps, t1, steer=steer, counts=het.counts if het is not None else None)
    return SimpleNamespace(m=m, M=M, B=B, n_in=n_in, train=train, cot=cot, cap=cap, dev=dev, xr=xr, pr=pr, er=er, t1=t1, het=het,
                           stream=_stream(_Buf(xr, icnf.nvars, M * B, torch)), bases=_bases_on(bases, dev))


def _launch(icnf: ICNF, s, width, call, steps_of, times_key, times, **more):
    """The first half of every ensemble call: the ABI call in launches of at most ``s.cap`` members (``s.M`` above the
    capacity: consecutive launches), and what every ensemble call reports.  ``call(lo, n, status, stats)`` makes the ABI call
    for the members ``lo .. lo + n - 1`` with the two pointers as its ``status_out`` and ``stats_out``; ``steps_of(icnf, i)``
    reads the steps of member i of the call just made (asked for the members that succeeded; None: no steps); ``times``: the
    members' own times (None: ``tspan[1]`` for all), reported as ``info[times_key]``; ``width``: the columns of the call's rectangle.  Returns ``(info, steps)``; failures are
    ``_finish``'s, so that a caller may publish ``info`` before they are raised."""
    h, M, het, bases = icnf.handle(), s.M, getattr(s, "het", None), getattr(s, "bases", None)
    after = more.pop("after", None)                        # after(lo, n): behind the ABI call for those members (the base pullbacks)
    status = np.empty(M, dtype=np.int32)
    stats = (_lib.cnf_solve_stats * M)()
    calls, steps = 0, [] if steps_of is not None else None
    for lo in range(0, M, s.cap):
        n = min(s.cap, M - lo)
        if het is not None:                                # (a split slices the members' arrays with the members)
            _set_members(h, het, lo, n)
        if bases is not None:                              # (... and the members' bases: one stream-ordered kernel, no host wait)
            _set_bases(h, bases, lo, n, s.stream)
            if getattr(s, "normals", None) is not None:    # a drawn z0: mu_m + L_m n with the bases just prepared (they stay pending)
                _lib.check(_lib.lib().cnf_ensemble_base_sample(h, n, s.normals[lo].data_ptr(), s.zr[lo].data_ptr(), s.n, s.stream), h)
        _lib.check(call(lo, n, status[lo:].ctypes.data, C.byref(stats, lo * C.sizeof(_lib.cnf_solve_stats))), h)
        calls += 1
        if after is not None:
            after(lo, n)
        if steps_of is not None:
            steps += [steps_of(icnf, i) if status[lo + i] == _lib.OK else None for i in range(n)]
    if times is None:
        times = np.full(M, icnf.tspan[1], dtype=np.float32)
    info = {"stats": [st.as_dict() for st in stats], "status": status, "launches": max(st.launches for st in stats),
            "calls": calls, "rerun": [], times_key: times, **_members_used(icnf, het, M, width), **more}
    return info, steps


def _finish(icnf: ICNF, info, steps, times, rerun, het=None, bases=None, learn=False):
    """The second half: a member that failed raises; the members whose part of the launch gave up are run again one at a
    time.  ``rerun(i, model, k)`` runs member i on the single-model route of ``model`` -- ``icnf``, or the twin that carries the
    member's own lambdas and tolerances -- at its ``k`` columns, writes its outputs and returns ``(stats, steps)`` as that
    route reports them (None for what it does not report).  Fills ``info["rerun"]`` and, when steps were asked for,
    ``info["steps"]``."""
    status = info["status"]
    _raise_failed(status)
    gave_up = [i for i in range(len(status)) if status[i] != _lib.OK]
    if gave_up:
        with _one_member_at_a_time(icnf, times, het, bases, learn) as member:
            for i in gave_up:
                stats_i, steps_i = rerun(i, member(i), int(info["counts"][i]))
                status[i] = _lib.OK
                if stats_i is not None:
                    info["stats"][i] = stats_i
                if steps is not None:
                    steps[i] = steps_i
        info["rerun"] = gave_up
    if steps is not None:
        info["steps"] = steps


def _raise_failed(status):
    l = _lib.lib()
    for i, s in enumerate(status):
        if s in (_lib.ERR_NONFINITE, _lib.ERR_MAXITERS):
            raise _lib.CNFError(int(s), f"ensemble member {i}: " + l.cnf_status_string(int(s)).decode())
        if s == _lib.ERR_BAD_ARG:                          # (what the device found in values the host could not look at)
            raise _lib.CNFError(int(s), f"ensemble member {i}: its base is not a Gaussian (a non-finite entry, or a scale whose "
                                        "diagonal is not positive)")


@contextmanager
def _one_member_at_a_time(icnf: ICNF, times, het=None, bases=None, learn=False):
    """For the re-run of the members whose part of the launch gave up -- the existing route, its fallbacks included: ``tspan``
    and ``steer_rate`` are set aside and restored; ``member(i)`` of the yielded function puts member i's own time in and returns
    the model to run it on: ``icnf`` itself, or -- members with their own lambdas or tolerances -- a ``member_twin`` that carries
    them (closed when the next one is asked for, and at the end)."""
    span, steer = icnf.tspan, icnf.steer_rate
    hown = het is not None and (het.lambdas is not None or het.tols is not None)
    own = hown or bases is not None                        # (a member's base is its twin's ``basedist``: the single-model route takes one)
    twin = []

    def member(i):
        if times is not None:
            icnf.tspan = (span[0], float(times[i]))
        if not own:
            return icnf
        while twin:
            twin.pop().close()
        twin.append(member_twin(icnf, het.lambdas[i] if hown and het.lambdas is not None else None,
                                het.tols[i] if hown and het.tols is not None else None,
                                _member_base(bases, i, learn) if bases is not None else None))
        return twin[0]                                     # (made behind the assignments above: it has the member's span, no steering)
    try:
        icnf.steer_rate = 0.0
        yield member
    finally:
        icnf.tspan, icnf.steer_rate = span, steer
        while twin:
            twin.pop().close()


def loss_and_grad_many(icnf: ICNF, mode, xs, ps, st=None, eps=None, t1=None, with_steps=False, counts=None, lambdas=None,
                       reltol=None, abstol=None, bases=None, with_base=False):
    """``loss_and_grad`` of M members at once: ``xs`` (M, nvars, B) and ``ps`` (M, n_params) device tensors, ``eps``
    (M, n_in, B; TrainMode, drawn with ``draw_eps`` when not given), ``t1`` one end time per member (with ``steer_rate > 0``
    and ``t1=None`` each member gets its own ``steer_tspan`` draw: on a host generator member by member, the member's probes and
    then its end time, as a loop of ``loss_and_grad`` would draw them; with a ``HIPRNG`` the probes of all members are ONE device
    draw and the M end times are drawn after it, from the generator's host side).  Returns ``(losses (M,) numpy, grads (M, n_params) device
    tensor, info)``; ``info`` has ``stats`` and ``status`` per member, the members' end times ``t1``, ``launches`` (kernel
    launches per ensemble call, whatever M), ``calls`` (ensemble calls: more than one when M exceeds ``ensemble_capacity``) and
    ``rerun``: the members whose part of the launch gave up and that were run again with ``loss_and_grad``; with
    ``with_steps`` also ``steps``: every member's signed accepted step sizes (cnf_ensemble_steps).  A member whose
    solve went non-finite or hit maxiters raises ``CNFError`` naming it.  ``NotImplementedError`` -- before anything is drawn --
    for what has no ensemble form: conditional models, a non-default ``basedist``, host arrays, PlanarLayer chains, networks
    outside the in-launch gradient's envelope, ``kernel="generic"``.

    Heterogeneous members (cnf_ensemble_set_members): ``counts`` -- M batch sizes within [1, B]: member m uses its first
    ``counts[m]`` columns, every tensor keeps its rectangular shape, the columns at and behind a count are never read or written
    by the device (value outputs there are NaN, input gradients 0, cotangents there are ignored) and a loss is the mean over the
    member's own count; ``reltol`` / ``abstol`` -- a scalar or one per member, in place of ``sol_kwargs``'.  Member m computes, bit
    for bit, what the call with M = 1 at ``B = counts[m]`` computes on ``member_twin`` of it.  ``info["counts"]``,
    ``info["lambdas"]`` and ``info["tols"]`` (abstol, reltol) report what was used.  ``lambdas`` -- (M, 3): the members' own lambda_1..3 (a sweep), zero exactly where the model's are.

    ``bases`` -- an ``EnsembleBases``: member m's base distribution is N(mean_m, L_m L_m') instead of N(0, I) (the model itself
    keeps the default base; cnf_ensemble_set_bases, stream-ordered, no host wait).  The loss is the one under the member's base,
    the gradient's terminal cotangent is formed inside the same launch; a member that is run again takes its base as its twin's
    ``basedist``.  ``with_base`` appends ``(g_mean (M, n_in), g_scale)`` -- d loss_m / d (mean_m, scale_m), ``g_scale`` shaped like
    the scale -- to the result, after ``info`` (cnf_ensemble_base_logpdf_pullback with the loss's weight ``-1 / counts[m]``)."""
    import torch
    if with_base and bases is None:
        raise ValueError("loss_and_grad_many: with_base needs bases")
    s = _settle_density(icnf, mode, xs, ps, eps, t1, "loss_and_grad_many", "loss_and_grad", "cnf_ensemble_capacity", shared=False,
                        members=dict(counts=counts, lambdas=lambdas, reltol=reltol, abstol=abstol), bases=bases)
    l, h = _lib.lib(), icnf.handle()
    m, M, B, xr, pr, er, t1 = s.m, s.M, s.B, s.xr, s.pr, s.er, s.t1
    opts = _solve_opts(icnf, icnf.tspan)
    grads = torch.empty((M, pr.shape[1]), dtype=torch.float32, device=s.dev)
    losses = np.empty(M, dtype=np.float32)
    gb, after = None, None
    if with_base:                                          # the loss is -mean(logpx) + what does not depend on the base: -1 / count per column
        gb = _base_grads(s.bases, M, s.dev)
        cnt = torch.as_tensor(np.asarray(s.het.counts if s.het is not None and s.het.counts is not None else np.full(M, B)), device=s.dev)
        w = (-1.0 / cnt.to(torch.float32))[:, None].expand(M, B).contiguous()
        after = lambda lo, n: _logpdf_pullback(h, s.bases, lo, n, w[lo:lo + n], B, gb, s.stream)
    info, steps = _launch(icnf, s, B, lambda lo, n, status, stats: l.cnf_loss_grad_many(
        h, m, n, pr[lo].data_ptr(), xr[lo].data_ptr(), er[lo].data_ptr() if er is not None else None, B, C.byref(opts),
        t1[lo:].ctypes.data if t1 is not None else None, losses[lo:].ctypes.data, grads[lo].data_ptr(), status, stats, s.stream),
        ensemble_steps if with_steps else None, "t1", t1, after=after)

    def rerun(i, model, k):
        args = dict(eps=er[i, :k].t()) if s.train else {}
        res = loss_and_grad(model, mode, xr[i, :k].t(), pr[i], st, with_base=with_base, **args)
        losses[i] = res[0]
        grads[i].copy_(res[1])
        if with_base:
            gb[0][i].copy_(res[2][0])
            gb[1][i].copy_(res[2][1])
        return _stats_and_steps(model)

    _finish(icnf, info, steps, t1, rerun, s.het, s.bases, with_base)
    icnf.last_stats = info["stats"][0]
    return (losses, grads, info, gb) if with_base else (losses, grads, info)


def _stats_and_steps(icnf: ICNF):
    """What a single-model gradient route reports of the solve it just made: its statistics and signed accepted step sizes."""
    return dict(icnf.last_stats), np.array(icnf.last_steps, dtype=np.float32)


def ensemble_steps(icnf: ICNF, member: int):
    """The signed sizes of the steps ``member`` accepted in the last ensemble CALL on this model (cnf_ensemble_steps; the index
    counts within that call)."""
    l, h = _lib.lib(), icnf.handle()
    n = l.cnf_ensemble_steps(h, int(member), None, 0)
    if n < 0:
        raise ValueError(f"no accepted steps on record for ensemble member {member}")
    hs = np.empty(max(n, 1), dtype=np.float32)
    l.cnf_ensemble_steps(h, int(member), hs.ctypes.data, n)
    return hs[:n]


def _fit_batches(ns, use_batch, batch_size):
    """The batches of one epoch of ``fit_many`` for data sets of ``ns`` rows: a list of ``(lo, counts)`` -- member m's batch is
    ``perm_m[lo : lo + counts[m]]``.  ``ValueError`` unless every member has the same number of batches per epoch
    (``ceil(n_m / batch_size)``): no member sits out an iteration.  Host logic only."""
    ns = np.asarray(ns, dtype=np.int64)
    if (ns < 1).any():
        raise ValueError("fit_many: every data set needs at least one row")
    if not use_batch:
        return [(0, ns.copy())]
    bs = int(batch_size)
    k = (ns + bs - 1) // bs
    if (k != k[0]).any():
        raise ValueError(f"fit_many: every member needs the same number of batches per epoch; batch_size = {bs} gives {k.tolist()} "
                         f"for data sets of {ns.tolist()} rows")
    return [(lo, np.minimum(bs, ns - lo)) for lo in range(0, int(ns.max()), bs)]


def fit_many(model, verbosity: int, Xs, *, seeds=None, lambdas=None, reltol=None, abstol=None, bases=None):
    """``mlj.fit`` for M data sets (folds, bootstrap replicas, or one set M times), trained side by
    side: member m is initialised with ``setup(seeds[m], ...)``, shuffles with its own generator seeded by ``seeds[m]`` and has
    its own rows of the optimiser's state; an iteration is one ``loss_and_grad_many`` and one application of the optimiser to
    the (M, n_params) tensor.  The loop is synchronous; the last, partial batch of an epoch is an ensemble call of its own
    size.  The built-in loss only.  Returns ``([(ps_m, st)], report)``; ``report["losses"]`` is (M, iterations).

    The data sets may have unequal numbers of rows as long as every member has the same number of batches per epoch
    (``ceil(n_m / batch_size)``; ``ValueError`` otherwise, before anything is drawn): the last batch of an epoch is then the one
    ragged call (``counts``).  ``lambdas`` (M, 3), ``reltol`` / ``abstol`` (scalar or M values) make the M members a sweep: they are
    passed to every ``loss_and_grad_many``.  ``bases``: the members' base distributions (an ``EnsembleBases``), kept constant --
    ``ps`` alone is optimised, as ``fit`` keeps its model's base constant."""
    import torch
    from .base_icnf import loss as _builtin_loss
    from .mlj import _device_matrix
    icnf = model.m
    if model.loss is not None and model.loss is not _builtin_loss:
        raise NotImplementedError("fit_many trains on the built-in loss; a custom model.loss goes through fit, one model at a time")
    why = _refusal(icnf)
    if why is not None:
        raise NotImplementedError("fit_many: " + why)
    M = len(Xs)
    if M < 1:
        raise ValueError("fit_many needs at least one data set")
    seeds = list(range(M)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != M:
        raise ValueError("one seed per data set")
    ns = [int(np.shape(X)[0]) for X in Xs]                             # rows of the (n, nvars) tables
    batches = _fit_batches(ns, model.use_batch, model.batch_size)
    sweep = dict(lambdas=lambdas, reltol=reltol, abstol=abstol)
    _members(icnf, M, max(ns), who="fit_many", **sweep)                # (checked before anything is drawn or asks for a device)
    sweep["bases"] = _check_bases(icnf, bases, M, "fit_many")
    mats = [_device_matrix(icnf, X) for X in Xs]
    ragged = len(set(ns)) > 1
    x = pad_columns(mats, max(ns)) if ragged else torch.stack(mats)   # (M, nvars, n)
    n = x.shape[2]
    gens = [np.random.default_rng(s) for s in seeds]
    st = {}
    ps = torch.from_numpy(np.stack([setup(g, icnf.nn, init=model.init)[0] for g in gens])).to(x.device)
    losses = []
    t0 = time.perf_counter()
    it = 0
    rows = torch.arange(M, device=x.device)[:, None]
    for opt in model.optimizers:
        state = opt.init(ps)
        for _epoch in range(model.n_epochs):
            perm = np.zeros((M, n), dtype=np.int64)                    # (behind a member's own rows: index 0, which no call reads)
            for i, g in enumerate(gens):
                perm[i, :ns[i]] = g.permutation(ns[i])
            perm = torch.from_numpy(perm).to(x.device)
            for lo, cnt in batches:
                idx = perm[:, lo:lo + int(cnt.max())]
                xb = x[rows, :, idx].permute(0, 2, 1)                  # (M, nvars, b): member m's own columns
                val, g, _ = loss_and_grad_many(icnf, TrainMode(), xb, ps, st, counts=cnt if (cnt != cnt[0]).any() else None, **sweep)
                opt.apply(state, ps, g)
                losses.append(val)
                it += 1
                if model.callback is not None:
                    model.callback(it, val)
            if verbosity > 0:
                k = len(batches)
                print(f"epoch {_epoch + 1}/{model.n_epochs}: mean loss per member "
                      f"{np.array2string(np.mean(losses[-k:], axis=0), precision=5)}", flush=True)
    torch.cuda.synchronize(x.device)
    report = {"stats": {"time": time.perf_counter() - t0, "iterations": it}, "losses": np.stack(losses, axis=1) if losses else np.zeros((M, 0))}
    host = ps.cpu().numpy()
    return [(host[m].copy(), st) for m in range(M)], report


# ---------------------------------------------------------------------------------------
# scoring and sampling the members (include/cnfhip_ensemble_eval.h)
# ---------------------------------------------------------------------------------------
def ensemble_eval_capacity(icnf: ICNF, mode, B: int) -> int:
    """The largest M one ``inference_many`` / ``generate_many`` launch takes for this model, mode and batch size
    (cnf_ensemble_eval_capacity); 0: no ensemble form."""
    return _capacity(icnf, mode, "cnf_ensemble_eval_capacity", B)


def ensemble_eval_steps(icnf: ICNF, member: int):
    """The step attempts of ``member`` in the last ``inference_many(with_steps=True)`` / ``generate_many(with_steps=True)``
    CALL on this model (cnf_ensemble_eval_steps; the index counts within that call): rows ``(t, signed h, EEst, accepted)``.
    A member that made more attempts than the call kept rows for (1024) returns the rows that were kept: its first ones."""
    l, h = _lib.lib(), icnf.handle()
    n = l.cnf_ensemble_eval_steps(h, int(member), None, 0)
    if n < 0:
        raise ValueError(f"no step attempts on record for ensemble member {member}")
    kept = min(n, _TRACE_ROWS)                             # (what the library copies: min(attempts, cap, trace_cap))
    rows = np.zeros((max(kept, 1), 4), dtype=np.float32)
    l.cnf_ensemble_eval_steps(h, int(member), rows.ctypes.data, kept)
    return rows[:kept]


_TRACE_ROWS = 1024                                         # rows of step trace a member keeps at most


def _trace_cap(opts, with_steps):
    """Rows of step trace per member: a member that makes more attempts than this keeps its first ones."""
    return min(int(opts.maxiters), _TRACE_ROWS) if with_steps else 0


def inference_many(icnf: ICNF, mode, xs, ps, st=None, eps=None, t1=None, with_steps=False, counts=None, lambdas=None, reltol=None,
                   abstol=None, bases=None):
    """``inference`` of M members in one launch (cnf_inference_many).  ``xs`` (M, nvars, B): one data set per member (the
    held-out folds), or (nvars, B): one data set scored by every member (bagging; expanded here, the kernel reads M copies);
    ``ps`` (M, n_params); ``eps`` (M, n_in, B; TrainMode) and ``t1`` as ``loss_and_grad_many`` takes and draws them, in its
    order.  Returns ``(logpx (M, B), (E, n, A) each (M, B), info)``, device tensors; ``info`` has ``stats`` and ``status`` per
    member, ``losses`` (M,), the end times ``t1``, ``launches`` (kernel launches per ensemble call: 1, whatever M), ``calls``
    (more than one when M exceeds ``ensemble_eval_capacity``), ``rerun`` (the members whose part of the launch gave up and
    that were run again with ``inference``) and, with ``with_steps``, ``steps``: per member the rows ``(t, signed h, EEst,
    accepted)`` of its step attempts (None for a member that was run again).  A member whose solve went non-finite or hit maxiters raises ``CNFError`` naming it;
    ``NotImplementedError`` -- before anything is drawn -- for what ``loss_and_grad_many`` refuses.

    Heterogeneous members (cnf_ensemble_set_members): ``counts`` -- M batch sizes within [1, B]: member m uses its first
    ``counts[m]`` columns, every tensor keeps its rectangular shape, the columns at and behind a count are never read or written
    by the device (value outputs there are NaN, input gradients 0, cotangents there are ignored) and a loss is the mean over the
    member's own count; ``reltol`` / ``abstol`` -- a scalar or one per member, in place of ``sol_kwargs``'.  Member m computes, bit
    for bit, what the call with M = 1 at ``B = counts[m]`` computes on ``member_twin`` of it.  ``info["counts"]``,
    ``info["lambdas"]`` and ``info["tols"]`` (abstol, reltol) report what was used.  ``lambdas`` -- (M, 3): they weigh ``info["losses"]`` (``loss_many``).

    ``bases`` -- an ``EnsembleBases``: ``logpx[m]`` and ``info["losses"][m]`` are those under member m's own base N(mean_m, L_m
    L_m'), computed afresh from the final states by a column pass behind the launch; the regulariser rows, the statistics and the
    step sequences are those of the call without bases (the base does not enter the solve)."""
    import torch
    s = _settle_density(icnf, mode, xs, ps, eps, t1, "inference_many", "inference", "cnf_ensemble_eval_capacity",
                        members=dict(counts=counts, lambdas=lambdas, reltol=reltol, abstol=abstol), bases=bases)
    l, h = _lib.lib(), icnf.handle()
    m, M, B, dev, xr, pr, er, t1 = s.m, s.M, s.B, s.dev, s.xr, s.pr, s.er, s.t1
    opts = _solve_opts(icnf, icnf.tspan)
    logpx, regs = _values(s.het, (M, B), dev), _values(s.het, (M, 3, B), dev)
    losses = np.empty(M, dtype=np.float32)
    tc = _trace_cap(opts, with_steps)
    info, steps = _launch(icnf, s, B, lambda lo, n, status, stats: l.cnf_inference_many(
        h, m, n, pr[lo].data_ptr(), xr[lo].data_ptr(), er[lo].data_ptr() if er is not None else None, B, C.byref(opts),
        t1[lo:].ctypes.data if t1 is not None else None, logpx[lo].data_ptr(), regs[lo].data_ptr(), losses[lo:].ctypes.data,
        status, stats, tc, s.stream), ensemble_eval_steps if with_steps else None, "t1", t1, losses=losses)

    def rerun(i, model, k):
        args = dict(eps=er[i, :k].t()) if s.train else {}
        lp, rg, sums = inference(model, mode, xr[i, :k].t(), pr[i], st, with_sums=True, **args)
        logpx[i, :k].copy_(lp)
        regs[i, :, :k].copy_(torch.stack(list(rg)))
        losses[i] = member_loss_from_sums(mode, sums, info["lambdas"][i])
        return dict(model.last_stats), None            # (inference keeps no step trace: None for a member that was run again)

    _finish(icnf, info, steps, t1, rerun, s.het, s.bases)
    icnf.last_stats = info["stats"][0]
    return logpx, (regs[:, 0], regs[:, 1], regs[:, 2]), info


def loss_many(icnf: ICNF, mode, xs, ps, st=None, eps=None, t1=None, counts=None, lambdas=None, reltol=None, abstol=None, bases=None):
    """The M members' losses (``loss`` of each on its own data): ``inference_many(...)[2]["losses"]``, a numpy vector -- with
    ``counts`` means over the members' own counts, with ``lambdas`` weighed by the members' own regularisers, with ``bases`` under
    the members' own base distributions."""
    return inference_many(icnf, mode, xs, ps, st, eps=eps, t1=t1, counts=counts, lambdas=lambdas, reltol=reltol,
                          abstol=abstol, bases=bases)[2]["losses"]


def _values(het, shape, dev):
    """A value output of an ensemble call: uninitialised, or -- members with their own counts -- NaN, which is what stays in the
    columns the device does not touch."""
    import torch
    if het is not None and het.counts is not None:
        return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _input_grads(het, shape, dev):
    """... and an input gradient: zeros there, so that autograd through padded inputs is clean."""
    import torch
    if het is not None and het.counts is not None:
        return torch.zeros(shape, dtype=torch.float32, device=dev)
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _host_gen(icnf: ICNF):
    """The numpy generator behind the model's scalar and index draws (a ``HIPRNG`` keeps one for them)."""
    return icnf.rng._host if isinstance(icnf.rng, HIPRNG) else icnf.rng


def _normals_info(s):
    """``info["normals"]`` of a sampling call whose base samples were drawn through the members' bases: (M, n_in, n)."""
    return dict(normals=s.normals.permute(0, 2, 1)) if s.normals is not None else {}


def _check_sampling_inputs(icnf: ICNF, mode, ps, n, z0, eps, t0, who, single):
    """The argument checks of the sampling calls (``generate_many``, ``generate_vjp_many``).  Host logic only: nothing is drawn,
    no handle is made.  Returns ``(mode id, M, n, n_in, t0 as a float32 vector or None)``."""
    m = _mode_id(mode)
    why = _refusal(icnf)
    if why is not None:
        raise NotImplementedError(f"{who}: " + why)
    if not _is_torch(ps):
        raise NotImplementedError(f"{who} takes device tensors (host arrays: {single}, one member at a time)")
    n_params = icnf.nn.n_params_internal
    if ps.dim() != 2 or ps.shape[0] < 1 or ps.shape[1] != n_params:
        raise ValueError(f"ps must be (M, n_params = {n_params}), got {tuple(ps.shape)}")
    M, n = int(ps.shape[0]), int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    n_in = icnf.nvars + n_augment_input(icnf)
    for name, a in (("z0", z0), ("eps", eps)):
        if a is not None and (not _is_torch(a) or tuple(a.shape) != (M, n_in, n)):
            raise ValueError(f"{name} must be a device tensor (M = {M}, n_in = {n_in}, n = {n})")
    if t0 is not None:
        t0 = np.asarray(t0, dtype=np.float32).reshape(-1)
        if t0.shape[0] != M:
            raise ValueError(f"t0 must have one start time per member (M = {M}), got {t0.shape[0]}")
        if not np.isfinite(t0).all() or (t0 == np.float32(icnf.tspan[0])).any():
            raise ValueError("t0: every member needs a finite start time different from tspan[0]")
    return m, M, n, n_in, t0


def _sampling_draws(icnf: ICNF, mode, train, M, n, n_in, dev, z0, eps, t0, steer=True, counts=None):
    """The members' base samples and probes ([M][n][n_in] on ``dev``) and start times (None: ``tspan[1]`` for all), given or
    drawn in the order ``generate_many`` documents.  ``steer=False``: no steer variate is drawn (the path calls, which are
    this draw with one member).  ``counts``: on a host generator member m draws ``counts[m]`` columns of each -- what a loop of
    ``generate`` at that size draws --, zeros behind them."""
    import torch
    zr = _rows(z0) if z0 is not None else None
    er = _rows(eps) if eps is not None else None
    steer = steer and train and t0 is None and icnf.STEER      # (given start times and TestMode never steer)
    if isinstance(icnf.rng, HIPRNG):
        if zr is None:
            zr = icnf.rng.normal(n_in * M * n, dev.index if dev.index is not None else icnf.device).view(M, n, n_in)
        if er is None:
            er = draw_eps(icnf, _Buf(zr.reshape(-1), n_in, M * n, torch), M * n).arr.view(M, n, n_in)
        if steer:
            t0 = np.asarray([steer_tspan(icnf, mode)[1] for _ in range(M)], dtype=np.float32)
    else:
        host, zs, es, starts = _Buf(None, n_in, n, None), [], [], []
        for i in range(M):                                 # generate_prob's order, member by member
            k = n if counts is None else int(counts[i])
            if zr is None:
                zs.append(np.zeros((n, n_in), dtype=np.float32))
                zs[-1][:k] = icnf.rng.standard_normal((k, n_in)).astype(np.float32)
            if er is None:
                es.append(np.zeros((n, n_in), dtype=np.float32))
                es[-1][:k] = draw_eps(icnf, host if k == n else _Buf(None, n_in, k, None), k).arr.reshape(k, n_in)
            if steer:
                starts.append(steer_tspan(icnf, mode)[1])
        if zr is None:
            zr = torch.from_numpy(np.stack(zs)).to(dev)
        if er is None:
            er = torch.from_numpy(np.stack(es)).to(dev)
        if steer:
            t0 = np.asarray(starts, dtype=np.float32)
    return zr, er, t0


def _settle_sampling(icnf: ICNF, mode, ps, n, z0, eps, t0, who, single, capacity_fn=None, cot_pair=None, members=None, steer=True,
                     bases=None, normals=None):
    """``_settle_density`` for the sampling direction, in the same order: ``_check_sampling_inputs`` and ``cot_pair(M, n)``
    (the call's cotangent tensors); the handle; the device check; the capacity (None: not asked); ``_sampling_draws``.
    ``members``: the call's ``counts``, ``reltol``, ``abstol`` (``_members``).  ``steer=False``: no steer variate is drawn (the path
    calls).  Returns a namespace: ``m, M, n, n_in, train, cot,
    cap, dev, stream, pr, zr, er, t0, het``."""
    import torch
    if normals is not None:                                # given standard normals in place of drawn ones: they go through the bases
        if bases is None or z0 is not None:
            raise ValueError(f"{who}: normals needs bases, and no z0")
        z0 = normals
    m, M, n, n_in, t0 = _check_sampling_inputs(icnf, mode, ps, n, z0, eps, t0, who, single)
    cot = cot_pair(M, n) if cot_pair is not None else ()
    het = _members(icnf, M, n, who=who, **members) if members else None
    bases = _check_bases(icnf, bases, M, who)
    h = icnf.handle() if capacity_fn is not None else None
    if not (ps.is_cuda and all(a is None or a.is_cuda for a in (z0, eps, *cot))):
        raise ValueError(f"{who}: torch tensors must live on the GPU")
    cap = _device_capacity(who, capacity_fn, h, m, n) if capacity_fn is not None else None
    train, dev = m == _lib.MODE_TRAIN, ps.device
    pr = ps.detach().to(torch.float32).contiguous()
    zr, er, t0 = _sampling_draws(icnf, mode, train, M, n, n_in, dev, z0, eps, t0, steer=steer, counts=het.counts if het is not None else None)
    s = SimpleNamespace(m=m, M=M, n=n, n_in=n_in, train=train, cot=cot, cap=cap, dev=dev, pr=pr, zr=zr, er=er, t0=t0, het=het,
                        stream=_stream(_Buf(pr, pr.shape[1], M, torch)), bases=_bases_on(bases, dev), normals=None)
    if s.bases is not None and (z0 is None or normals is not None) and capacity_fn is not None:
        # the standard normals the default would have drawn, at the same offsets, go through mu_m + L_m n: ``_launch`` fills
        # ``s.zr`` from them behind the one cnf_ensemble_set_bases of each launch (cnf_ensemble_base_sample)
        s.normals, s.zr = zr, torch.empty_like(zr)
    return s


def generate_many(icnf: ICNF, mode, ps, st=None, n: int = 1, z0=None, eps=None, t0=None, with_logp=False, with_steps=False,
                  counts=None, reltol=None, abstol=None, bases=None, normals=None):
    """``generate`` of M members in one launch (cnf_generate_many): ``ps`` (M, n_params) on the device, ``z0`` and ``eps``
    (M, n_in, n) device tensors or drawn as ``generate_prob`` draws them -- on a host generator member by member: the member's
    base sample, its probes (drawn in TestMode too, and not used there), then its steered time; with a ``HIPRNG`` ONE draw of
    M n columns for the base samples, one for the probes, then the M steered times from the generator's host side.  ``t0``:
    the members' start times of the reversed span (what ``steer_tspan`` would return as the end time); every member ends at
    ``tspan[0]``.  Returns ``xs (M, nvars, n)``, with ``with_logp`` ``(xs, logq (M, n))``: the log-density of each sample under
    its member (``generate(..., with_logp=True)``).  ``icnf.last_ensemble_info`` holds ``stats``, ``status``, ``launches`` (2:
    the solve and the column kernel), ``calls``, ``rerun``, ``t0`` and the inputs used (``z0``, ``eps``); after ``with_steps``
    the members' step attempts are read with ``ensemble_eval_steps`` (``info["steps"]``).  Failures and refusals as
    ``inference_many``.  ``counts``, ``reltol``, ``abstol``: heterogeneous members, as ``loss_and_grad_many`` takes them (``n`` is then the rectangle's width: member m samples ``counts[m]``
    columns, ``xs`` and ``logq`` behind them are NaN).

    ``bases`` -- an ``EnsembleBases``: member m samples its own base N(mean_m, L_m L_m').  A ``z0`` that is drawn is the standard
    normals the default would have drawn, at the same offsets, passed through ``mean_m + L_m n`` on the device
    (cnf_ensemble_base_sample; ``info["normals"]`` keeps them, ``info["z0"]`` the base samples); a given ``z0`` is taken as it
    is.  ``logq`` is the density under the member's base.  ``normals`` (M, n_in, n; with ``bases``, without ``z0``): standard
    normals to pass through the bases instead of drawing them."""
    import torch
    s = _settle_sampling(icnf, mode, ps, n, z0, eps, t0, "generate_many", "generate", "cnf_ensemble_eval_capacity",
                         members=dict(counts=counts, reltol=reltol, abstol=abstol), bases=bases, normals=normals)
    l, h = _lib.lib(), icnf.handle()
    m, M, n, dev, pr, zr, er, t0 = s.m, s.M, s.n, s.dev, s.pr, s.zr, s.er, s.t0
    opts = _solve_opts(icnf, (icnf.tspan[1], icnf.tspan[0]))              # reverse(tspan)
    xo = _values(s.het, (M, n, icnf.nvars), dev)
    lq = _values(s.het, (M, n), dev) if with_logp else None
    tc = _trace_cap(opts, with_steps)
    info, steps = _launch(icnf, s, n, lambda lo, k, status, stats: l.cnf_generate_many(
        h, m, k, pr[lo].data_ptr(), zr[lo].data_ptr(), er[lo].data_ptr() if s.train else None, n, C.byref(opts),
        t0[lo:].ctypes.data if t0 is not None else None, xo[lo].data_ptr(), lq[lo].data_ptr() if with_logp else None,
        status, stats, tc, s.stream), ensemble_eval_steps if with_steps else None, "t0", t0,
        z0=zr.permute(0, 2, 1), eps=er.permute(0, 2, 1), **_normals_info(s))
    icnf.last_ensemble_info = info                         # (published before a failed member raises: it says which)

    def rerun(i, model, k):
        r = generate(model, mode, pr[i], st, k, z0=zr[i, :k].t(), eps=er[i, :k].t(), with_logp=with_logp)
        xs_i = r[0] if with_logp else r
        xo[i, :k].copy_(torch.as_tensor(xs_i, device=dev)[: icnf.nvars].t())
        if with_logp:
            lq[i, :k].copy_(torch.as_tensor(r[1], device=dev))
        return None, None                              # (generate reports no statistics: the launch's stay)

    _finish(icnf, info, steps, t0, rerun, s.het, s.bases)
    xs = xo.permute(0, 2, 1)                               # (generate does not set icnf.last_stats; nor does this)
    return (xs, lq) if with_logp else xs


# ---------------------------------------------------------------------------------------
# differentiable ensembles (include/cnfhip_ensemble_vjp.h)
# ---------------------------------------------------------------------------------------
def ensemble_vjp_capacity(icnf: ICNF, mode, B: int) -> int:
    """The largest M one ``inference_vjp_many`` launch takes for this model, mode and batch size (cnf_ensemble_vjp_capacity);
    0: no ensemble form."""
    return _capacity(icnf, mode, "cnf_ensemble_vjp_capacity", B)


def _cot_many(cot, M, B):
    """``(g_logpx, (g_E, g_n, g_A))``, each an (M, B) tensor or None (the convention of ``inference_pullback``; a bare None for
    the triple: no cotangent on the regularisers) -> the four rows; ``ValueError`` for anything else.  Host logic only."""
    rows = _cot_rows(cot)
    if rows is None:                                       # (a bare tensor: the single-model calls' other form)
        raise ValueError("cot must be (g_logpx, (g_E, g_n, g_A))")
    for name, r in zip(("g_logpx", "g_E", "g_n", "g_A"), rows):
        if r is None:
            continue
        if not _is_torch(r):
            raise ValueError(f"cot: {name} must be a device tensor or None")
        if tuple(r.shape) != (M, B):
            raise ValueError(f"cot: {name} must be (M = {M}, B = {B}), got {tuple(r.shape)}")
    return rows


def inference_vjp_many(icnf: ICNF, mode, xs, ps, st, cot, eps=None, t1=None, with_x=False, with_steps=False, counts=None,
                       reltol=None, abstol=None, bases=None, with_base=False):
    """``inference`` of M members and its vector-Jacobian product for a per-sample cotangent, in ONE launch and one of the
    partial sums (cnf_inference_vjp_many): what ``inference_record`` + ``inference_pullback`` give for one model.  ``xs``
    (M, nvars, B) or (nvars, B): one data set shared by all members, as ``inference_many`` takes it; ``ps`` (M, n_params);
    ``cot = (g_logpx, (g_E, g_n, g_A))``, each (M, B) or None (zeros) -- the cotangents themselves, not multiplied by the
    regularisers' weights; a row the model does not integrate (``lambda1``, ``lambda2``, ``lambda3`` = 0; all three in
    TestMode) is ignored.  ``eps`` and ``t1`` as ``loss_and_grad_many`` takes and draws them, in its order.  Returns
    ``(logpx (M, B), (E, n, A), grads (M, n_params), [grad_x (M, nvars, B) with with_x,] info)``:
    ``grads[m] = sum_b sum_r cot[r][m, b] d out_r[m, b] / d ps[m]`` through the steps member m's own solve accepted.  ``info``
    as ``loss_and_grad_many``'s, with ``eps`` (M, n_in, B; None in TestMode): the probes used; a member whose part of the launch
    gave up is run again with ``inference_record`` + ``inference_pullback`` (``info["rerun"]``).  Failures and refusals as
    ``loss_and_grad_many``.  ``counts``, ``reltol``, ``abstol``: heterogeneous members, as ``loss_and_grad_many`` takes them (``grad_x`` is 0 behind a member's count, the cotangents there are
    ignored).  ``bases``: the members' own base distributions, as ``loss_and_grad_many`` takes them; ``with_base`` appends
    ``(g_mean (M, n_in), g_scale)`` after ``info``: ``sum_b g_logpx[m, b] d logpx[m, b] / d (mean_m, scale_m)``."""
    import torch
    if with_base and bases is None:
        raise ValueError("inference_vjp_many: with_base needs bases")
    s = _settle_density(icnf, mode, xs, ps, eps, t1, "inference_vjp_many", "inference_record and inference_pullback",
                        "cnf_ensemble_vjp_capacity", cot_rows=lambda M, B: _cot_many(cot, M, B),
                        members=dict(counts=counts, reltol=reltol, abstol=abstol), bases=bases)
    l, h = _lib.lib(), icnf.handle()
    m, M, B, dev, xr, pr, er, t1 = s.m, s.M, s.B, s.dev, s.xr, s.pr, s.er, s.t1
    cm = torch.zeros((M, 4, B), dtype=torch.float32, device=dev)
    for i, r in enumerate(s.cot):
        if r is not None:
            cm[:, i].copy_(r.detach())
    opts = _solve_opts(icnf, icnf.tspan)
    logpx, regs = _values(s.het, (M, B), dev), _values(s.het, (M, 3, B), dev)
    grads = torch.empty((M, pr.shape[1]), dtype=torch.float32, device=dev)
    gz = _input_grads(s.het, (M, B, s.n_in), dev) if with_x else None
    gb, after = None, None
    if with_base:                                          # (logpx alone depends on the base: its cotangent is the weight)
        gb = _base_grads(s.bases, M, dev)
        after = lambda lo, n: _logpdf_pullback(h, s.bases, lo, n, cm[lo:lo + n, 0], B, gb, s.stream)
    info, steps = _launch(icnf, s, B, lambda lo, n, status, stats: l.cnf_inference_vjp_many(
        h, m, n, pr[lo].data_ptr(), xr[lo].data_ptr(), er[lo].data_ptr() if er is not None else None, B, C.byref(opts),
        t1[lo:].ctypes.data if t1 is not None else None, cm[lo].data_ptr(), logpx[lo].data_ptr(), regs[lo].data_ptr(),
        grads[lo].data_ptr(), gz[lo].data_ptr() if with_x else None, status, stats, s.stream),
        ensemble_steps if with_steps else None, "t1", t1, eps=er.permute(0, 2, 1) if er is not None else None, after=after)
    icnf._record = None                                    # (the call ended whatever was recorded on the handle)
    gx = gz[:, :, :icnf.nvars].permute(0, 2, 1).contiguous() if with_x else None

    def rerun(i, model, k):
        from .vjp import inference_pullback, inference_record
        lp, rg = inference_record(model, mode, xr[i, :k].t(), pr[i], st, eps=er[i, :k].t() if s.train else None, tspan=icnf.tspan)
        res = inference_pullback(model, cm[i, :, :k].contiguous(), with_x=with_x, with_base=with_base)
        res = res if isinstance(res, tuple) else (res,)
        logpx[i, :k].copy_(lp)
        regs[i, :, :k].copy_(torch.stack(list(rg)))
        grads[i].copy_(res[0])
        if with_x:
            gx[i, :, :k].copy_(res[1])
        if with_base:
            gb[0][i].copy_(res[-1][0])
            gb[1][i].copy_(res[-1][1])
        return _stats_and_steps(model)

    _finish(icnf, info, steps, t1, rerun, s.het, s.bases, with_base)
    icnf._record = None                                    # (the members' records are not the caller's)
    icnf.last_stats = info["stats"][0]
    out = (logpx, (regs[:, 0], regs[:, 1], regs[:, 2]), grads)
    return out + ((gx, info) if with_x else (info,)) + ((gb,) if with_base else ())


@functools.lru_cache(maxsize=None)
def _autograd_function_many():
    import torch

    class _InferenceMany(torch.autograd.Function):
        @staticmethod
        def forward(ctx, icnf, mode, xs, ps, eps, t1, het, bases, bmean, bscale):
            # (bmean / bscale: the tensors of the members' bases, here so that autograd routes their gradient; the backward
            # launch is given the values the forward read)
            ctx.bases = _frozen_bases(bases, bmean, bscale)
            logpx, (E, n, A), _ = inference_many(icnf, mode, xs.detach(), ps.detach(), None, eps=eps, t1=t1, bases=ctx.bases, **het)
            ctx.icnf, ctx.mode, ctx.het = icnf, mode, het
            # what the backward launch solves again: the same data, parameters, probes and end times
            ctx.xs, ctx.ps, ctx.eps, ctx.t1 = xs.detach(), ps.detach().clone(), eps, t1
            ctx.set_materialize_grads(False)
            return logpx, E.clone(), n.clone(), A.clone()

        @staticmethod
        def backward(ctx, g_logpx, g_E, g_n, g_A):
            icnf = ctx.icnf
            need_x, need_ps = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
            need_b = ctx.bases is not None and (ctx.needs_input_grad[8] or ctx.needs_input_grad[9])
            if not (need_x or need_ps or need_b):
                return (None,) * 10
            res = inference_vjp_many(icnf, ctx.mode, ctx.xs, ctx.ps, None, (g_logpx, (g_E, g_n, g_A)), eps=ctx.eps, t1=ctx.t1,
                                     with_x=bool(need_x), bases=ctx.bases, with_base=bool(need_b), **ctx.het)
            icnf.last_backward_logpx = res[0]              # (the backward launch's own logpx: compared with the forward's in the tests)
            gx = None
            if need_x:
                gx = res[3] if ctx.xs.dim() == 3 else res[3].sum(dim=0)    # (a shared data set collects every member's)
            gm, gs = res[-1] if need_b else (None, None)
            return (None, None, gx, res[2] if need_ps else None, None, None, None, None,
                    gm if ctx.needs_input_grad[8] else None, gs if ctx.needs_input_grad[9] else None)

    return _InferenceMany


def _frozen_bases(bases, bmean, bscale):
    """The members' bases with the values of now (detached copies): what a backward launch is given.  None for None."""
    if bases is None:
        return None
    return EnsembleBases(bmean.detach().clone(), **{bases._name: bscale.detach().clone()})


def _bases_tensors(bases, dev):
    """``(mean, scale)`` of the members' bases on ``dev`` as float32 tensors in the caller's graph; ``(None, None)`` for None."""
    import torch
    if bases is None:
        return None, None
    return tuple(a.to(torch.float32) for a in bases.tensors(dev))


def differentiable_inference_many(icnf: ICNF, mode, xs, ps, st=None, eps=None, t1=None, counts=None, reltol=None, abstol=None,
                                  bases=None):
    """``inference_many`` as a differentiable function of ``ps`` (M, n_params) and, when it requires grad, ``xs`` ((M, nvars, B),
    or (nvars, B) shared by all members): the forward is ``inference_many``, keeping the probes and end times it used; the
    backward is ONE ``inference_vjp_many`` with those same draws.  Returns ``(logpx (M, B), (E, n, A))`` attached to the autograd
    graph.  The backward launch solves again: its gradient is the exact discrete adjoint of the steps IT accepts (the solve is
    deterministic, so they are the forward's for the same inputs; DESIGN 4.4 says how its ``logpx`` compares with the
    forward's -- ``icnf.last_backward_logpx`` keeps it).  ``counts``, ``reltol``, ``abstol``: heterogeneous members, as ``loss_and_grad_many`` takes them: the outputs behind a member's count are NaN
    (mask them out of a loss: their cotangents are ignored) and the gradient of ``xs`` there is 0.  ``bases``: the members' own base
    distributions (an ``EnsembleBases``); when its tensors require grad the backward also returns their gradient -- one ensemble
    call forward, one ensemble call plus the base pullback backward, no host wait for the base in either."""
    if not (_is_torch(xs) and _is_torch(ps)):
        raise NotImplementedError("differentiable_inference_many takes device tensors")
    # the probes and the steered end times are settled here, once (inference_many's order: the probes, then the end times), so
    # that forward and backward are given the very same ones
    het = dict(counts=counts, reltol=reltol, abstol=abstol)
    s = _settle_density(icnf, mode, xs.detach(), ps, eps, t1, "differentiable_inference_many", "differentiable_inference", members=het,
                        bases=bases)
    eps = s.er.permute(0, 2, 1) if s.er is not None else None
    logpx, E, n, A = _autograd_function_many().apply(icnf, mode, xs, ps, eps, s.t1, het, bases, *_bases_tensors(bases, s.dev))
    return logpx, (E, n, A)


# ---------------------------------------------------------------------------------------
# differentiable ensemble sampling (include/cnfhip_ensemble_generate_vjp.h)
# ---------------------------------------------------------------------------------------
def ensemble_generate_vjp_capacity(icnf: ICNF, mode, n: int) -> int:
    """The largest M one ``generate_vjp_many`` launch takes for this model, mode and number of samples per member
    (cnf_ensemble_generate_vjp_capacity); 0: no ensemble form."""
    return _capacity(icnf, mode, "cnf_ensemble_generate_vjp_capacity", n)


def _cot_pair_many(icnf: ICNF, cot, M, n):
    """``(g_x, g_logq)`` -> ``(g_x, g_logq)`` checked: ``g_x`` an (M, nvars, n) or (M, n_in, n) tensor or None, ``g_logq`` an
    (M, n) tensor or None, not both None; ``ValueError`` for anything else.  Host logic only."""
    gx, gl = _cot_two(cot)
    n_in = icnf.nvars + n_augment_input(icnf)
    if gx is None and gl is None:
        raise ValueError("cot: g_x and g_logq are both None")
    if gx is not None:
        if not _is_torch(gx):
            raise ValueError("cot: g_x must be a device tensor or None")
        if tuple(gx.shape) not in ((M, icnf.nvars, n), (M, n_in, n)):
            raise ValueError(f"cot: g_x must be (M = {M}, nvars = {icnf.nvars} or n_in = {n_in}, n = {n}), got {tuple(gx.shape)}")
    if gl is not None:
        if not _is_torch(gl):
            raise ValueError("cot: g_logq must be a device tensor or None")
        if tuple(gl.shape) != (M, n):
            raise ValueError(f"cot: g_logq must be (M = {M}, n = {n}), got {tuple(gl.shape)}")
    return gx, gl


def generate_vjp_many(icnf: ICNF, mode, ps, st, n, cot, z0=None, eps=None, t0=None, with_z0=False, with_steps=False, counts=None,
                      reltol=None, abstol=None, bases=None, with_base=False, normals=None):
    """``generate`` of M members with the log-density of every sample, and the vector-Jacobian product of both for a per-sample
    cotangent, in ONE launch and one of the partial sums plus the column kernels (cnf_generate_vjp_many): what
    ``generate_record`` + ``generate_pullback`` give for one model.  ``ps`` (M, n_params) on the device; ``cot = (g_x, g_logq)``:
    ``g_x`` is (M, nvars, n) or (M, n_in, n) -- rows beyond those given are zero --, ``g_logq`` is (M, n); either may be None
    (zeros), not both.  ``z0``, ``eps`` (M, n_in, n) and ``t0`` (the members' start times of the reversed span) as
    ``generate_many`` takes and draws them, in its order, on a host generator and on a ``HIPRNG``.  Returns
    ``(xs (M, nvars, n), logq (M, n), grads (M, n_params), [grad_z0 (M, n_in, n) with with_z0,] info)``:
    ``grads[m] = sum_b (<g_x[m, :, b], d xs[m, :, b] / d ps[m]> + g_logq[m, b] d logq[m, b] / d ps[m])`` through the steps member
    m's own solve accepted; ``logq`` is the density of the whole n_in-row final state, as ``generate_record``'s.  ``info`` as
    ``generate_many``'s (``t0``, ``z0``, ``eps``: the inputs used), ``launches`` counting the column kernels too; with
    ``with_steps`` also ``steps``: every member's signed accepted step sizes (cnf_ensemble_steps).  A member whose part of the
    launch gave up is run again with ``generate_record`` + ``generate_pullback`` (``info["rerun"]``).  Failures and refusals as
    ``generate_many``: ``NotImplementedError`` before anything is drawn.  ``counts``, ``reltol``, ``abstol``: heterogeneous members, as ``loss_and_grad_many`` takes them (``grad_z0`` is 0 behind a
    member's count, the cotangents there are ignored).  ``bases``: the members' own base distributions, as ``generate_many``
    takes them (a drawn ``z0`` goes through them; ``logq`` and the ``g_logq`` tail of ``grad_z0`` are the member's base's).
    ``with_base`` appends ``(g_mean (M, n_in), g_scale)`` after ``info``: the log-density part at fixed ``z0``, ``sum_b g_logq[m, b]
    d logpdf_m(z0_b) / d (mean_m, scale_m)``, plus -- when ``z0`` was drawn here -- the pullback of the draw ``mean_m + L_m n`` for
    ``grad_z0``: the TOTAL derivative, as ``generate_pullback(..., with_base=True)`` composes it for one model.  ``normals``: as
    ``generate_many`` takes them (they count as drawn here)."""
    import torch
    if with_base and bases is None:
        raise ValueError("generate_vjp_many: with_base needs bases")
    s = _settle_sampling(icnf, mode, ps, n, z0, eps, t0, "generate_vjp_many", "generate_record and generate_pullback",
                         "cnf_ensemble_generate_vjp_capacity", cot_pair=lambda M, n: _cot_pair_many(icnf, cot, M, n),
                         members=dict(counts=counts, reltol=reltol, abstol=abstol), bases=bases, normals=normals)
    with_z0_asked, with_z0 = with_z0, bool(with_z0 or (with_base and s.normals is not None))
    l, h = _lib.lib(), icnf.handle()
    m, M, n, n_in, dev, pr, zr, er, t0 = s.m, s.M, s.n, s.n_in, s.dev, s.pr, s.zr, s.er, s.t0
    gx, gl = s.cot
    cz = cl = None
    if gx is not None:                                     # [M][n][n_in], zeros on the rows that were not given
        cz = torch.zeros((M, n, n_in), dtype=torch.float32, device=dev)
        cz[:, :, :gx.shape[1]] = gx.detach().permute(0, 2, 1)
    if gl is not None:
        cl = gl.detach().to(torch.float32).contiguous()
    opts = _solve_opts(icnf, (icnf.tspan[1], icnf.tspan[0]))              # reverse(tspan)
    xo = _values(s.het, (M, n, icnf.nvars), dev)
    lq = _values(s.het, (M, n), dev)
    grads = torch.empty((M, pr.shape[1]), dtype=torch.float32, device=dev)
    gz = _input_grads(s.het, (M, n, n_in), dev) if with_z0 else None
    gb, after = None, None
    if with_base:
        gb = _base_grads(s.bases, M, dev)
        wl = cl if cl is not None else torch.zeros((M, n), dtype=torch.float32, device=dev)
        after = lambda lo, k: _logpdf_pullback(h, s.bases, lo, k, wl[lo:lo + k], n, gb, s.stream)
    info, steps = _launch(icnf, s, n, lambda lo, k, status, stats: l.cnf_generate_vjp_many(
        h, m, k, pr[lo].data_ptr(), zr[lo].data_ptr(), er[lo].data_ptr() if s.train else None, n, C.byref(opts),
        t0[lo:].ctypes.data if t0 is not None else None, cz[lo].data_ptr() if cz is not None else None,
        cl[lo].data_ptr() if cl is not None else None, xo[lo].data_ptr(), lq[lo].data_ptr(), grads[lo].data_ptr(),
        gz[lo].data_ptr() if with_z0 else None, status, stats, s.stream), ensemble_steps if with_steps else None, "t0", t0,
        z0=zr.permute(0, 2, 1), eps=er.permute(0, 2, 1), after=after, **_normals_info(s))
    icnf._record = None                                    # (the call ended whatever was recorded on the handle)
    icnf.last_ensemble_info = info

    def rerun(i, model, k):
        from .gen_vjp import generate_pullback, generate_record
        x_i, lq_i = generate_record(model, mode, pr[i], st, k, z0=zr[i, :k].t(), eps=er[i, :k].t(), tspan=icnf.tspan)
        res = generate_pullback(model, (cz[i, :k].t() if cz is not None else None, cl[i, :k] if cl is not None else None),
                                with_z0=with_z0, with_base=with_base)
        res = res if isinstance(res, tuple) else (res,)
        xo[i, :k].copy_(x_i.t())
        lq[i, :k].copy_(lq_i)
        grads[i].copy_(res[0])
        if with_z0:
            gz[i, :k].copy_(res[1].t())
        if with_base:                                      # (the log-density part at fixed z0: the record was given its z0)
            gb[0][i].copy_(res[-1][0])
            gb[1][i].copy_(res[-1][1])
        return _stats_and_steps(model)

    _finish(icnf, info, steps, t0, rerun, s.het, s.bases, with_base)
    icnf._record = None                                    # (the members' records are not the caller's)
    icnf.last_stats = info["stats"][0]
    if with_base and s.normals is not None:                # ... plus the pullback of the draw z0 = mean_m + L_m n, for grad_z0
        sm, ss = _sample_pullback(h, s, s.normals, gz)
        gb = (gb[0] + sm, gb[1] + ss)
    out = (xo.permute(0, 2, 1), lq, grads)
    return out + ((gz.permute(0, 2, 1), info) if with_z0_asked else (info,)) + ((gb,) if with_base else ())


def _sample_pullback(h, s, normals, g_z0):
    """cnf_ensemble_base_sample_pullback: ``(sum_b g_z0[m, b], tril(sum_b g_z0[m, b] normals[m, b]'))`` per member, for
    ``normals`` and ``g_z0`` [M][n][n_in]; the members' counts, when the call has some, mask the columns behind them."""
    import torch
    out = _base_grads(s.bases, s.M, s.dev)
    cnt = None
    if s.het is not None and s.het.counts is not None:
        cnt = torch.as_tensor(s.het.counts, device=s.dev).to(torch.int32).contiguous()
    g = g_z0.contiguous()
    _lib.check(_lib.lib().cnf_ensemble_base_sample_pullback(h, s.M, s.bases.kind, normals.data_ptr(), g.data_ptr(), s.n,
                                                            cnt.data_ptr() if cnt is not None else None, out[0].data_ptr(),
                                                            out[1].data_ptr(), s.stream), h)
    return out


@functools.lru_cache(maxsize=None)
def _autograd_function_generate_many():
    import torch

    class _GenerateMany(torch.autograd.Function):
        @staticmethod
        def forward(ctx, icnf, mode, ps, z0, eps, t0, het, bases, bmean, bscale, drawn):
            # (bases, bmean, bscale: as in _InferenceMany; drawn: z0 holds the standard normals that go through the bases)
            n = z0.shape[2]
            ctx.bases = _frozen_bases(bases, bmean, bscale)
            ctx.src = dict(normals=z0.detach()) if drawn else dict(z0=z0.detach())
            xs, logq = generate_many(icnf, mode, ps.detach(), None, n, eps=eps, t0=t0, with_logp=True, bases=ctx.bases, **ctx.src, **het)
            ctx.icnf, ctx.mode, ctx.het = icnf, mode, het
            # what the backward launch solves again: the same parameters, base draws, probes and start times
            ctx.ps, ctx.z0, ctx.eps, ctx.t0 = ps.detach().clone(), z0.detach(), eps, t0
            ctx.set_materialize_grads(False)
            return xs.clone(), logq

        @staticmethod
        def backward(ctx, g_x, g_logq):
            icnf = ctx.icnf
            need_ps, need_z0 = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
            need_b = ctx.bases is not None and (ctx.needs_input_grad[8] or ctx.needs_input_grad[9])
            if (g_x is None and g_logq is None) or not (need_ps or need_z0 or need_b):
                return (None,) * 11
            res = generate_vjp_many(icnf, ctx.mode, ctx.ps, None, ctx.z0.shape[2], (g_x, g_logq), eps=ctx.eps, t0=ctx.t0,
                                    with_z0=bool(need_z0), bases=ctx.bases, with_base=bool(need_b), **ctx.src, **ctx.het)
            # (the backward launch's own outputs: compared with the forward's in the tests)
            icnf.last_backward_xs, icnf.last_backward_logq = res[0], res[1]
            gm, gs = res[-1] if need_b else (None, None)
            return (None, None, res[2] if need_ps else None, res[3].contiguous() if need_z0 else None, None, None, None, None,
                    gm if ctx.needs_input_grad[8] else None, gs if ctx.needs_input_grad[9] else None, None)

    return _GenerateMany


def differentiable_generate_many(icnf: ICNF, mode, ps, st=None, n: int = 1, z0=None, eps=None, t0=None, counts=None, reltol=None,
                                 abstol=None, bases=None):
    """``generate_many(with_logp=True)`` as a differentiable function of ``ps`` (M, n_params) and, when it requires grad, ``z0``
    (M, n_in, n): the forward is ``generate_many`` with the base draws, probes and steered start times settled once (its order);
    the backward is ONE ``generate_vjp_many`` with those same draws.  Returns ``(xs (M, nvars, n), logq (M, n))`` attached to the
    autograd graph.  The backward launch solves again: its gradient is the exact discrete adjoint of the steps IT accepts (the
    solve is deterministic, so they are the forward's for the same inputs; DESIGN 4.4 says how its ``xs`` / ``logq`` compare with
    the forward's -- ``icnf.last_backward_logq`` and ``icnf.last_backward_xs`` keep them).  ``counts``, ``reltol``, ``abstol``: heterogeneous members, as ``loss_and_grad_many`` takes them: ``xs`` and
    ``logq`` behind a member's count are NaN (mask them out of a loss) and the gradient of ``z0`` there is 0.  ``bases``: the members'
    own base distributions (an ``EnsembleBases``): a ``z0`` that is drawn here goes through them, and when its tensors require
    grad the backward returns their TOTAL gradient (the log-density part plus the pullback of the draw) -- the location-scale
    family of a variational fit, per member, with no host wait for the base."""
    het = dict(counts=counts, reltol=reltol, abstol=abstol)
    s = _settle_sampling(icnf, mode, ps, n, z0.detach() if _is_torch(z0) else z0, eps, t0, "differentiable_generate_many",
                         "differentiable_generate", members=het, bases=bases)
    drawn = bases is not None and z0 is None               # (s.zr then holds the standard normals: the launches pass them through the bases)
    if not (z0 is not None and z0.requires_grad):          # (a z0 that asks for a gradient stays the caller's tensor)
        z0 = s.zr.permute(0, 2, 1)
    return _autograd_function_generate_many().apply(icnf, mode, ps, z0, s.er.permute(0, 2, 1), s.t0, het, bases,
                                                    *_bases_tensors(bases, s.dev), drawn)


def reverse_kl_many(icnf: ICNF, mode, ps, st, n, target_logpdf, counts=None, reltol=None, abstol=None, bases=None, **kw):
    """The M members' reverse Kullback-Leibler divergences to unnormalised targets, each estimated on ``n`` samples of its
    member: ``(logq - target_logpdf(xs)).mean(dim=1)``, an (M,) tensor, with ``(xs, logq) = differentiable_generate_many(icnf,
    mode, ps, st, n, **kw)`` -- M variational fits (restarts, targets of one family, a temperature ladder) differentiated by one
    launch; sum or weight the losses as the problem asks.  ``target_logpdf`` is ONE torch callable for all members: it takes
    the samples (M, nvars, n) and returns (M, n) log-densities, so that members with different targets index their own
    parameters by the leading axis (a per-member list would be M calls on slices of one tensor).  ``counts``, ``reltol``, ``abstol``: heterogeneous members, as ``loss_and_grad_many`` takes them: member
    m's divergence is the mean over its own ``counts[m]`` samples (``target_logpdf`` sees zeros in the columns behind them, and
    what it returns there is not used).  ``bases``: the members' own (learnable) base distributions, as
    ``differentiable_generate_many`` takes them: M restarts, each with its own location-scale family."""
    import torch
    xs, logq = differentiable_generate_many(icnf, mode, ps, st, n, counts=counts, reltol=reltol, abstol=abstol, bases=bases, **kw)
    if counts is None:
        t = target_logpdf(xs)
        if tuple(t.shape) != tuple(logq.shape):
            raise ValueError(f"target_logpdf must return (M = {logq.shape[0]}, n = {logq.shape[1]}), got {tuple(t.shape)}")
        return (logq - t).mean(dim=1)
    c = torch.as_tensor(np.asarray(counts), device=logq.device)
    live = torch.arange(logq.shape[1], device=logq.device)[None, :] < c[:, None]
    t = target_logpdf(torch.where(live[:, None, :], xs, torch.zeros_like(xs)))
    if tuple(t.shape) != tuple(logq.shape):
        raise ValueError(f"target_logpdf must return (M = {logq.shape[0]}, n = {logq.shape[1]}), got {tuple(t.shape)}")
    return torch.where(live, logq - t, torch.zeros_like(logq)).sum(dim=1) / c.to(logq.dtype)


# ---- the bagged density: a mixture of the members ----
def mixture_logpdf(logp, weights):
    """``logsumexp_m(log w_m + logp[m, :])`` of an (M, n) matrix of the members' log-densities (numpy array or torch tensor;
    the result is of the same kind).  A member of weight 0 or of log-density -inf contributes nothing; a column in which every
    member does is -inf."""
    if _is_torch(logp):
        import torch
        w = torch.as_tensor(np.asarray(weights, dtype=np.float64), device=logp.device).to(logp.dtype)
        a = logp + torch.log(w)[:, None]
        mx = a.max(dim=0).values
        safe = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        return safe + torch.log(torch.exp(a - safe).sum(dim=0))
    logp = np.asarray(logp)
    with np.errstate(divide="ignore"):
        a = logp + np.log(np.asarray(weights, dtype=logp.dtype))[:, None]
        mx = a.max(axis=0)
        safe = np.where(np.isfinite(mx), mx, 0)
        return safe + np.log(np.exp(a - safe).sum(axis=0))


def split_counts(rng, n: int, weights):
    """How many of ``n`` draws of a mixture come from each member: ONE multinomial draw of the numpy generator ``rng``.  Returns
    an int64 vector that sums to n; members may get none."""
    w = check_weights(weights, len(weights))
    return np.asarray(rng.multinomial(int(n), w), dtype=np.int64)


def check_weights(weights, M):
    """Mixture weights as float64: M finite values >= 0 that sum to 1 (within 1e-6: they are normalised); None: uniform."""
    if weights is None:
        return np.full(M, 1.0 / M)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != M or not np.isfinite(w).all() or (w < 0).any() or abs(w.sum() - 1.0) > 1e-6:
        raise ValueError(f"weights: {M} values >= 0 that sum to 1")
    return w / w.sum()


class EnsembleDist:
    """The bagged density of M members of one architecture: ``sum_m w_m p_m`` (``weights``: uniform by default).  ``ps`` is the
    (M, n_params) device tensor ``fit_many`` trains (or a list of its ``(ps_m, st)`` results).  ``bases``: an ``EnsembleBases`` --
    component m has the base N(mean_m, L_m L_m'): a mixture whose components sit in different places."""

    def __init__(self, icnf: ICNF, mode, ps, st=None, weights=None, bases=None):
        why = _refusal(icnf)
        if why is not None:
            raise NotImplementedError("EnsembleDist: " + why)
        _mode_id(mode)
        if isinstance(ps, (list, tuple)):
            import torch
            ps = torch.from_numpy(np.stack([np.asarray(p[0] if isinstance(p, tuple) else p, dtype=np.float32) for p in ps]))
            ps = ps.to(torch.device("cuda", icnf.device))
        if not _is_torch(ps) or ps.dim() != 2:
            raise ValueError("ps must be an (M, n_params) tensor")
        self.m, self.mode, self.ps, self.st = icnf, mode, ps, st
        self.bases = _check_bases(icnf, bases, int(ps.shape[0]), "EnsembleDist")      # the components' own base distributions
        # (a tensor of weights -- e.g. the softmax of logits that stacking trains -- is kept for log_prob; its values are checked
        # like any others)
        self.weights_t = weights if _is_torch(weights) else None
        self.weights = check_weights(weights.detach().cpu().numpy() if _is_torch(weights) else weights, int(ps.shape[0]))

    def __len__(self):
        return self.m.nvars

    def logpdf_members(self, A, *, eps=None):
        """Every member's ``logpdf`` of the columns of ``A`` (nvars, n): (M, n), one launch."""
        return inference_many(self.m, self.mode, A, self.ps, self.st, eps=eps, bases=self.bases)[0]

    def logpdf(self, A, *, eps=None):
        return mixture_logpdf(self.logpdf_members(A, eps=eps), self.weights)

    def pdf(self, A, *, eps=None):
        return self.logpdf(A, eps=eps).exp()

    def log_prob(self, xs):
        """The mixture's exact log-density ``logsumexp_m(log w_m + logpdf_m(xs))`` of the columns of ``xs`` (nvars, n) as a
        differentiable function of the members' parameters ``ps``, of ``xs`` and of ``weights`` when that is a tensor requiring
        grad (stacking: the mixture weights trained together with the members; ``log_softmax`` of logits is the caller's
        business): ``differentiable_inference_many`` in TestMode -- one launch forward, one ``inference_vjp_many`` backward."""
        import torch
        from .types import TestMode
        logp = differentiable_inference_many(self.m, TestMode(), xs, self.ps, self.st, bases=self.bases)[0]
        w = self.weights_t if self.weights_t is not None else torch.as_tensor(self.weights)
        return torch.logsumexp(logp + torch.log(w.to(device=logp.device, dtype=logp.dtype))[:, None], dim=0)

    def rand(self, n: int, *, with_members=False, ragged=False):
        """``n`` draws of the mixture, (nvars, n) on the device: the members' counts from one multinomial draw on the model's
        host generator (``split_counts``), then ONE ``generate_many`` with ``B = max count`` columns per member, of which member
        m keeps its first ``count_m``; the draws are ordered by member.  The launch computes M max(count) columns for n kept
        ones: M max(count) - n are wasted (about (M - 1) / M of them for a one-hot mixture, few for uniform weights and
        n >> M).  ``with_members``: also the member index of every column.  ``ragged=True``: the same multinomial draw, then one
        ``generate_many`` over the members with a non-zero count only, with ``counts`` = their counts: every member solves just
        its own columns (a one-hot mixture launches one member); on a host generator the base draws are then the members' own
        ``count_m`` columns, so the samples differ from the default's for the same seed."""
        import torch
        if int(n) < 1:                                     # (nothing is drawn, nothing is launched)
            if int(n) < 0:
                raise ValueError("n must be >= 0")
            out = torch.empty((self.m.nvars, 0), dtype=torch.float32, device=self.ps.device)
            return (out, np.zeros(0, dtype=np.int64)) if with_members else out
        counts = split_counts(_host_gen(self.m), n, self.weights)
        if ragged:
            live = np.flatnonzero(counts)
            xs = generate_many(self.m, self.mode, self.ps[torch.as_tensor(live, device=self.ps.device)], self.st, int(counts.max()),
                               counts=counts[live], bases=self.bases.take(live) if self.bases is not None else None)
            out = torch.cat([xs[j, :, :counts[i]] for j, i in enumerate(live)], dim=1)
            return (out, np.repeat(np.arange(len(counts)), counts)) if with_members else out
        xs = generate_many(self.m, self.mode, self.ps, self.st, int(counts.max()), bases=self.bases)
        out = torch.cat([xs[i, :, :c] for i, c in enumerate(counts)], dim=1)
        if with_members:
            return out, np.repeat(np.arange(len(counts)), counts)
        return out


def logpdf_members(d: EnsembleDist, A, *, eps=None):
    return d.logpdf_members(A, eps=eps)
