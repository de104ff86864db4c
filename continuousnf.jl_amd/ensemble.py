"""Ensembles: M independent models of one architecture -- cross-validation folds, bootstrap replicas, seeds, sweeps -- whose
losses and gradients come out of ONE launch (cnf_loss_grad_many, include/cnfhip_ensemble.h).  The reference trains its README /
regression networks at ``batch_size = 32`` (src/exts/mlj_ext/core_icnf.jl:59-73); a gradient of one such model occupies two
workgroups of the device; here M of them run side by side on M times as many (measured: tools/prof_ensemble.py).

``loss_and_grad_many`` is ``loss_and_grad`` for M members with their own parameters, data, probes and end times;
``fit_many`` is ``mlj.fit`` for M data sets trained side by side.  Inference and ``logpdf`` of the members go through the
existing calls, one member at a time."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import _lib
from .base_icnf import ICNF, _Buf, _is_torch, _mode_id, _solve_opts, draw_eps, loss_and_grad, n_augment_input, steer_tspan
from .layers import setup
from .rng import HIPRNG
from .types import TrainMode


def _refusal(icnf: ICNF):
    """Why this model has no ensemble form, or None.  Host logic only: nothing is drawn, no handle is made.  The network
    envelope restates `ens_fn` / `pick_grad_ens` of csrc/cnf_wave.hip (which decides for the C ABI): change both together."""
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


def ensemble_capacity(icnf: ICNF, mode, B: int) -> int:
    """The largest M one launch takes for this model, mode and batch size (cnf_ensemble_capacity); 0: no ensemble form."""
    m = _mode_id(mode)
    if _refusal(icnf) is not None:
        return 0
    return int(_lib.lib().cnf_ensemble_capacity(icnf.handle(), m, int(B)))


def _check_inputs(icnf: ICNF, mode, xs, ps, eps, t1):
    m = _mode_id(mode)
    why = _refusal(icnf)
    if why is not None:
        raise NotImplementedError("loss_and_grad_many: " + why)
    if not (_is_torch(xs) and _is_torch(ps)):
        raise NotImplementedError("loss_and_grad_many takes device tensors (host arrays: loss_and_grad, one member at a time)")
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


def _rows(x):
    """(M, rows, B) -> the bytes the C ABI reads: [M][B][rows]."""
    import torch
    return x.detach().to(torch.float32).permute(0, 2, 1).contiguous()


def loss_and_grad_many(icnf: ICNF, mode, xs, ps, st=None, eps=None, t1=None, with_steps=False):
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
    outside the in-launch gradient's envelope, ``kernel="generic"``."""
    import torch
    m, M, B, n_in, t1 = _check_inputs(icnf, mode, xs, ps, eps, t1)
    l, h = _lib.lib(), icnf.handle()                       # (no device: cnf_create's error, as everywhere)
    if not (xs.is_cuda and ps.is_cuda and (eps is None or eps.is_cuda)):
        raise ValueError("loss_and_grad_many: torch tensors must live on the GPU")
    cap = int(l.cnf_ensemble_capacity(h, m, B))
    if cap < 1:
        raise NotImplementedError("loss_and_grad_many: no ensemble form for this model, mode or batch on this device "
                                  "(cnf_ensemble_capacity is 0)")
    train = m == _lib.MODE_TRAIN
    dev = xs.device
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    xr = _rows(xs)
    pr = ps.detach().to(torch.float32).contiguous()
    if not train:
        er = None
    elif eps is not None:
        er = _rows(eps)
    elif isinstance(icnf.rng, HIPRNG):                     # one draw of M B columns
        er = draw_eps(icnf, _Buf(xr.view(-1), icnf.nvars, M * B, torch), M * B).arr.view(M, B, n_in)
    else:
        # the host generator, member by member in the order a loop of ``loss_and_grad`` consumes it (the member's probes, then
        # its end time: base_icnf.loss_and_grad), so that one seed gives the members the draws that loop would; one upload
        host, draws = _Buf(None, icnf.nvars, B, None), []
        steer = t1 is None and icnf.STEER
        ends = []
        for _ in range(M):
            draws.append(draw_eps(icnf, host, B).arr.reshape(B, n_in))
            if steer:
                ends.append(steer_tspan(icnf, mode)[1])
        er = torch.from_numpy(np.stack(draws)).to(dev)
        if steer:
            t1 = np.asarray(ends, dtype=np.float32)
    if t1 is None and icnf.STEER and train:                # (given probes, TestMode never steers, or a device generator: M draws)
        t1 = np.asarray([steer_tspan(icnf, mode)[1] for _ in range(M)], dtype=np.float32)
    opts = _solve_opts(icnf, icnf.tspan)
    n_params = pr.shape[1]
    grads = torch.empty((M, n_params), dtype=torch.float32, device=dev)
    losses = np.empty(M, dtype=np.float32)
    status = np.empty(M, dtype=np.int32)
    stats = (_lib.cnf_solve_stats * M)()
    calls, steps = 0, []
    for lo in range(0, M, cap):                            # M above the capacity: consecutive launches
        n = min(cap, M - lo)
        _lib.check(l.cnf_loss_grad_many(
            h, m, n, pr[lo].data_ptr(), xr[lo].data_ptr(), er[lo].data_ptr() if er is not None else None, B, C.byref(opts),
            t1[lo:].ctypes.data if t1 is not None else None, losses[lo:].ctypes.data, grads[lo].data_ptr(),
            status[lo:].ctypes.data, C.byref(stats, lo * C.sizeof(_lib.cnf_solve_stats)), stream), h)
        calls += 1
        if with_steps:
            steps += [ensemble_steps(icnf, i) if status[lo + i] == _lib.OK else None for i in range(n)]
    info = {"stats": [s.as_dict() for s in stats], "status": status, "launches": max(s.launches for s in stats), "calls": calls, "rerun": [],
            "t1": t1 if t1 is not None else np.full(M, icnf.tspan[1], dtype=np.float32)}
    for i in range(M):
        if status[i] in (_lib.ERR_NONFINITE, _lib.ERR_MAXITERS):
            raise _lib.CNFError(int(status[i]), f"ensemble member {i}: " + l.cnf_status_string(int(status[i])).decode())
    gave_up = [i for i in range(M) if status[i] != _lib.OK]
    if gave_up:
        # the existing route, its fallbacks included, on the member's own end time
        span = icnf.tspan
        try:
            for i in gave_up:
                if t1 is not None:
                    icnf.tspan = (span[0], float(t1[i]))
                steer, icnf.steer_rate = icnf.steer_rate, 0.0
                try:
                    args = dict(eps=er[i].t()) if train else {}
                    val, g = loss_and_grad(icnf, mode, xr[i].t(), pr[i], st, **args)
                finally:
                    icnf.steer_rate = steer
                losses[i] = val
                grads[i].copy_(g)
                status[i] = _lib.OK
                info["stats"][i] = dict(icnf.last_stats)
                if with_steps:
                    steps[i] = np.array(icnf.last_steps, dtype=np.float32)
        finally:
            icnf.tspan = span
        info["rerun"] = gave_up
    if with_steps:
        info["steps"] = steps
    icnf.last_stats = info["stats"][0]
    return losses, grads, info


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


def fit_many(model, verbosity: int, Xs, *, seeds=None):
    """``mlj.fit`` for M data sets of the same number of rows (folds, bootstrap replicas, or one set M times), trained side by
    side: member m is initialised with ``setup(seeds[m], ...)``, shuffles with its own generator seeded by ``seeds[m]`` and has
    its own rows of the optimiser's state; an iteration is one ``loss_and_grad_many`` and one application of the optimiser to
    the (M, n_params) tensor.  The loop is synchronous; the last, partial batch of an epoch is an ensemble call of its own
    size.  The built-in loss only.  Returns ``([(ps_m, st)], report)``; ``report["losses"]`` is (M, iterations)."""
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
    x = torch.stack([_device_matrix(icnf, X) for X in Xs])             # (M, nvars, n): equal row counts or stack refuses
    n = x.shape[2]
    gens = [np.random.default_rng(s) for s in seeds]
    st = {}
    ps = torch.from_numpy(np.stack([setup(g, icnf.nn, init=model.init)[0] for g in gens])).to(x.device)
    bs = model.batch_size if model.use_batch else n
    losses = []
    t0 = time.perf_counter()
    it = 0
    rows = torch.arange(M, device=x.device)[:, None]
    for opt in model.optimizers:
        state = opt.init(ps)
        for _epoch in range(model.n_epochs):
            perm = torch.from_numpy(np.stack([g.permutation(n) for g in gens])).to(x.device)
            for lo in range(0, n, bs):
                idx = perm[:, lo:lo + bs]
                xb = x[rows, :, idx].permute(0, 2, 1)                  # (M, nvars, b): member m's own columns
                val, g, _ = loss_and_grad_many(icnf, TrainMode(), xb, ps, st)
                opt.apply(state, ps, g)
                losses.append(val)
                it += 1
                if model.callback is not None:
                    model.callback(it, val)
            if verbosity > 0:
                k = max(1, (n + bs - 1) // bs)
                print(f"epoch {_epoch + 1}/{model.n_epochs}: mean loss per member "
                      f"{np.array2string(np.mean(losses[-k:], axis=0), precision=5)}", flush=True)
    torch.cuda.synchronize(x.device)
    report = {"stats": {"time": time.perf_counter() - t0, "iterations": it}, "losses": np.stack(losses, axis=1) if losses else np.zeros((M, 0))}
    host = ps.cpu().numpy()
    return [(host[m].copy(), st) for m in range(M)], report
