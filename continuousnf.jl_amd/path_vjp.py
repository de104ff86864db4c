"""Differentiable flow paths: the state of the flow at caller-given times AND the vector-Jacobian product of a cotangent of
those slices, in one launch (cnf_inference_path_vjp / cnf_generate_path_vjp, include/cnfhip_path_vjp.h).  ``path.py`` is the
forward half; here a loss may sit on the path itself: matching the particles at ``tau_k`` to observed snapshots, annealed
reverse-KL over the intermediate ``logq(tau_k)``, kinetic penalties between save times, consistency of intermediate densities.

The launch solves, stores the path and runs the discrete adjoint of the steps it accepted with the slices' cotangents injected
at the save times (the adjoint of Tsit5's interpolant).  The accepted steps -- hence ``theta = (tau - t_n) / h_n`` -- are
constants of that adjoint, as everywhere in this package.  It is the launch of ``inference_vjp_many`` / ``generate_vjp_many``
with one member, so its envelope is ``ensemble._refusal``'s, and device tensors only.  Neither call steers, as the path calls
do not.  There is no streamed route behind it: a solve of more accepted steps than one launch differentiates is an error.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _lib
from .base_icnf import ICNF, _Buf, _is_torch, _mode_id, _solve_opts, _stream, n_augment_input
from .ensemble import _capacity, _probes_and_ends, _refusal, _sampling_draws
from .path import _accepted_steps, _path_rows, check_saveat, generate_path, inference_path


def path_vjp_max_batch(icnf: ICNF, mode) -> int:
    """The largest batch one ``inference_path_vjp`` / ``generate_path_vjp`` launch takes for this model and mode
    (cnf_path_vjp_max_batch); 0: no such form."""
    return _capacity(icnf, mode, "cnf_path_vjp_max_batch")


def path_vjp_steps(icnf: ICNF):
    """``(t_n, h_n)`` of the accepted steps of the last ``*_path_vjp`` call on this model (cnf_path_vjp_steps): two float32
    vectors, or ``None`` when there is none."""
    return _accepted_steps(icnf, "cnf_path_vjp_steps")


def _refuse(icnf: ICNF, who, single, *tensors):
    """The refusals both calls share, on the host, before anything is drawn or a handle is made."""
    why = _refusal(icnf)
    if why is not None:
        raise NotImplementedError(f"{who}: " + why)          # (in the words of the ensemble calls: it is their launch)
    if not all(_is_torch(t) for t in tensors):
        raise NotImplementedError(f"{who} takes device tensors (host arrays: {single} over the sub-spans)")


def _check_batch(icnf: ICNF, who, m, B):
    h = icnf.handle()
    key, hit = (h.value if hasattr(h, "value") else h, m), getattr(icnf, "_path_vjp_cap", None)
    if hit is None or hit[0] != key:                       # (asked once per handle and mode: the answer walks the batch sizes)
        hit = icnf._path_vjp_cap = (key, int(_lib.lib().cnf_path_vjp_max_batch(h, m)))
    cap = hit[1]
    if B > cap:
        raise NotImplementedError(f"{who}: B = {B} is above what one launch takes (cnf_path_vjp_max_batch = {cap})")


def _path_cot(icnf: ICNF, who, path_cot, names, K, B, train, dev):
    """The dict of row cotangents -> ``[K][B][D]`` (None: nothing given).  ``names``: key -> state row (``z``: rows 0..n_in)."""
    import torch
    if path_cot is None:
        return None
    if not isinstance(path_cot, dict) or any(k not in names for k in path_cot):
        raise ValueError(f"{who}: path_cot is a dict with any of {sorted(names)}")
    n_in = icnf.nvars + n_augment_input(icnf)
    D = n_in + (3 if train else 1)
    given = {k: v for k, v in path_cot.items() if v is not None}
    if not given:
        return None
    pc = torch.zeros((K, B, D), dtype=torch.float32, device=dev)
    for k, v in given.items():
        if not _is_torch(v):
            raise ValueError(f"{who}: path_cot[{k!r}] must be a device tensor")
        row = names[k]
        if row >= n_in + (3 if train else 1):
            raise ValueError(f"{who}: path_cot[{k!r}] has no meaning in TestMode (the row is not integrated)")
        want = (K, n_in, B) if k == "z" else (K, B)
        if tuple(v.shape) != want:
            raise ValueError(f"{who}: path_cot[{k!r}] must be {want}, got {tuple(v.shape)}")
        v = v.detach().to(device=dev, dtype=torch.float32)
        if k == "z":
            pc[:, :, :n_in] = v.permute(0, 2, 1)
        else:
            pc[:, :, row] = v
    return pc


def _probes(icnf: ICNF, mode, train, xr, eps):
    """The probes of a single-model call on the data ``xr`` ([B][nvars]), as [B][n_in] (None in TestMode): ``eps`` (n_in, B), or
    the ensemble calls' draw with one member -- and no steer variate: the path calls integrate ``icnf.tspan``."""
    B, n_in = xr.shape[0], icnf.nvars + n_augment_input(icnf)
    er, _ = _probes_and_ends(icnf, mode, train, 1, B, n_in, xr[None], eps[None] if eps is not None else None, None, steer=False)
    return er[0] if er is not None else None


def inference_path_vjp(icnf: ICNF, mode, xs, ps, st=None, *, saveat, cot=None, path_cot=None, eps=None, with_x=False):
    """``inference_path`` and the vector-Jacobian product of its outputs and of the path, in ONE launch and one of the partial
    sums.  ``xs`` (nvars, B) and ``ps`` (n_params,) are device tensors; ``cot = (g_logpx, (g_E, g_n, g_A))`` as
    ``inference_pullback`` takes it (each (B,) or None; None: no cotangent of the outputs); ``path_cot``: a dict with any of
    ``z`` (K, n_in, B), ``dlogp`` (K, B) and in TrainMode ``E``, ``n`` (K, B) -- the cotangents of ``path[...]``, missing rows
    are zero.  Returns ``(logpx, (E, n, A), path, grads[, grad_x], info)``: ``path`` as ``inference_path``'s, ``grads``
    (n_params,) ``= sum_b (sum_r cot[r][b] d out_r[b] + sum_k <path_cot[k][:, b], d path[k][:, b]>) / d ps`` through the steps
    this solve accepted, ``grad_x`` (nvars, B) the same w.r.t. ``xs``; ``info`` holds ``steps`` (``(t_n, h_n)``) and ``stats``.
    Integrates ``icnf.tspan``: no steer variate is drawn.  ``NotImplementedError`` -- before anything is drawn, without making
    a handle -- for whatever ``inference_vjp_many`` refuses (conditional models, non-default bases, Planar chains,
    ``kernel='generic'``, networks outside two tanh layers / n_in <= 16 / <= 64 hidden units) and host arrays; and for
    ``B > path_vjp_max_batch``.  ``CNFError`` when the solve fails -- ``ERR_UNSUPPORTED`` for a solve of more accepted steps
    than one launch differentiates: this call has no streamed route."""
    import torch
    who = "inference_path_vjp"
    m = _mode_id(mode)
    _refuse(icnf, who, "inference_record and inference_pullback", xs, ps)
    sv = check_saveat(saveat, icnf.tspan)
    if xs.dim() != 2 or xs.shape[0] != icnf.nvars or xs.shape[1] < 1:
        raise ValueError(f"xs must be (nvars = {icnf.nvars}, B), got {tuple(xs.shape)}")
    B, K = int(xs.shape[1]), int(sv.size)
    n_params = icnf.nn.n_params_internal
    if ps.numel() != n_params:
        raise ValueError(f"ps must have n_params = {n_params} entries, got {ps.numel()}")
    train = m == _lib.MODE_TRAIN
    n_in = icnf.nvars + n_augment_input(icnf)
    D = n_in + (3 if train else 1)
    if eps is not None:
        if not train:
            raise ValueError("eps has no meaning in TestMode (exact trace)")
        if not _is_torch(eps) or tuple(eps.shape) != (n_in, B):
            raise ValueError(f"eps must be a device tensor (n_in = {n_in}, B = {B})")
    if not (xs.is_cuda and ps.is_cuda and (eps is None or eps.is_cuda)):
        raise ValueError(f"{who}: torch tensors must live on the GPU")
    dev = xs.device
    from .vjp import _cot_matrix
    cm = _cot_matrix(cot, B, dev) if cot is not None else None
    pc = _path_cot(icnf, who, path_cot, {"z": 0, "dlogp": n_in, "E": n_in + 1, "n": n_in + 2}, K, B, train, dev)
    l, h = _lib.lib(), icnf.handle()
    _check_batch(icnf, who, m, B)
    xr = xs.detach().to(torch.float32).t().contiguous()
    pr = ps.detach().to(torch.float32).contiguous().reshape(-1)
    er = _probes(icnf, mode, train, xr, eps)
    opts = _solve_opts(icnf, icnf.tspan)
    stream = _stream(_Buf(xr.view(-1), icnf.nvars, B, torch))
    logpx, regs = torch.empty(B, dtype=torch.float32, device=dev), torch.empty((3, B), dtype=torch.float32, device=dev)
    pth = torch.empty((K, B, D), dtype=torch.float32, device=dev)
    grads = torch.empty(n_params, dtype=torch.float32, device=dev)
    gz = torch.empty((B, n_in), dtype=torch.float32, device=dev) if with_x else None
    stats = _lib.cnf_solve_stats()
    icnf._record = None                                    # (the call ends whatever was recorded on the handle)
    _lib.check(l.cnf_inference_path_vjp(h, m, pr.data_ptr(), xr.data_ptr(), er.data_ptr() if er is not None else None, B, C.byref(opts),
                                        sv.ctypes.data, K, cm.data_ptr() if cm is not None else None,
                                        pc.data_ptr() if pc is not None else None, logpx.data_ptr(), regs.data_ptr(), pth.data_ptr(),
                                        grads.data_ptr(), gz.data_ptr() if with_x else None, C.byref(stats), stream), h)
    icnf.last_stats = stats.as_dict()
    info = {"stats": icnf.last_stats, "steps": path_vjp_steps(icnf), "eps": er.t() if er is not None else None}
    path = _path_rows(icnf, m, pth.permute(0, 2, 1), {"t": sv, "steps": info["steps"]})
    out = (logpx, (regs[0], regs[1], regs[2]), path, grads)
    return out + ((gz[:, :icnf.nvars].t().contiguous(), info) if with_x else (info,))


def generate_path_vjp(icnf: ICNF, mode, ps, st=None, n: int = 1, *, saveat, cot=None, path_cot=None, z0=None, eps=None, with_z0=False):
    """``generate_path`` and the vector-Jacobian product of ``(xs, logq)`` and of the path, in ONE launch, one of the partial
    sums and the column kernels.  ``ps`` (n_params,) on the device; ``saveat`` runs from ``tspan[1]`` to ``tspan[0]``;
    ``cot = (g_x, g_logq)`` as ``generate_pullback`` takes it (``g_x`` (nvars, n) or (n_in, n), ``g_logq`` (n,); None entries,
    or None for the pair: zeros); ``path_cot``: a dict with any of ``z`` (K, n_in, n) and ``logq`` (K, n) -- the cotangent of
    ``path["logq"] = logpdf(N(0, I), z0) + dlogp(tau_k)``: it goes to the dlogp row, and its sum over k joins ``g_logq`` in the
    ``-(...) z0`` tail of ``grad_z0``.  ``z0`` / ``eps`` (n_in, n) device tensors, drawn as ``generate_prob`` draws them when
    not given.  Returns ``(xs, logq, path, grads[, grad_z0], info)``; ``info`` holds ``steps``, ``stats`` and the inputs used
    (``z0``, ``eps``).  No steer variate is drawn.  Refusals and failures as ``inference_path_vjp``."""
    import torch
    who = "generate_path_vjp"
    m = _mode_id(mode)
    _refuse(icnf, who, "generate_record and generate_pullback", ps)
    t0, t1 = icnf.tspan
    sv = check_saveat(saveat, (t1, t0))
    n, K = int(n), int(sv.size)
    if n < 1:
        raise ValueError("n must be >= 1")
    n_params = icnf.nn.n_params_internal
    if ps.numel() != n_params:
        raise ValueError(f"ps must have n_params = {n_params} entries, got {ps.numel()}")
    train = m == _lib.MODE_TRAIN
    n_in = icnf.nvars + n_augment_input(icnf)
    D = n_in + (3 if train else 1)
    for name, a in (("z0", z0), ("eps", eps)):
        if a is not None and (not _is_torch(a) or tuple(a.shape) != (n_in, n)):
            raise ValueError(f"{name} must be a device tensor (n_in = {n_in}, n = {n})")
    if not (ps.is_cuda and (z0 is None or z0.is_cuda) and (eps is None or eps.is_cuda)):
        raise ValueError(f"{who}: torch tensors must live on the GPU")
    dev = ps.device
    cz = cl = None
    if cot is not None:
        from .gen_vjp import _cot_pair
        cz, cl, Bc = _cot_pair(icnf, cot, dev)
        if (cz is not None or cl is not None) and Bc != n:
            raise ValueError("g_x and g_logq need one column / entry per sample")
    pc = _path_cot(icnf, who, path_cot, {"z": 0, "logq": n_in}, K, n, train, dev)
    l, h = _lib.lib(), icnf.handle()
    _check_batch(icnf, who, m, n)
    zr, er, _ = _sampling_draws(icnf, mode, train, 1, n, n_in, dev, z0.unsqueeze(0) if z0 is not None else None,
                                eps.unsqueeze(0) if eps is not None else None, None, steer=False)
    zr, er = zr[0].contiguous(), er[0].contiguous()
    pr = ps.detach().to(torch.float32).contiguous().reshape(-1)
    opts = _solve_opts(icnf, (t1, t0))                     # reverse(tspan)
    stream = _stream(_Buf(pr, n_params, 1, torch))
    xo, lq = torch.empty((n, icnf.nvars), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    pth = torch.empty((K, n, D), dtype=torch.float32, device=dev)
    grads = torch.empty(n_params, dtype=torch.float32, device=dev)
    gz = torch.empty((n, n_in), dtype=torch.float32, device=dev) if with_z0 else None
    stats = _lib.cnf_solve_stats()
    icnf._record = None                                    # (the call ends whatever was recorded on the handle)
    _lib.check(l.cnf_generate_path_vjp(h, m, pr.data_ptr(), zr.data_ptr(), er.data_ptr() if train else None, n, C.byref(opts),
                                       sv.ctypes.data, K, cz.data_ptr() if cz is not None else None,
                                       cl.data_ptr() if cl is not None else None, pc.data_ptr() if pc is not None else None,
                                       xo.data_ptr(), lq.data_ptr(), pth.data_ptr(), grads.data_ptr(),
                                       gz.data_ptr() if with_z0 else None, C.byref(stats), stream), h)
    icnf.last_stats = stats.as_dict()
    info = {"stats": icnf.last_stats, "steps": path_vjp_steps(icnf), "z0": zr.t(), "eps": er.t()}
    path = _path_rows(icnf, m, pth.permute(0, 2, 1), {"t": sv, "steps": info["steps"]})
    log2pi = np.float32(1.8378770664093453)
    path["logq"] = (-0.5 * ((zr * zr).sum(1) + n_in * log2pi))[None, :] + path["dlogp"]
    if with_z0 and pc is not None and path_cot.get("logq") is not None:
        # logq(tau_k) = logpdf(N(0, I), z0) + dlogp(tau_k): the first term's part of the cotangent, -(sum_k g_k) z0
        gz -= pc[:, :, n_in].sum(0)[:, None] * zr
    out = (xo.t(), lq, path, grads)
    return out + ((gz.t(), info) if with_z0 else (info,))


# ---------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _autograd_inference():
    import torch

    class _InferencePath(torch.autograd.Function):
        @staticmethod
        def forward(ctx, icnf, mode, xs, ps, eps, saveat):
            logpx, (E, n, A), path = inference_path(icnf, mode, xs.detach(), ps.detach(), None, saveat=saveat, eps=eps)
            ctx.icnf, ctx.mode, ctx.saveat = icnf, mode, saveat
            ctx.train = "E" in path
            # what the backward launch solves again: the same data, parameters and probes
            ctx.xs, ctx.ps, ctx.eps, ctx.ps_shape = xs.detach(), ps.detach().clone(), eps, ps.shape
            ctx.set_materialize_grads(False)
            outs = [logpx.clone(), E.clone(), n.clone(), A.clone(), path["z"].clone(), path["dlogp"].clone()]
            if ctx.train:
                outs += [path["E"].clone(), path["n"].clone()]
            return tuple(outs)

        @staticmethod
        def backward(ctx, g_logpx, g_E, g_n, g_A, g_z, g_dlogp, *g_more):
            icnf = ctx.icnf
            need_x, need_ps = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
            if not (need_x or need_ps):
                return (None,) * 6
            pc = {"z": g_z, "dlogp": g_dlogp}
            if ctx.train:
                pc["E"], pc["n"] = g_more
            res = inference_path_vjp(icnf, ctx.mode, ctx.xs, ctx.ps, None, saveat=ctx.saveat, cot=(g_logpx, (g_E, g_n, g_A)),
                                     path_cot=pc, eps=ctx.eps, with_x=bool(need_x))
            # (the backward launch's own outputs: compared with the forward's in the tests)
            icnf.last_backward_logpx, icnf.last_backward_path = res[0], res[2]
            return None, None, res[4] if need_x else None, res[3].reshape(ctx.ps_shape) if need_ps else None, None, None

    return _InferencePath


def differentiable_inference_path(icnf: ICNF, mode, xs, ps, st=None, *, saveat, eps=None):
    """``inference_path`` as a differentiable function of ``ps`` and, when it requires grad, ``xs``: returns ``(logpx, (E, n, A),
    path)`` attached to the autograd graph, ``path`` a dict with ``t``, ``z`` (K, n_in, B), ``dlogp`` (K, B) and in TrainMode
    ``E``, ``n`` (K, B).  The forward is the one-launch ``inference_path`` with the probes settled once; the backward is ONE
    ``inference_path_vjp`` launch with the same draws.  The backward launch solves again with the gradient form's tanh: its
    gradient is the exact discrete adjoint of the steps IT accepts, and DESIGN 4.4 says how its path compares with the forward's
    (``icnf.last_backward_path`` keeps it).  Refusals as ``inference_path_vjp``."""
    import torch
    who = "differentiable_inference_path"
    m = _mode_id(mode)
    _refuse(icnf, who, "differentiable_inference", xs, ps)
    sv = check_saveat(saveat, icnf.tspan)
    if not (xs.is_cuda and ps.is_cuda and (eps is None or (_is_torch(eps) and eps.is_cuda))):
        raise ValueError(f"{who}: torch tensors must live on the GPU")
    B = int(xs.shape[1])
    _check_batch(icnf, who, m, B)
    if m == _lib.MODE_TRAIN and eps is None:               # settled here, once, so that forward and backward are given the same
        eps = _probes(icnf, mode, True, xs.detach().to(torch.float32).t().contiguous(), None).t()
    outs = _autograd_inference().apply(icnf, mode, xs, ps, eps, sv)
    path = {"t": sv, "z": outs[4], "dlogp": outs[5]}
    if len(outs) > 6:
        path["E"], path["n"] = outs[6], outs[7]
    return outs[0], (outs[1], outs[2], outs[3]), path


@functools.lru_cache(maxsize=None)
def _autograd_generate():
    import torch

    class _GeneratePath(torch.autograd.Function):
        @staticmethod
        def forward(ctx, icnf, mode, ps, z0, eps, saveat):
            n = z0.shape[1]
            xs, logq, path = generate_path(icnf, mode, ps.detach(), None, n, saveat=saveat, z0=z0.detach(), eps=eps)
            ctx.icnf, ctx.mode, ctx.saveat = icnf, mode, saveat
            ctx.train = "E" in path
            ctx.ps, ctx.z0, ctx.eps, ctx.ps_shape = ps.detach().clone(), z0.detach(), eps, ps.shape
            ctx.set_materialize_grads(False)
            outs = [xs.clone(), logq.clone(), path["z"].clone(), path["logq"].clone()]
            if ctx.train:
                outs += [path["E"].clone(), path["n"].clone()]
            return tuple(outs)

        @staticmethod
        def backward(ctx, g_x, g_logq, g_z, g_lq, *g_more):
            icnf = ctx.icnf
            need_ps, need_z0 = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
            if not (need_ps or need_z0):
                return (None,) * 6
            if ctx.train and any(g is not None for g in g_more):
                raise NotImplementedError("differentiable_generate_path: E_path and n_path are not outputs of sampling (no cotangent)")
            res = generate_path_vjp(icnf, ctx.mode, ctx.ps, None, ctx.z0.shape[1], saveat=ctx.saveat,
                                    cot=(g_x, g_logq) if (g_x is not None or g_logq is not None) else None,
                                    path_cot={"z": g_z, "logq": g_lq}, z0=ctx.z0, eps=ctx.eps, with_z0=bool(need_z0))
            icnf.last_backward_xs, icnf.last_backward_logq, icnf.last_backward_path = res[0], res[1], res[2]
            return None, None, res[3].reshape(ctx.ps_shape) if need_ps else None, res[4].contiguous() if need_z0 else None, None, None

    return _GeneratePath


def differentiable_generate_path(icnf: ICNF, mode, ps, st=None, n: int = 1, *, saveat, z0=None, eps=None):
    """``generate_path`` as a differentiable function of ``ps`` and of a ``z0`` that requires grad: returns ``(xs, logq, path)``
    attached to the autograd graph, ``path`` a dict with ``t``, ``z`` (K, n_in, n), ``logq`` (K, n) and in TrainMode ``E``, ``n``
    (running integrals: they are not outputs of sampling and take no cotangent).  The forward is the one-launch
    ``generate_path`` with the draws kept; the backward is ONE ``generate_path_vjp`` launch.  As for
    ``differentiable_inference_path``, the backward launch solves again (``icnf.last_backward_path``)."""
    import torch
    who = "differentiable_generate_path"
    m = _mode_id(mode)
    _refuse(icnf, who, "differentiable_generate", ps)
    t0, t1 = icnf.tspan
    sv = check_saveat(saveat, (t1, t0))
    n = int(n)
    n_in = icnf.nvars + n_augment_input(icnf)
    for name, a in (("z0", z0), ("eps", eps)):
        if a is not None and (not _is_torch(a) or tuple(a.shape) != (n_in, n)):
            raise ValueError(f"{name} must be a device tensor (n_in = {n_in}, n = {n})")
    if not (ps.is_cuda and (z0 is None or z0.is_cuda) and (eps is None or eps.is_cuda)):
        raise ValueError(f"{who}: torch tensors must live on the GPU")
    _check_batch(icnf, who, m, n)
    zr, er, _ = _sampling_draws(icnf, mode, m == _lib.MODE_TRAIN, 1, n, n_in, ps.device,
                                z0.detach().unsqueeze(0) if z0 is not None else None,
                                eps.unsqueeze(0) if eps is not None else None, None, steer=False)
    if not (z0 is not None and z0.requires_grad):          # (a z0 that asks for a gradient stays the caller's tensor)
        z0 = zr[0].t()
    outs = _autograd_generate().apply(icnf, mode, ps, z0, er[0].t(), sv)
    path = {"t": sv, "z": outs[2], "logq": outs[3]}
    if len(outs) > 4:
        path["E"], path["n"] = outs[4], outs[5]
    return outs[0], outs[1], path
