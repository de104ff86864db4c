"""Differentiable sampling: ``generate`` with the log-density of the sample from the one solve, the vector-Jacobian product of
``(xs, logq)`` for any cotangent (cnf_generate_record / cnf_generate_pullback), a ``torch.autograd.Function`` over it and one
ready-made loss on samples, the reverse KL divergence.  For users of a normalizing-flow library this is ``rsample`` +
``log_prob``; ``vjp.py`` is the density direction.

``generate`` integrates the augmented state over ``reverse(tspan)`` from ``u0 = [z0; 0]`` (src/base_icnf.jl:358-380) and keeps
rows 1..nvars (:202-211).  The dlogp row of that same solve gives the density of what it produced:

    logq = logpdf(basedist, z0) + dlogp_end                  (sign +; ``inference`` has logpz - dlogp)

With ``naugmented > 0``, ``logq`` is the density of the whole ``n_in``-dimensional final state (``icnf._record["z"]``), the
counterpart of what ``inference`` scores, not the marginal of its first ``nvars`` rows.  In TestMode it is exact; in TrainMode
it is the Hutchinson estimate for the ``eps`` used.  Gradients are taken w.r.t. ``ps``, the base draw ``z0`` and, for a
conditional model, ``ys``; ``eps`` and the time span are constants, and the accepted step sizes are constants of the discrete
adjoint, as everywhere in this package.

With a ``distributions.LearnableNormal`` base the gradient also reaches its ``mean`` and scale.  ``generate_pullback`` returns
the partial derivative at FIXED ``z0`` (``g_logq d logpdf(base, z0) / d base``, cnf_base_logpdf_pullback); when
``differentiable_generate`` drew ``z0 = mean + L n`` itself it keeps the normals ``n`` and adds the pullback of that draw applied
to ``grad_z0`` (cnf_base_sample_pullback), which is the total derivative.  A ``z0`` the caller passes is a leaf: the base gets
the fixed-``z0`` partial only.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _lib
from .base_icnf import (ICNF, _generate_inputs, _is_torch, _mode_id, _solve_opts, _stream, base_logpdf_pullback,
                        base_sample_pullback, grad_result, grad_steps, grad_ys, n_augment_input, raise_if_no_gpu, set_grad_ys,
                        steer_tspan, to_device)
from .distributions import learnable
from .vjp import _base_grads, _base_key, _base_tensors, _pull_recorded


def _device(icnf: ICNF):
    import torch
    raise_if_no_gpu()
    return torch.device("cuda", icnf.device)


def generate_record(icnf: ICNF, mode, ps, st=None, n: int = 1, *, ys=None, z0=None, eps=None, tspan=None):
    """``generate(icnf, mode, ps, st, n)`` with the log-density of every sample and the solve recorded on the model's handle,
    for ``generate_pullback``.  Returns ``(xs [nvars x n], logq [n])``: device tensors when the inputs live on the device (a
    ``HIPRNG`` or a device ``z0``), numpy arrays otherwise (host draws are staged through the device).  ``z0`` / ``eps`` are
    drawn as ``generate_prob`` draws them when not given; ``tspan``: the model's (steered) span -- it is integrated in reverse.
    The full ``n_in x n`` final state is ``icnf._record["z"]``.  The record lasts until the next call on this model that
    solves, uploads parameters or conditioning, or changes the base distribution."""
    import torch
    m = _mode_id(mode)
    n_in = icnf.nvars + n_augment_input(icnf)
    zb, eb = _generate_inputs(icnf, mode, ps, n, ys, z0, eps)
    if eb.B != n:
        raise ValueError("eps must have one column per sample")
    host = zb.torch is None
    zb, eb = to_device(icnf, zb), to_device(icnf, eb)
    if tspan is None:
        tspan = steer_tspan(icnf, mode)
    t0, t1 = tspan
    dev = zb.arr.device
    out = torch.empty(n * n_in + n, dtype=torch.float32, device=dev)
    z, logq = out[:n * n_in], out[n * n_in:]
    opts = _solve_opts(icnf, (t1, t0))                     # reverse(tspan)
    stats = _lib.cnf_solve_stats()
    l, h = _lib.lib(), icnf.handle()
    icnf._record = None
    _lib.check(l.cnf_generate_record(h, m, zb.ptr, eb.ptr if m == _lib.MODE_TRAIN else None, n, C.byref(opts), z.data_ptr(),
                                     logq.data_ptr(), C.byref(stats), _stream(zb)), h)
    icnf.last_stats = stats.as_dict()
    grad_steps(icnf)
    zfull = z.view(n, n_in).t()
    # ("xb": the buffer the density direction's pullback looks its device up in -- the library then refuses the wrong kind)
    icnf._record = {"kind": "generate", "xb": zb, "zb": zb, "eb": eb, "B": n, "host": host, "tspan": tuple(tspan), "z": zfull,
                    "token": object()}
    xs = zfull[:icnf.nvars]
    if host:
        return xs.cpu().numpy(), logq.cpu().numpy()
    return xs, logq


def _cot_two(cot):
    """``(g_x, g_logq)`` -> the two entries as given (either may be None); ``ValueError`` for anything that is not such a pair.
    The one check of this convention: what the entries may be is the caller's (host arrays here, device tensors only in
    ``ensemble._cot_pair_many``)."""
    if not isinstance(cot, (tuple, list)) or len(cot) != 2:
        raise ValueError("cot must be (g_x, g_logq)")
    return cot[0], cot[1]


def _cot_pair(icnf: ICNF, cot, dev):
    """(g_x, g_logq) -> (cot_z [B][n_in] or None, cot_logq [B] or None, B); rows of g_x beyond those given are zero."""
    import torch
    gx, gl = _cot_two(cot)
    n_in = icnf.nvars + n_augment_input(icnf)
    t = lambda a: (a if _is_torch(a) else torch.from_numpy(np.asarray(a, dtype=np.float32))).detach().to(device=dev, dtype=torch.float32)
    cz = cl = None
    sizes = set()
    if gx is not None:
        gx = t(gx)
        if gx.dim() != 2 or gx.shape[0] not in (icnf.nvars, n_in):
            raise ValueError(f"g_x must be {icnf.nvars} x n or {n_in} x n")
        sizes.add(int(gx.shape[1]))
    if gl is not None:
        cl = t(gl).reshape(-1).contiguous()
        sizes.add(int(cl.numel()))
    if len(sizes) > 1:
        raise ValueError("g_x and g_logq need one column / entry per sample")
    B = sizes.pop() if sizes else 0
    if gx is not None:
        cz = torch.zeros(B, n_in, dtype=torch.float32, device=dev)
        cz[:, :gx.shape[0]] = gx.t()
    return cz, cl, B


def generate_pullback(icnf: ICNF, cot, with_z0=False, with_ys=False, with_base=False):
    """``sum_b (<g_x[:, b], d xs_b / d ps> + g_logq[b] d logq_b / d ps)`` through the steps ``generate_record`` recorded, in the
    caller's parameter layout; with ``with_z0`` the same w.r.t. the base draw (``n_in x n``), with ``with_ys`` w.r.t. the
    conditioning inputs (``n_cond x n``), with ``with_base`` the pair ``(/ d mean, / d scale)`` of a ``LearnableNormal`` base AT
    FIXED ``z0`` (the pullback of the draw itself is ``base_sample_pullback`` of the ``with_z0`` result), appended in that
    order.  ``cot = (g_x, g_logq)``: ``g_x`` is ``nvars x n`` or ``n_in x n`` (rows beyond ``nvars`` are zero when not given),
    ``None`` entries are zeros (not both).  May be called several times on one record.  ``CNFError`` (``ERR_BAD_ARG``) when the
    record is gone or is not a sampling record; ``ValueError`` for ``with_base`` with any other base."""
    import torch
    if with_base:
        learnable(icnf.basedist)
    l, h = _lib.lib(), icnf.handle()
    rec = getattr(icnf, "_record", None)
    dev = rec["xb"].arr.device if rec is not None else _device(icnf)
    host = rec["host"] if rec is not None else False
    cz, cl, B = _cot_pair(icnf, cot, dev)            # (B is the cotangent's: the library refuses one that does not match the record)
    if cz is None and cl is None:
        B = rec["B"] if rec is not None else 1       # (the library refuses two null cotangents)
    n_in = icnf.nvars + n_augment_input(icnf)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    grad = torch.empty(icnf.nn.n_params_internal, dtype=torch.float32, device=dev)
    gz0 = torch.empty(B * n_in, dtype=torch.float32, device=dev) if with_z0 else None
    set_grad_ys(icnf, with_ys)
    _lib.check(l.cnf_generate_pullback(h, cz.data_ptr() if cz is not None else None, cl.data_ptr() if cl is not None else None, B,
                                       grad.data_ptr(), gz0.data_ptr() if with_z0 else None, stream), h)
    grad = icnf.nn.grad_to_external(grad)
    if with_z0:
        gz0 = gz0.view(B, n_in).t()
    gy = grad_ys(icnf, B, dev, stream, host) if with_ys else None
    gb = None
    if with_base:                                    # (only logq depends on the base at fixed z0)
        gb = base_logpdf_pullback(icnf, cl if cl is not None else torch.zeros(B, dtype=torch.float32, device=dev))
    return grad_result((grad,), host, (with_z0, gz0), (with_ys, gy), (with_base, gb))


@functools.lru_cache(maxsize=None)
def _autograd_function():
    import torch

    class _Generate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, icnf, mode, ps, ys, z0, eps, tspan, normals, base_mean, base_scale):
            # (base_mean / base_scale: the tensors of a LearnableNormal base, here so that autograd routes their gradient;
            # normals: what z0 = mean + L n was drawn from inside differentiable_generate, None for a caller's z0)
            if _is_torch(ys) and ys.requires_grad:   # (a ys that asks for nothing stays the caller's object: set_cond knows it)
                ys = ys.detach()
            n = z0.shape[1]
            xs, logq = generate_record(icnf, mode, ps, None, n, ys=ys, z0=z0.detach(), eps=eps, tspan=tspan)
            rec = icnf._record
            ctx.icnf, ctx.mode, ctx.token = icnf, mode, rec["token"]
            # what a second recording needs: the solve is deterministic, so the same inputs give the same record bit for bit
            ctx.ps, ctx.ys, ctx.z0, ctx.eps, ctx.tspan = ps.detach(), ys, z0.detach(), eps, rec["tspan"]
            ctx.ys_shape = None if ys is None else ys.shape
            ctx.ps_shape = ps.shape
            ctx.normals = normals
            ctx.base_key = _base_key(icnf)
            ctx.set_materialize_grads(False)
            return xs.clone(), logq.clone()

        @staticmethod
        def backward(ctx, g_x, g_logq):
            icnf = ctx.icnf
            need_ps, need_ys, need_z0 = ctx.needs_input_grad[2], bool(ctx.needs_input_grad[3]), ctx.needs_input_grad[4]
            need_base = bool(ctx.needs_input_grad[8] or ctx.needs_input_grad[9])
            if g_x is None and g_logq is None:
                return (None,) * 10

            def record_again():
                generate_record(icnf, ctx.mode, ctx.ps, None, ctx.z0.shape[1], ys=ctx.ys, z0=ctx.z0, eps=ctx.eps, tspan=ctx.tspan)

            res = _pull_recorded(icnf, ctx, record_again,
                                 lambda: generate_pullback(icnf, (g_x, g_logq), with_z0=True, with_ys=need_ys, with_base=need_base))
            grad, gz0 = res[0], res[1]
            gy = res[2].reshape(ctx.ys_shape).contiguous() if need_ys else None
            gm = gs = None
            if need_base:
                pm, psc = res[-1]                    # the partial at fixed z0 ...
                if ctx.normals is not None:          # ... and the chain through z0 = mean + L n: the pullback of the draw
                    sm, ssc = base_sample_pullback(icnf, ctx.normals, gz0)
                    pm, psc = pm + sm, psc + ssc
                gm, gs = _base_grads(icnf, (pm, psc), ctx.needs_input_grad[8], ctx.needs_input_grad[9])
            return (None, None, grad.reshape(ctx.ps_shape) if need_ps else None, gy, gz0.contiguous() if need_z0 else None,
                    None, None, None, gm, gs)

    return _Generate


def differentiable_generate(icnf: ICNF, mode, ps, st=None, n: int = 1, *, ys=None, z0=None, eps=None):
    """``generate`` with ``logq`` as a differentiable function of ``ps``, of ``z0`` when it requires grad (``z0 = g(context)``:
    amortised inference), for a conditional model of ``ys`` when it requires grad, and of the ``mean`` / scale tensors of a
    ``LearnableNormal`` base when either requires grad (through the draw ``z0 = mean + L n`` too when ``z0`` is drawn here):
    forward = ``generate_record``, backward = ``generate_pullback``.  Returns ``(xs [nvars x n], logq [n])`` attached to the
    autograd graph (device tensors).  ``z0`` and ``eps`` are drawn as ``generate`` draws them when not given.  If another call on the model displaced the record before
    ``backward``, the solve is recorded again from the saved inputs (same outputs bit for bit) and then pulled back; the values
    of a ``LearnableNormal`` base are not saved, so ``RuntimeError`` if they changed in between."""
    import torch
    m = _mode_id(mode)
    dev = _device(icnf)
    ps = ps if _is_torch(ps) else to_device(icnf, ps, dev)
    if _is_torch(z0) and z0.shape[1] != n:
        raise ValueError("z0 must have n columns")
    bmean, bscale = _base_tensors(icnf)
    kept = []
    # the draws, in the order of generate_prob (z0, eps, the steered span), so that one seed gives one problem; the standard
    # normals a z0 drawn here was made from are kept for the pullback of the draw
    zb, eb = _generate_inputs(icnf, mode, ps, n, ys.detach() if _is_torch(ys) and ys.requires_grad else ys,
                              z0.detach() if _is_torch(z0) else z0, eps, normals_out=kept)
    n_in = icnf.nvars + n_augment_input(icnf)
    normals = kept[0].view(n, n_in).t() if kept and bmean is not None else None
    tspan = steer_tspan(icnf, mode)
    if not (_is_torch(z0) and z0.requires_grad):
        z0 = to_device(icnf, zb).view()
    eps = to_device(icnf, eb).view() if m == _lib.MODE_TRAIN else None
    return _autograd_function().apply(icnf, mode, ps, ys, z0, eps, tspan, normals, bmean, bscale)


def reverse_kl(icnf: ICNF, mode, ps, st, n, target_logpdf, **kw):
    """The reverse Kullback-Leibler divergence to an unnormalised target, estimated on ``n`` samples of the flow:
    ``mean(logq - target_logpdf(xs))`` with ``(xs, logq) = differentiable_generate(icnf, mode, ps, st, n)`` -- the variational
    objective, differentiable w.r.t. ``ps`` (and ``z0`` / ``ys`` given through ``kw``, and the tensors of a ``LearnableNormal`` base).  ``target_logpdf``: a torch callable,
    ``nvars x n`` samples -> ``n`` log-densities."""
    xs, logq = differentiable_generate(icnf, mode, ps, st, n, **kw)
    return (logq - target_logpdf(xs).reshape(-1)).mean()
