"""Differentiable inference: the vector-Jacobian product of ``inference`` for any cotangent of its four outputs
(cnf_inference_record / cnf_inference_pullback), a ``torch.autograd.Function`` over it, and two ready-made losses that are
not means over the batch.

The reference lets a user differentiate any function of ``inference``'s outputs: ``ICNFModel(m, loss)`` takes the loss as a
hook (src/exts/mlj_ext/core_icnf.jl:1-29, used at :59-62), the model is a Lux layer (``icnf(xs, ps, st)``,
src/base_icnf.jl:528-543) and test/call_tests.jl:193-252 differentiates a closure.  Here that is one primitive: the discrete
adjoint of the recorded solve with per-sample cotangents.

Rows the model does not integrate carry no cotangent: with ``lambda1 = 0`` the E row is identically zero and its cotangent is
ignored, likewise ``lambda2`` / n and ``lambda3`` / A, and all three in TestMode.  Gradients are taken w.r.t. ``ps``, ``xs`` and,
for a conditional model, the conditioning inputs ``ys`` (cnf_set_grad_ys / cnf_grad_ys: ``ys = encoder(context)`` trains through
the flow) and, with a ``distributions.LearnableNormal`` base, its ``mean`` and scale (cnf_base_logpdf_pullback: the final state
does not depend on the base, so the cotangent of ``logpx`` is all it takes); ``eps`` and the time span are constants.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _lib
from .base_icnf import (ICNF, _is_torch, _mode_id, _solve_opts, _split_cond_args, _stream, _xs_colmajor, base_logpdf_pullback,
                        draw_eps, grad_result, grad_steps, grad_x, grad_ys, resolve_eps, set_grad_ys, steer_tspan, to_device)
from .distributions import LearnableNormal, learnable


def inference_record(icnf: ICNF, mode, xs, *args, eps=None, tspan=None):
    """``inference(icnf, mode, xs, [ys,] ps, st)`` with the solve recorded on the model's handle, for ``inference_pullback``.
    Returns ``(logpx, (E, n, A))`` exactly as ``inference`` does (device tensors for device inputs, numpy arrays for host
    inputs, which are staged through the device).  The record lasts until the next call on this model that solves, uploads
    parameters or conditioning, or changes the base distribution.  ``tspan``: the (steered) span to integrate over; drawn as
    ``inference`` draws it when not given -- after ``eps``, the order of ``loss_and_grad``."""
    host = not _is_torch(xs)
    ys, ps, st = _split_cond_args(icnf, args)
    m = _mode_id(mode)
    if host:
        xs, ys, eps = to_device(icnf, xs), to_device(icnf, ys), to_device(icnf, eps)
    xb = _xs_colmajor(icnf, xs)
    B = xb.B
    icnf.set_params(ps)
    icnf.set_cond(ys, B)
    eb = resolve_eps(icnf, m, eps, xb, B)
    if tspan is None:
        tspan = steer_tspan(icnf, mode)
    t = xb.torch
    buf = t.empty(4 * B, dtype=t.float32, device=xb.arr.device)
    logpx, regs = buf[:B], buf[B:]
    opts = _solve_opts(icnf, tuple(tspan))
    stats = _lib.cnf_solve_stats()
    l, h = _lib.lib(), icnf.handle()
    icnf._record = None
    _lib.check(l.cnf_inference_record(h, m, xb.ptr, eb.ptr if eb is not None else None, B, C.byref(opts), logpx.data_ptr(),
                                      regs.data_ptr(), C.byref(stats), _stream(xb)), h)
    icnf.last_stats = stats.as_dict()
    grad_steps(icnf)
    # (the library reads eps again in the pullback: the record keeps its buffers alive, and says whose record it is)
    icnf._record = {"xb": xb, "eb": eb, "B": B, "host": host, "tspan": tuple(tspan), "token": object()}
    r = regs.view(3, B)
    if host:
        return logpx.cpu().numpy(), tuple(a.cpu().numpy() for a in (r[0], r[1], r[2]))
    return logpx, (r[0], r[1], r[2])


def _cot_rows(cot):
    """``(g_logpx, (g_E, g_n, g_A))`` -- a bare None for the triple: no cotangent on the regularisers -- -> the four rows, as
    given (entries may be None); ``ValueError`` for a triple that is not three; None for anything that is not such a pair (the
    callers that take a bare ``4 x B`` array go on with it, the others refuse).  The one parse of this convention."""
    if not (isinstance(cot, (tuple, list)) and len(cot) == 2 and (cot[1] is None or isinstance(cot[1], (tuple, list)))):
        return None
    rows = [cot[0]] + list(cot[1] if cot[1] is not None else (None, None, None))
    if len(rows) != 4:
        raise ValueError("cot must be (g_logpx, (g_E, g_n, g_A))")
    return rows


def _cot_matrix(cot, B, device):
    """(g_logpx, (g_E, g_n, g_A)) or a 4 x B array -> one contiguous 4 x B float32 device tensor; None entries are zeros."""
    import torch
    rows = _cot_rows(cot)
    out = torch.zeros(4, B, dtype=torch.float32, device=device)
    if rows is None:
        c = cot if _is_torch(cot) else torch.from_numpy(np.asarray(cot, dtype=np.float32))
        if tuple(c.shape) != (4, B):
            raise ValueError(f"cot must be 4 x {B}")
        out.copy_(c.detach().to(device=device, dtype=torch.float32))
        return out
    for i, r in enumerate(rows):
        if r is None:
            continue
        r = r if _is_torch(r) else torch.from_numpy(np.asarray(r, dtype=np.float32))
        if r.numel() != B:
            raise ValueError("every cotangent row needs one entry per sample")
        out[i].copy_(r.detach().reshape(-1).to(device=device, dtype=torch.float32))
    return out


def inference_pullback(icnf: ICNF, cot, with_x=False, with_ys=False, with_base=False):
    """``sum_b sum_r cot[r][b] d out_r[b] / d ps`` (and ``/ d xs`` with ``with_x``, ``/ d ys`` -- ``n_cond x B``, conditional
    models only -- with ``with_ys``, and the pair ``(/ d mean, / d scale)`` of a ``LearnableNormal`` base with ``with_base``,
    appended in that order) through the steps ``inference_record`` recorded, in the caller's parameter layout.  ``cot``:
    ``(g_logpx, (g_E, g_n, g_A))`` or a ``4 x B`` array; ``None`` entries are zeros.  May be called several times on one
    record.  ``CNFError`` (``ERR_BAD_ARG``) when the record is gone; ``ValueError`` for ``with_base`` with any other base."""
    import torch
    if with_base:
        learnable(icnf.basedist)
    l, h = _lib.lib(), icnf.handle()
    rec = getattr(icnf, "_record", None)
    dev = rec["xb"].arr.device if rec is not None else torch.device("cuda", icnf.device)
    host = rec["host"] if rec is not None else False
    # (B is the cotangent's: the library refuses one that does not match the record)
    rows = _cot_rows(cot)
    if rows is not None:
        sizes = {int(r.numel()) if _is_torch(r) else int(np.size(r)) for r in rows if r is not None}
        if len(sizes) > 1:
            raise ValueError("every cotangent row needs one entry per sample")
        B = sizes.pop() if sizes else (rec["B"] if rec is not None else 0)
    else:
        B = int(cot.shape[1])
    if B < 1:
        raise ValueError("empty cotangent")
    cm = _cot_matrix(cot, B, dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    grad = torch.empty(icnf.nn.n_params_internal, dtype=torch.float32, device=dev)
    set_grad_ys(icnf, with_ys)
    _lib.check(l.cnf_inference_pullback(h, cm.data_ptr(), B, grad.data_ptr(), stream), h)
    grad = icnf.nn.grad_to_external(grad)
    return grad_result((grad,), host,
                       (with_x, grad_x(icnf, B, dev, stream, host) if with_x else None),
                       (with_ys, grad_ys(icnf, B, dev, stream, host) if with_ys else None),
                       (with_base, base_logpdf_pullback(icnf, cm[0]) if with_base else None))      # (row 0: the cotangent of logpx)


@functools.lru_cache(maxsize=None)
def _autograd_function():
    import torch

    class _Inference(torch.autograd.Function):
        @staticmethod
        def forward(ctx, icnf, mode, xs, ys, ps, eps, tspan, base_mean, base_scale):
            # (base_mean / base_scale: the tensors of a LearnableNormal base, here only so that autograd routes their gradient;
            # their values were uploaded by the record's set_params)
            if _is_torch(ys) and ys.requires_grad:   # (a ys that asks for nothing stays the caller's object: set_cond knows it)
                ys = ys.detach()
            args = (ys, ps, None) if icnf.cond else (ps, None)
            logpx, (E, n, A) = inference_record(icnf, mode, xs.detach(), *args, eps=eps, tspan=tspan)
            rec = icnf._record
            ctx.icnf, ctx.mode, ctx.token = icnf, mode, rec["token"]
            # what a second recording needs: the solve is deterministic, so the same inputs give the same record bit for bit
            ctx.xs, ctx.ys, ctx.ps, ctx.eb, ctx.tspan = xs.detach(), ys, ps.detach(), rec["eb"], rec["tspan"]
            ctx.ys_shape = None if ys is None else ys.shape
            ctx.ps_shape = ps.shape
            ctx.base_key = _base_key(icnf)
            ctx.set_materialize_grads(False)
            return logpx.clone(), E.clone(), n.clone(), A.clone()

        @staticmethod
        def backward(ctx, g_logpx, g_E, g_n, g_A):
            icnf = ctx.icnf
            cot = (g_logpx, (g_E, g_n, g_A))

            def record_again():
                args = (ctx.ys, ctx.ps, None) if icnf.cond else (ctx.ps, None)
                eps = ctx.eb.view() if ctx.eb is not None else None
                inference_record(icnf, ctx.mode, ctx.xs, *args, eps=eps, tspan=ctx.tspan)

            # d / d ys is asked of the library only when whatever produced ys wants it (also after record_again)
            need_ys = bool(ctx.needs_input_grad[3])
            need_base = bool(ctx.needs_input_grad[7] or ctx.needs_input_grad[8])
            res = _pull_recorded(icnf, ctx, record_again,
                                 lambda: inference_pullback(icnf, cot, with_x=True, with_ys=need_ys, with_base=need_base))
            grad, gx = res[0], res[1]
            gy = res[2].reshape(ctx.ys_shape).contiguous() if need_ys else None
            gm, gs = _base_grads(icnf, res[-1], ctx.needs_input_grad[7], ctx.needs_input_grad[8]) if need_base else (None, None)
            need_x, need_ps = ctx.needs_input_grad[2], ctx.needs_input_grad[4]
            return (None, None, gx.contiguous() if need_x else None, gy,
                    grad.reshape(ctx.ps_shape) if need_ps else None, None, None, gm, gs)

    return _Inference


def _pull_recorded(icnf: ICNF, ctx, record_again, pull):
    """``pull()`` on the record ``ctx.token`` names -- what both autograd functions' ``backward`` do.  A record another call on
    the model has displaced (its token is gone, or the library refuses the pullback with ``ERR_BAD_ARG``) is made again from
    the saved inputs first, with the base's values checked to be those of the first recording, and pulled once more."""
    def again():
        _base_unchanged(icnf, ctx.base_key)
        record_again()
        ctx.token = icnf._record["token"]

    rec = getattr(icnf, "_record", None)
    if rec is None or rec["token"] is not ctx.token:
        again()
    try:
        return pull()
    except _lib.CNFError as e:          # the record was displaced by another call on the handle: record again
        if e.status != _lib.ERR_BAD_ARG:
            raise
        again()
        return pull()


def _base_grads(icnf: ICNF, pair, need_mean, need_scale):
    """(g_mean, g_scale) of a pullback as the gradients of the base's own tensors: their device, dtype and shape."""
    d = icnf.basedist
    like = lambda g, t: g.to(device=t.device, dtype=t.dtype).reshape(t.shape)
    return (like(pair[0], d.mean_t) if need_mean else None, like(pair[1], d.scale_t) if need_scale else None)


def _base_key(icnf: ICNF):
    """Which values of a LearnableNormal base a record was made with: (the object, its generation); None for any other base."""
    d = icnf.basedist
    return (d, d.generation) if isinstance(d, LearnableNormal) else None


def _base_unchanged(icnf: ICNF, key):
    """Before a displaced record is made again from saved inputs: the base's values are not among them, so they must still be
    the ones of the first recording -- a second recording with another base would silently differentiate another function."""
    d = icnf.basedist
    if isinstance(d, LearnableNormal):
        d.refresh()
    cur = _base_key(icnf)
    if (cur is None) != (key is None) or (cur is not None and (cur[0] is not key[0] or cur[1] != key[1])):
        raise RuntimeError("the base distribution changed between forward and backward and the recorded solve was displaced by "
                           "another call on the model: call backward before updating the base")


def _base_tensors(icnf: ICNF):
    """The tensors of a LearnableNormal base when either requires grad (what the autograd functions take), else (None, None)."""
    d = icnf.basedist
    if isinstance(d, LearnableNormal) and d.requires_grad:
        return d.mean_t, d.scale_t
    return None, None


def differentiable_inference(icnf: ICNF, mode, xs, *args, eps=None):
    """``inference`` as a differentiable function of ``ps``, ``xs``, (conditional models) ``ys`` and the ``mean`` / scale tensors
    of a ``LearnableNormal`` base when either requires grad (device tensors): forward
    = ``inference_record``, backward = ``inference_pullback`` (which is asked for d / d ys only when ``ys`` requires grad).  Returns ``(logpx, (E, n, A))`` attached to the autograd graph.  If another call on the
    model displaced the record before ``backward``, the solve is recorded again from the saved inputs (same outputs bit for
    bit: the solve is deterministic) and then pulled back; the values of a ``LearnableNormal`` base are not saved, so
    ``RuntimeError`` if they changed in between."""
    import torch
    if not _is_torch(xs):
        raise ValueError("differentiable_inference needs device tensors")
    ys, ps, st = _split_cond_args(icnf, args)
    ps = ps if _is_torch(ps) else to_device(icnf, ps, xs.device)
    # eps first and then the steered t1: the order in which loss_and_grad draws, so that one seed gives one problem
    m = _mode_id(mode)
    if m == _lib.MODE_TRAIN and eps is None:
        eps = draw_eps(icnf, _xs_colmajor(icnf, xs.detach()), xs.shape[1]).view()
    tspan = steer_tspan(icnf, mode)
    logpx, E, n, A = _autograd_function().apply(icnf, mode, xs, ys, ps, eps, tspan, *_base_tensors(icnf))
    return logpx, (E, n, A)


def _lambdas(icnf: ICNF, mode):
    if _mode_id(mode) != _lib.MODE_TRAIN:
        return 0.0, 0.0, 0.0
    return icnf.lambda1, icnf.lambda2, icnf.lambda3


def weighted_loss(weights):
    """A loss for ``ICNFModel.loss``: ``sum_b w_b (-logpx_b + l1 E_b + l2 n_b + l3 A_b) / sum_b w_b`` with one weight per
    sample of the batch it is called on (a tensor, an array, or a callable ``weights(xs) -> B`` weights)."""
    def _loss(icnf, mode, xs, *args):
        import torch
        logpx, (E, n, A) = differentiable_inference(icnf, mode, xs, *args)
        w = weights(xs) if callable(weights) else weights
        w = w if _is_torch(w) else torch.from_numpy(np.asarray(w, dtype=np.float32))
        w = w.to(device=logpx.device, dtype=logpx.dtype).reshape(-1)
        l1, l2, l3 = _lambdas(icnf, mode)
        return (w * (-logpx + l1 * E + l2 * n + l3 * A)).sum() / w.sum()
    return _loss


def tempered_loss(beta):
    """A loss for ``ICNFModel.loss``: ``-(logsumexp_b(beta logpx_b) - log B) / beta + mean_b(l1 E_b + l2 n_b + l3 A_b)``: the
    tempered (power) mean of the likelihoods in place of their geometric mean (``beta -> 0`` gives the built-in loss)."""
    beta = float(beta)
    if beta == 0.0:
        raise ValueError("beta must be non-zero")

    def _loss(icnf, mode, xs, *args):
        import math
        import torch
        logpx, (E, n, A) = differentiable_inference(icnf, mode, xs, *args)
        l1, l2, l3 = _lambdas(icnf, mode)
        nll = -(torch.logsumexp(beta * logpx, 0) - math.log(logpx.numel())) / beta
        return nll + (l1 * E + l2 * n + l3 * A).mean()
    return _loss
