"""Ensemble forward-mode: ``inference_jvp`` / ``generate_jvp`` / ``loss_jvp`` of M members at once (cnf_inference_jvp_many /
cnf_generate_jvp_many, include/cnfhip_ensemble_jvp.h) -- ``jvp.py`` with a member axis, on the call skeleton of ``ensemble.py``.

A single tangent call at the reference's training batch of 32 is two waves on the whole device: its cost is launch and
latency.  The workloads that take tangents of many small models -- a directional derivative of M folds' losses along each
fold's optimiser update (a line search), ``J v`` per replica for Gauss-Newton / Fisher products, the reference's forward-mode
gradient (``AutoEnzyme(mode = Forward)``, test/call_tests.jl) for M seeds -- are here TWO launches whatever M: the plain ensemble
solve, which keeps every member's step attempts on the device, and the ensemble form of the tangent kernel right behind it, one
wave per (16-column tile, direction, member), with no host wait in between.

Envelope: what ``inference_many`` and ``inference_jvp`` both take; ``counts``, ``reltol`` / ``abstol`` (and, for the loss,
``lambdas``) make the members heterogeneous as everywhere in ``ensemble.py``.  No ``bases=``, no conditional members, no paths.
Everything else raises ``NotImplementedError`` before anything is drawn or a handle is made.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import ensemble as _ens
from . import jvp as _jvp
from .base_icnf import ICNF, _is_torch, _mode_id, _solve_opts, n_augment_input


def _refuse(icnf: ICNF, who, bases, *tensors):
    """The refusals of these calls.  Host logic only: nothing is drawn, no handle is made."""
    why = _ens._refusal(icnf) or _jvp._refusal(icnf)
    if why is not None:
        raise NotImplementedError(f"{who}: " + why)
    if bases is not None:
        raise NotImplementedError(f"{who}: the tangent calls take no bases (a base per member: one member at a time on member_twin)")
    if not all(t is None or _is_torch(t) for t in tensors):
        raise NotImplementedError(f"{who} takes device tensors (host arrays: the single-model call, one member at a time)")


def _check_directions(d_ps, d_x, M, n_params, rows, B, x_name):
    """The shapes of the members' directions: ``d_ps`` (M, n_params) or (M, R, n_params), ``d_x`` (M, rows, B) or
    (M, R, rows, B); at least one, the same R and the same stacking for both.  -> (R, single).  Host logic only."""
    if d_ps is None and d_x is None:
        raise ValueError(f"give a direction: d_ps, {x_name} or both")
    R, single = None, None
    for d, one_dim, shape, name in ((d_ps, 2, (n_params,), "d_ps"), (d_x, 3, (rows, B), x_name)):
        if d is None:
            continue
        want = f"{name} must be (M = {M},) + {shape} or (M = {M}, R) + {shape}, got {tuple(d.shape)}"
        if d.dim() not in (one_dim, one_dim + 1) or d.shape[0] != M:
            raise ValueError(want)
        s = d.dim() == one_dim
        if tuple(d.shape[(1 if s else 2):]) != shape or (not s and d.shape[1] < 1):
            raise ValueError(want)
        r = 1 if s else int(d.shape[1])
        if R is not None and (r != R or s != single):
            raise ValueError(f"d_ps and {x_name} must carry the same number of directions")
        R, single = r, s
    return R, single


def _place_directions(d_ps, d_x, single, dev):
    """-> (dp [M][R][n_params] | None, dx [M][R][B][rows] | None): float32, contiguous, on ``dev``."""
    import torch

    def put(d):
        d = d.detach().to(device=dev, dtype=torch.float32)
        return d.unsqueeze(1) if single else d

    dp = put(d_ps).contiguous() if d_ps is not None else None
    dx = put(d_x).permute(0, 1, 3, 2).contiguous() if d_x is not None else None
    return dp, dx


def ensemble_jvp_steps(icnf: ICNF, member: int):
    """``(t_n, h_n)`` of the steps ``member`` accepted in the last ``inference_jvp_many`` / ``generate_jvp_many`` CALL on this
    model (cnf_ensemble_jvp_steps; the index counts within that call): two float32 vectors, or ``None`` when there is none."""
    read, h = _lib.lib().cnf_ensemble_jvp_steps, icnf.handle()
    n = read(h, int(member), None, None, 0)
    if n < 0:
        return None
    t, hs = np.empty(max(n, 1), dtype=np.float32), np.empty(max(n, 1), dtype=np.float32)
    read(h, int(member), t.ctypes.data, hs.ctypes.data, n)
    return t[:n], hs[:n]


def _blocks(R):
    """The direction blocks of a call: at most ``_lib.JVP_MAX_R`` each (the grid's second axis), as in ``jvp._run``."""
    return [(r0, min(R, r0 + _lib.JVP_MAX_R)) for r0 in range(0, R, _lib.JVP_MAX_R)]


def _block(t, r0, r1, R):
    """Directions ``r0 .. r1 - 1`` of an [M][R][...] tensor as the C ABI reads them (the tensor itself when that is all of them)."""
    if t is None or (r0 == 0 and r1 == R):
        return t
    return t[:, r0:r1].contiguous()


def _member_dirs(d, i, k, single):
    """Member i's directions for the single-model call that runs it again: [R][k][rows] -> (R, rows, k), or (rows, k)."""
    if d is None:
        return None
    d = d[i] if d.dim() == 3 else d[i, :, :k].permute(0, 2, 1)
    return d[0] if single else d


def _alone_cap(trace_cap):
    """``trace_cap`` of the single-model call that runs a member again: that call's own default (4096 attempts), or the caller's
    when it is larger -- a member is also run again BECAUSE it made more attempts than the ensemble launch kept rows for."""
    return int(trace_cap) if int(trace_cap) > 4096 else 0


def loss_jvp_reduce(mode, primal, tangent, counts, lambdas):
    """The reduction of ``loss_jvp_many``: ``primal = (logpx, (E, n, A))`` each (M, B), ``tangent`` shaped like it with an ``R``
    axis behind ``M`` when stacked; ``counts`` (M,) integers and ``lambdas`` (M, 3).  Member m's loss and its derivative are the
    means over its first ``counts[m]`` columns of ``-logpx + l1 E + l2 n + l3 A`` with its own lambdas (``-logpx`` in TestMode) --
    the arithmetic of ``loss_jvp`` on the member's own columns.  -> (losses (M,) float32 numpy, d_losses (M,) or (M, R))."""
    import torch
    (logpx, (E, nn, A)), (dl, (dE, dn, dA)) = primal, tangent
    train = _mode_id(mode) == _lib.MODE_TRAIN
    M, B = logpx.shape
    counts = np.asarray(counts).reshape(-1)
    if train:
        lam = torch.as_tensor(np.array(lambdas, dtype=np.float32), device=logpx.device)
        l = lam.view(M, 3, 1)
        lt = l if dl.dim() == 2 else l.unsqueeze(-1)
        val = -logpx + l[:, 0] * E + l[:, 1] * nn + l[:, 2] * A
        tan = -dl + lt[:, 0] * dE + lt[:, 1] * dn + lt[:, 2] * dA
    else:
        val, tan = -logpx, -dl
    if (counts == B).all():
        losses, d = val.mean(dim=-1), tan.mean(dim=-1)
    else:                                                  # (ragged members: each mean over the member's own columns)
        losses = torch.stack([val[m, :int(k)].mean() for m, k in enumerate(counts)])
        d = torch.stack([tan[m, ..., :int(k)].mean(dim=-1) for m, k in enumerate(counts)])
    return losses.cpu().numpy(), d


def _inference_jvp_many(icnf, who, mode, xs, ps, st, d_ps, d_xs, eps, t1, counts, lambdas, reltol, abstol, trace_cap, bases):
    import torch
    _refuse(icnf, who, bases, xs, ps, d_ps, d_xs, eps)
    n_params = icnf.nn.n_params_internal
    shape = {}

    def dirs(M, B):
        shape["R"], shape["single"] = _check_directions(d_ps, d_xs, M, n_params, icnf.nvars, B, "d_xs")
        return tuple(d for d in (d_ps, d_xs) if d is not None)

    s = _ens._settle_density(icnf, mode, xs, ps, eps, t1, who, "inference_jvp", "cnf_ensemble_eval_capacity", cot_rows=dirs,
                             members=dict(counts=counts, lambdas=lambdas, reltol=reltol, abstol=abstol))
    l, h = _lib.lib(), icnf.handle()
    m, M, B, dev, xr, pr, er, t1 = s.m, s.M, s.B, s.dev, s.xr, s.pr, s.er, s.t1
    R, single = shape["R"], shape["single"]
    dp, dx = _place_directions(d_ps, d_xs, single, dev)
    opts = _solve_opts(icnf, icnf.tspan)
    logpx, regs = _ens._values(s.het, (M, B), dev), _ens._values(s.het, (M, 3, B), dev)
    dout = torch.empty((M, R, 4, B), dtype=torch.float32, device=dev)
    losses = np.empty(M, dtype=np.float32)
    info, calls = None, 0
    for r0, r1 in _blocks(R):
        dpb, dxb = _block(dp, r0, r1, R), _block(dx, r0, r1, R)
        db = dout if (r0 == 0 and r1 == R) else torch.empty((M, r1 - r0, 4, B), dtype=torch.float32, device=dev)
        info, steps = _ens._launch(icnf, s, B, lambda lo, n, status, stats: l.cnf_inference_jvp_many(
            h, m, n, pr[lo].data_ptr(), xr[lo].data_ptr(), er[lo].data_ptr() if er is not None else None, B,
            dpb[lo].data_ptr() if dpb is not None else None, dxb[lo].data_ptr() if dxb is not None else None, r1 - r0, C.byref(opts),
            t1[lo:].ctypes.data if t1 is not None else None, int(trace_cap), logpx[lo].data_ptr(), regs[lo].data_ptr(),
            db[lo].data_ptr(), losses[lo:].ctypes.data, status, stats, s.stream), ensemble_jvp_steps, "t1", t1, losses=losses)

        def rerun(i, model, k):
            args = dict(eps=er[i, :k].t()) if s.train else {}
            (lp, rg), (tl, tr), inf = _jvp.inference_jvp(model, mode, xr[i, :k].t(), pr[i], st, d_ps=_member_dirs(dpb, i, k, single),
                                                         d_xs=_member_dirs(dxb, i, k, single), trace_cap=_alone_cap(trace_cap), **args)
            logpx[i, :k].copy_(lp)
            regs[i, :, :k].copy_(torch.stack(list(rg)))
            rows = torch.stack([tl, *tr], dim=-2)                      # (4, k) or (R, 4, k)
            db[i, :, :, :k].copy_(rows.unsqueeze(0) if single else rows)
            lam = info["lambdas"][i]
            losses[i] = _jvp_loss(mode, lp, rg, lam)
            return inf["stats"], inf["steps"]

        _ens._finish(icnf, info, steps, t1, rerun, s.het)
        if db is not dout:
            dout[:, r0:r1].copy_(db)
        calls += info["calls"]
    info["calls"] = calls
    icnf.last_stats = info["stats"][0]
    d = dout[:, 0] if single else dout.permute(0, 2, 1, 3)             # (M, 4, B) | (M, 4, R, B)
    return (logpx, (regs[:, 0], regs[:, 1], regs[:, 2])), (d[:, 0], (d[:, 1], d[:, 2], d[:, 3])), info


def _jvp_loss(mode, logpx, regs, lam):
    """One member's loss from its outputs, as ``loss_jvp`` forms it, with the member's own lambdas."""
    if _mode_id(mode) == _lib.MODE_TRAIN:
        return float((-logpx + float(lam[0]) * regs[0] + float(lam[1]) * regs[1] + float(lam[2]) * regs[2]).mean())
    return float(-logpx.mean())


def inference_jvp_many(icnf: ICNF, mode, xs, ps, st=None, d_ps=None, d_xs=None, eps=None, t1=None, counts=None, reltol=None,
                       abstol=None, trace_cap=0, bases=None):
    """``inference_many`` and the tangents of every member's four outputs along the member's own directions, in TWO launches
    whatever M (cnf_inference_jvp_many): the plain ensemble solve, then the ensemble form of the tangent kernel right behind it.

    ``xs`` (M, nvars, B), or (nvars, B): one data set scored by all members; ``ps`` (M, n_params); ``d_ps`` (M, n_params) or
    (M, R, n_params); ``d_xs`` (M, nvars, B) or (M, R, nvars, B); at least one of them, ``None`` is zero; R is the same for all
    members.  ``eps`` and ``t1`` as ``inference_many`` takes and draws them, in its order.  Returns ``((logpx (M, B), (E, n, A)),
    (d_logpx, (d_E, d_n, d_A)), info)``: the primal outputs are ``inference_many``'s bit for bit; the tangents are shaped like
    them, with an ``R`` axis behind ``M`` for stacked directions.  ``info`` as ``inference_many``'s (``launches``: 2), with
    ``steps``: per member the accepted ``(t_n, h_n)``.  A member whose part of the launch gave up, or that made more attempts
    than ``trace_cap`` (0: 1024), is run again alone with ``inference_jvp`` on ``member_twin`` (``info["rerun"]``; that call has
    room for 4096 attempts, or ``trace_cap`` when larger); more than
    65535 directions are blocks of calls.  ``counts``, ``reltol``, ``abstol``: heterogeneous members, as ``inference_many`` takes
    them (tangent columns at and behind a member's count are NaN).  ``NotImplementedError`` -- before anything is drawn or a
    handle is made -- for what ``inference_many`` or ``inference_jvp`` refuse, for ``bases=`` and for host arrays."""
    return _inference_jvp_many(icnf, "inference_jvp_many", mode, xs, ps, st, d_ps, d_xs, eps, t1, counts, None, reltol, abstol,
                               trace_cap, bases)


def loss_jvp_many(icnf: ICNF, mode, xs, ps, st=None, d_ps=None, d_xs=None, eps=None, t1=None, counts=None, lambdas=None,
                  reltol=None, abstol=None, trace_cap=0, bases=None):
    """``(losses, d_losses)``: the M members' losses (``loss_many``) and their directional derivatives -- per member the mean over
    its own count of ``-d_logpx + lambda1 d_E + lambda2 d_n + lambda3 d_A`` with its own lambdas (``lambdas`` (M, 3); the model's
    when not given), ``-mean(d_logpx)`` in TestMode: the arithmetic of ``loss_jvp``.  ``losses`` is a float32 numpy vector (M,);
    ``d_losses`` a device tensor, (M,) for one direction per member and (M, R) for stacked ones: with the ``n_params`` one-hot
    directions it is the forward-mode gradient of all M members in one call."""
    primal, tangent, info = _inference_jvp_many(icnf, "loss_jvp_many", mode, xs, ps, st, d_ps, d_xs, eps, t1, counts, lambdas, reltol,
                                                abstol, trace_cap, bases)
    return loss_jvp_reduce(mode, primal, tangent, info["counts"], info["lambdas"])


def generate_jvp_many(icnf: ICNF, mode, ps, st=None, n: int = 1, d_ps=None, d_z0=None, z0=None, eps=None, t0=None, counts=None,
                      reltol=None, abstol=None, trace_cap=0, bases=None):
    """``generate_many(with_logp=True)`` and the tangents of every member's ``(xs, logq)`` along ``(d_ps, d_z0)``
    (cnf_generate_jvp_many).  ``d_z0``: (M, n_in, n) or (M, R, n_in, n).  Returns ``((xs (M, nvars, n), logq (M, n)), (d_xs,
    d_logq), info)``; the full ``n_in`` rows of the final states and of their tangents are ``info["z"]`` / ``info["d_z"]``.
    ``z0``, ``eps`` and ``t0`` as ``generate_many`` takes and draws them, in its order; ``info`` as its
    ``icnf.last_ensemble_info`` (``launches``: 3), with ``steps``.  Reruns (with ``generate_jvp``), blocks, heterogeneous members
    and refusals as ``inference_jvp_many``."""
    import torch
    _refuse(icnf, "generate_jvp_many", bases, ps, d_ps, d_z0, z0, eps)
    n_params, n_in = icnf.nn.n_params_internal, icnf.nvars + n_augment_input(icnf)
    shape = {}

    def dirs(M, k):
        shape["R"], shape["single"] = _check_directions(d_ps, d_z0, M, n_params, n_in, k, "d_z0")
        return tuple(d for d in (d_ps, d_z0) if d is not None)

    s = _ens._settle_sampling(icnf, mode, ps, n, z0, eps, t0, "generate_jvp_many", "generate_jvp", "cnf_ensemble_eval_capacity",
                              cot_pair=dirs, members=dict(counts=counts, reltol=reltol, abstol=abstol))
    l, h = _lib.lib(), icnf.handle()
    m, M, n, dev, pr, zr, er, t0 = s.m, s.M, s.n, s.dev, s.pr, s.zr, s.er, s.t0
    R, single = shape["R"], shape["single"]
    dp, dz = _place_directions(d_ps, d_z0, single, dev)
    opts = _solve_opts(icnf, (icnf.tspan[1], icnf.tspan[0]))              # reverse(tspan)
    zo, lq = _ens._values(s.het, (M, n, n_in), dev), _ens._values(s.het, (M, n), dev)
    d_z = torch.empty((M, R, n, n_in), dtype=torch.float32, device=dev)
    d_lq = torch.empty((M, R, n), dtype=torch.float32, device=dev)
    info, calls = None, 0
    for r0, r1 in _blocks(R):
        whole = r0 == 0 and r1 == R
        dpb, dzb = _block(dp, r0, r1, R), _block(dz, r0, r1, R)
        zb = d_z if whole else torch.empty((M, r1 - r0, n, n_in), dtype=torch.float32, device=dev)
        qb = d_lq if whole else torch.empty((M, r1 - r0, n), dtype=torch.float32, device=dev)
        info, steps = _ens._launch(icnf, s, n, lambda lo, k, status, stats: l.cnf_generate_jvp_many(
            h, m, k, pr[lo].data_ptr(), zr[lo].data_ptr(), er[lo].data_ptr() if s.train else None, n,
            dpb[lo].data_ptr() if dpb is not None else None, dzb[lo].data_ptr() if dzb is not None else None, r1 - r0, C.byref(opts),
            t0[lo:].ctypes.data if t0 is not None else None, int(trace_cap), zo[lo].data_ptr(), lq[lo].data_ptr(), zb[lo].data_ptr(),
            qb[lo].data_ptr(), status, stats, s.stream), ensemble_jvp_steps, "t0", t0, z0=zr.permute(0, 2, 1), eps=er.permute(0, 2, 1))

        def rerun(i, model, k):
            (_, lg), (_, tq), inf = _jvp.generate_jvp(model, mode, pr[i], st, k, d_ps=_member_dirs(dpb, i, k, single),
                                                      d_z0=_member_dirs(dzb, i, k, single), z0=zr[i, :k].t(), eps=er[i, :k].t(),
                                                      trace_cap=_alone_cap(trace_cap))
            zo[i, :k].copy_(inf["z"].t())
            lq[i, :k].copy_(lg)
            tz = inf["d_z"]
            zb[i, :, :k].copy_((tz.unsqueeze(0) if single else tz).permute(0, 2, 1))
            qb[i, :, :k].copy_(tq.unsqueeze(0) if single else tq)
            return inf["stats"], inf["steps"]

        _ens._finish(icnf, info, steps, t0, rerun, s.het)
        if not whole:
            d_z[:, r0:r1].copy_(zb)
            d_lq[:, r0:r1].copy_(qb)
        calls += info["calls"]
    info["calls"] = calls
    zfull = zo.permute(0, 2, 1)                            # (M, n_in, n)
    dzfull = d_z.permute(0, 1, 3, 2)                       # (M, R, n_in, n)
    if single:
        dzfull, d_lq = dzfull[:, 0], d_lq[:, 0]
    info["z"], info["d_z"] = zfull, dzfull
    icnf.last_ensemble_info = info
    return (zfull[:, :icnf.nvars], lq), (dzfull[..., :icnf.nvars, :], d_lq), info
