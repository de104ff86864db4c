"""Forward-mode derivatives: ``inference`` and ``generate`` together with the TANGENT of their outputs along given directions
of the parameters and of the data / the base draw (cnf_inference_jvp / cnf_generate_jvp, include/cnfhip_jvp.h) -- what the
reference's tests take with ``DifferentiationInterface.gradient(diff_loss, AutoEnzyme(mode = Forward), ...)``
(test/call_tests.jl:32-66, :239-252).  ``vjp.py`` / ``gen_vjp.py`` are the reverse mode.

A pullback gives ``sum_b cot_b d out_b``; a tangent gives ``d out_b . v`` for EVERY sample ``b`` at once: per-sample
sensitivities, the ``J v`` of Gauss-Newton / Fisher products, directional derivatives along an optimiser step.  ``R``
directions ride in one launch behind the plain one-launch solve (one wave per 16-column tile and direction); the primal
outputs are ``inference``'s / ``generate(with_logp=True)``'s.  As everywhere in this package the derivative is the one of the
discrete map through the accepted steps: step sizes, ``eps`` and the (steered) time span are constants.

Envelope: one model on device tensors; two layers, tanh then tanh or identity (or one tanh layer ``n -> n``), ``n_in <= 16``, at
most 64 hidden units (16 with the identity); the default base, no conditioning.  Everything else raises
``NotImplementedError`` before anything is drawn or a handle is made.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .base_icnf import (ICNF, _as_colmajor, _generate_inputs, _is_torch, _mode_id, _solve_opts, _stream, _xs_colmajor, draw_eps,
                        n_augment_input, steer_tspan)
from .path import _accepted_steps
from .rng import HIPRNG


def _refusal(icnf: ICNF):
    """Why this model has no tangent call, or None.  Host logic only: nothing is drawn, no handle is made.  The network envelope
    restates ``tangent_supported`` of csrc/cnf_tangent.hip (which decides for the C ABI): change both together."""
    if icnf.cond:
        return "conditional models have no tangent kernel"
    if icnf.basedist is not None:
        return "a non-default basedist has no tangent kernel"
    if icnf.compute_mode.kernel == "generic":
        return "the tangent follows the one-launch solve of the wave kernels (kernel = 'generic' was asked for)"
    if icnf.nn.planar is not None:
        return "PlanarLayer chains keep (u, w, b) vectors: no tangent kernel"
    dims, acts = icnf.nn.dims, icnf.nn.acts
    tanh, ident = _lib.ACT["tanh"], _lib.ACT["identity"]
    one = len(acts) == 1 and acts[0] == tanh and dims[0] == dims[1] and dims[0] <= 16
    two = len(acts) == 2 and acts[0] == tanh and acts[1] in (tanh, ident) and dims[0] <= 16 and dims[1] <= 64 and \
        not (acts[1] == ident and dims[1] > 16)
    if not (one or two):
        return (f"no tangent kernel for the network {dims}: two layers, tanh then tanh (or identity, up to 16 hidden units), "
                "n_in <= 16 and at most 64 hidden units, or one tanh layer n -> n with n <= 16")
    return None


def _check_model(icnf: ICNF, who, *tensors):
    why = _refusal(icnf)
    if why is not None:
        raise NotImplementedError(f"{who}: " + why)
    if not all(_is_torch(t) for t in tensors):
        raise NotImplementedError(f"{who} takes device tensors")


def _directions(d_ps, d_x, n_params, rows, B, x_name, dev):
    """-> (dp [R][n_params] | None, dx [R][B][rows] | None, R, single): float32, contiguous, on ``dev``."""
    import torch
    if d_ps is None and d_x is None:
        raise ValueError(f"give a direction: d_ps, {x_name} or both")
    R, single = None, None

    def take(d, one_dim, shape, name):
        nonlocal R, single
        if not _is_torch(d):
            d = torch.as_tensor(np.asarray(d, dtype=np.float32))
        d = d.detach().to(device=dev, dtype=torch.float32)
        if d.dim() == one_dim:
            d, s = d.unsqueeze(0), True
        elif d.dim() == one_dim + 1:
            s = False
        else:
            raise ValueError(f"{name} must be {shape} or (R,) + {shape}, got {tuple(d.shape)}")
        if tuple(d.shape[1:]) != shape or d.shape[0] < 1:
            raise ValueError(f"{name} must be {shape} or (R,) + {shape}, got {tuple(d.shape)}")
        if R is not None and (d.shape[0] != R or s != single):
            raise ValueError(f"d_ps and {x_name} must carry the same number of directions")
        R, single = int(d.shape[0]), s
        return d

    dp = take(d_ps, 1, (n_params,), "d_ps").contiguous() if d_ps is not None else None
    dx = take(d_x, 2, (rows, B), x_name).permute(0, 2, 1).contiguous() if d_x is not None else None
    return dp, dx, R, single


def _check_eps(eps, n_in, B):
    """``eps`` given by the caller is ``(n_in, B)``: looked at by shape alone, before any layout or device is."""
    if eps is not None and tuple(getattr(eps, "shape", ())) != (n_in, B):
        raise ValueError(f"eps must be ({n_in}, {B}): one column per sample, got {tuple(getattr(eps, 'shape', ()))}")


def _ptr(t):
    return t.data_ptr() if t is not None else None


def jvp_steps(icnf: ICNF):
    """``(t_n, h_n)`` of the accepted steps of the last ``inference_jvp`` / ``generate_jvp`` on this model (cnf_jvp_steps): two
    float32 vectors, or ``None`` when there is none."""
    return _accepted_steps(icnf, "cnf_jvp_steps")


def _run(icnf, call, R, args_for):
    """The C call once per block of at most ``_lib.JVP_MAX_R`` directions (the grid's second axis); -> (stats, calls)."""
    l, h = _lib.lib(), icnf.handle()
    stats = _lib.cnf_solve_stats()
    calls = 0
    for r0 in range(0, R, _lib.JVP_MAX_R):
        _lib.check(getattr(l, call)(*args_for(r0, min(R, r0 + _lib.JVP_MAX_R), C.byref(stats))), h)
        calls += 1
    return stats.as_dict(), calls


def inference_jvp(icnf: ICNF, mode, xs, ps, st=None, d_ps=None, d_xs=None, eps=None, t1=None, trace_cap=0):
    """``inference(icnf, mode, xs, ps, st)`` and the tangents of its four outputs along ``(d_ps, d_xs)``.

    ``d_ps``: ``(n_params,)`` or ``(R, n_params)``;  ``d_xs``: ``(nvars, B)`` or ``(R, nvars, B)``;  at least one of them, ``None``
    is zero.  Returns ``((logpx, (E, n, A)), (d_logpx, (d_E, d_n, d_A)), info)``: the primal outputs are ``inference``'s bit for
    bit; the tangents are shaped like them, with a leading ``R`` axis for stacked directions.  ``eps`` is drawn as ``inference``
    draws it when not given (TrainMode), then the steered end time unless ``t1`` is given.  ``info``: ``stats`` (the solve's, its
    ``launches`` counting the tangent launch), ``steps`` (the accepted ``(t_n, h_n)``), ``launches`` and ``calls`` (C calls: one
    per 65535 directions).  ``trace_cap``: step attempts the call has room for (0: 4096)."""
    import torch
    _check_model(icnf, "inference_jvp", xs, ps)
    m = _mode_id(mode)
    n_in = icnf.nvars + n_augment_input(icnf)
    # the shapes first -- of xs, of the directions, of eps --, before a layout is made, anything is drawn or a device is asked for
    if xs.dim() != 2 or xs.shape[0] != icnf.nvars or xs.shape[1] < 1:
        raise ValueError(f"xs must be (nvars = {icnf.nvars}, B), got {tuple(xs.shape)}")
    B, dev = int(xs.shape[1]), xs.device
    dp, dx, R, single = _directions(d_ps, d_xs, icnf.nn.n_params_internal, icnf.nvars, B, "d_xs", dev)
    _check_eps(eps, n_in, B)
    xb = _xs_colmajor(icnf, xs)
    icnf.set_params(ps)
    if eps is not None:
        eb = _as_colmajor(eps, n_in, "eps")
    elif m == _lib.MODE_TRAIN:
        eb = draw_eps(icnf, xb, B)
    else:
        eb = None
    tspan = steer_tspan(icnf, mode) if t1 is None else (icnf.tspan[0], float(t1))
    opts = _solve_opts(icnf, tspan)
    buf = torch.empty(4 * B, dtype=torch.float32, device=dev)
    logpx, regs = buf[:B], buf[B:]
    dout = torch.empty(R, 4, B, dtype=torch.float32, device=dev)
    h = icnf.handle()
    ep = eb.ptr if (eb is not None and m == _lib.MODE_TRAIN) else None
    stream = _stream(xb)
    stats, calls = _run(
        icnf, "cnf_inference_jvp", R,
        lambda r0, r1, sp: (h, m, xb.ptr, ep, B, _ptr(dp[r0:r1] if dp is not None else None), _ptr(dx[r0:r1] if dx is not None else None),
                            r1 - r0, C.byref(opts), int(trace_cap), logpx.data_ptr(), regs.data_ptr(), dout[r0:r1].data_ptr(), sp, stream))
    icnf.last_stats = stats
    r = regs.view(3, B)
    d = dout[0] if single else dout.permute(1, 0, 2)
    info = {"stats": stats, "steps": jvp_steps(icnf), "launches": stats["launches"], "calls": calls}
    return (logpx, (r[0], r[1], r[2])), (d[0], (d[1], d[2], d[3])), info


def generate_jvp(icnf: ICNF, mode, ps, st=None, n: int = 1, d_ps=None, d_z0=None, z0=None, eps=None, t0=None, trace_cap=0):
    """``generate(icnf, mode, ps, st, n, with_logp=True)`` and the tangents of ``(xs, logq)`` along ``(d_ps, d_z0)``.

    ``d_z0``: ``(n_in, n)`` or ``(R, n_in, n)``.  Returns ``((xs, logq), (d_xs, d_logq), info)`` -- ``d_xs`` is ``(nvars, n)`` or
    ``(R, nvars, n)``; the full ``n_in`` rows of the final state and of its tangent are ``info["z"]`` / ``info["d_z"]``.  ``z0``
    and ``eps`` are drawn as ``generate`` draws them when not given (a device generator, or device tensors: the call takes device
    tensors), then the steered span; ``t0``: the time sampling starts from instead (it integrates down to ``icnf.tspan[0]``)."""
    import torch
    _check_model(icnf, "generate_jvp", ps)
    m = _mode_id(mode)
    n_in = icnf.nvars + n_augment_input(icnf)
    if (z0 is not None and not _is_torch(z0)) or (z0 is None and not isinstance(icnf.rng, HIPRNG)):
        raise NotImplementedError("generate_jvp takes device tensors (a z0 on the device, or a HIPRNG that draws it there)")
    if z0 is not None and (z0.dim() != 2 or tuple(z0.shape) != (n_in, n)):
        raise ValueError(f"z0 must be ({n_in}, n = {n}), got {tuple(z0.shape)}")
    dev = z0.device if z0 is not None else torch.device("cuda", icnf.device)
    dp, dz, R, single = _directions(d_ps, d_z0, icnf.nn.n_params_internal, n_in, n, "d_z0", dev)
    _check_eps(eps, n_in, n)
    zb, eb = _generate_inputs(icnf, mode, ps, n, None, z0, eps)
    if eb.torch is None:
        eb = _as_colmajor(torch.as_tensor(eb.view()).to(dev), n_in, "eps")
    t_lo, t_hi = steer_tspan(icnf, mode) if t0 is None else (icnf.tspan[0], float(t0))
    opts = _solve_opts(icnf, (t_hi, t_lo))                 # reverse(tspan)
    out = torch.empty(n * n_in + n, dtype=torch.float32, device=dev)
    z, logq = out[:n * n_in], out[n * n_in:]
    d_z = torch.empty(R, n, n_in, dtype=torch.float32, device=dev)
    d_lq = torch.empty(R, n, dtype=torch.float32, device=dev)
    h = icnf.handle()
    ep = eb.ptr if m == _lib.MODE_TRAIN else None
    stream = _stream(zb)
    stats, calls = _run(
        icnf, "cnf_generate_jvp", R,
        lambda r0, r1, sp: (h, m, zb.ptr, ep, n, _ptr(dp[r0:r1] if dp is not None else None), _ptr(dz[r0:r1] if dz is not None else None),
                            r1 - r0, C.byref(opts), int(trace_cap), z.data_ptr(), logq.data_ptr(), d_z[r0:r1].data_ptr(),
                            d_lq[r0:r1].data_ptr(), sp, stream))
    icnf.last_stats = stats
    zfull = z.view(n, n_in).t()
    dzfull = d_z.permute(0, 2, 1)
    if single:
        dzfull, d_lq = dzfull[0], d_lq[0]
    info = {"stats": stats, "steps": jvp_steps(icnf), "launches": stats["launches"], "calls": calls, "z": zfull, "d_z": dzfull}
    return (zfull[:icnf.nvars], logq), (dzfull[..., :icnf.nvars, :], d_lq), info


def loss_jvp(icnf: ICNF, mode, xs, ps, st=None, d_ps=None, d_xs=None, eps=None, t1=None, trace_cap=0):
    """``(loss, d_loss)``: the loss of ``loss(icnf, mode, xs, ps, st)`` and its directional derivative(s) --
    ``d_loss = mean(-d_logpx + lambda1 d_E + lambda2 d_n + lambda3 d_A)`` in TrainMode (src/icnf.jl:481-490), ``-mean(d_logpx)``
    in TestMode (src/base_icnf.jl:489-497) --, the quantity the reference's forward-mode ``gradient(diff_loss, ...)`` assembles
    entry by entry.  ``loss`` is a float; ``d_loss`` a device tensor, a scalar for one direction and ``(R,)`` for stacked ones:
    with the ``n_params`` one-hot directions it is the gradient of ``loss_and_grad``."""
    (logpx, (E, nn, A)), (dl, (dE, dn, dA)), _ = inference_jvp(icnf, mode, xs, ps, st, d_ps=d_ps, d_xs=d_xs, eps=eps, t1=t1,
                                                                trace_cap=trace_cap)
    if _mode_id(mode) == _lib.MODE_TRAIN:
        l1, l2, l3 = float(icnf.lambda1), float(icnf.lambda2), float(icnf.lambda3)
        return float((-logpx + l1 * E + l2 * nn + l3 * A).mean()), (-dl + l1 * dE + l2 * dn + l3 * dA).mean(dim=-1)
    return float(-logpx.mean()), -dl.mean(dim=-1)
