"""Flow paths: the state of a solve at caller-given times (``solve(prob; saveat = ...)`` of the reference's ODEProblems), from
Tsit5's free interpolant over the ``k_1 .. k_7`` of the accepted steps (cnf_solve_path, include/cnfhip_path.h).

The step sequence is not touched -- no clamping to the save times, no extra evaluations --, so the final state and the
statistics are those of ``base_sol`` on the same route.  A save time is served by the accepted step with
``t_n < tau <= t_n + h`` along the direction of integration; the start of the span gives ``u0`` itself and the end of a step
the accepted state itself, so ``saveat[-1] == tspan[1]`` reproduces the final state bit for bit.

Small two-layer tanh networks (the README / regression networks, conditional models included, up to 8192 columns) get their
path in the launch of the one-launch solve; everything else one attempt at a time on the per-stage kernels
(``info["stats"]["launches"]`` tells which).  Host arrays are staged through device tensors here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .base_icnf import (ICNF, ODEProblem, _Buf, _mode_id, _post, _solve_opts, device_and_stream, generate_prob, inference_prob,
                        n_augment_input, to_device)


def check_saveat(saveat, tspan):
    """``saveat`` as a float32 vector of ``K >= 1`` finite times, monotone (not necessarily strictly) from ``tspan[0]`` to
    ``tspan[1]`` and inside that closed span; ``ValueError`` otherwise.  Touches no device."""
    try:
        sv = np.asarray(saveat, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError) as e:
        raise ValueError(f"saveat must be a sequence of times: {e}") from None
    if sv.size < 1:
        raise ValueError("saveat is empty")
    if not np.all(np.isfinite(sv)):
        raise ValueError("saveat must be finite")
    t0, t1 = np.float32(tspan[0]), np.float32(tspan[1])
    if not (np.isfinite(t0) and np.isfinite(t1)) or t0 == t1:
        raise ValueError("empty or non-finite time span")
    d = np.float32(1.0 if t1 >= t0 else -1.0)
    if np.any(d * (sv - t0) < 0) or np.any(d * (t1 - sv) < 0):
        raise ValueError(f"saveat must lie inside the span it is integrated over, from {float(t0)} to {float(t1)}")
    if np.any(d * np.diff(sv) < 0):
        raise ValueError(f"saveat must be monotone along the direction of integration, from {float(t0)} to {float(t1)}")
    return np.ascontiguousarray(sv)


def _accepted_steps(icnf: ICNF, steps_fn):
    """``(t_n, h_n)`` of the accepted steps ``steps_fn`` of the C ABI keeps for this model: two float32 vectors, or ``None``
    when there is none."""
    read, h = getattr(_lib.lib(), steps_fn), icnf.handle()
    n = read(h, None, None, 0)
    if n < 0:
        return None
    t, hs = np.empty(max(n, 1), dtype=np.float32), np.empty(max(n, 1), dtype=np.float32)
    read(h, t.ctypes.data, hs.ctypes.data, n)
    return t[:n], hs[:n]


def path_steps(icnf: ICNF):
    """``(t_n, h_n)`` of the accepted steps of the last ``solve_path`` on this model (cnf_path_steps): two float32 vectors, or
    ``None`` when there is none."""
    return _accepted_steps(icnf, "cnf_path_steps")


def solve_path(icnf: ICNF, prob: ODEProblem, saveat):
    """``base_sol`` plus the path: returns ``(fsol, path, info)``.  ``fsol`` is what ``base_sol`` returns (the final ``D x B``
    state); ``path`` is ``(K, D, B)`` -- ``path[k]`` the state at ``saveat[k]``, all ``D`` rows --, a device tensor for a
    problem on device tensors and a numpy array otherwise; ``info`` holds ``stats`` (as ``prob.stats``), ``steps`` (the accepted
    steps ``(t_n, h_n)``) and ``t`` (the save times as the library took them, float32)."""
    import torch
    sv = check_saveat(saveat, prob.tspan)
    l, h = _lib.lib(), icnf.handle()
    m = _mode_id(prob.mode)
    host = prob.u0.torch is None
    u0, eb = to_device(icnf, prob.u0), to_device(icnf, prob.eps)
    D, B, K = u0.rows, u0.B, int(sv.size)
    dev, stream = device_and_stream(icnf, u0)
    out = torch.empty(D * B, dtype=torch.float32, device=dev)
    pth = torch.empty(K * B * D, dtype=torch.float32, device=dev)
    opts = _solve_opts(icnf, prob.tspan)
    stats = _lib.cnf_solve_stats()
    _lib.check(l.cnf_solve_path(h, m, u0.ptr, eb.ptr if eb is not None else None, out.data_ptr(), B, C.byref(opts),
                                sv.ctypes.data, K, pth.data_ptr(), C.byref(stats), stream), h)
    prob.stats = stats.as_dict()
    info = {"stats": prob.stats, "steps": path_steps(icnf), "t": sv}
    pv = pth.view(K, B, D).transpose(1, 2)
    if host:
        return _Buf(out.cpu().numpy(), D, B, None), pv.cpu().numpy(), info
    return _Buf(out, D, B, torch), pv, info


def _path_rows(icnf: ICNF, m, pv, info):
    n_in = icnf.nvars + n_augment_input(icnf)
    rows = {"t": info["t"], "z": pv[:, :n_in, :], "dlogp": pv[:, n_in, :], "steps": info["steps"]}
    if m == _lib.MODE_TRAIN:
        rows["E"], rows["n"] = pv[:, n_in + 1, :], pv[:, n_in + 2, :]
    return rows


def inference_path(icnf: ICNF, mode, xs, *args, saveat, eps=None):
    """``inference`` with the path of the flow from the data towards the base: ``inference_path(icnf, mode, xs, [ys,] ps, st,
    saveat=...)`` returns ``(logpx, (E, n, A), path)``.  ``logpx`` and the regularisers are ``inference_sol``'s for the same
    problem; ``path`` is a dict: ``t`` (the save times, from ``tspan[0]`` to ``tspan[1]``), ``z`` ``(K, n_in, B)``, ``dlogp``
    ``(K, B)``, in TrainMode ``E`` and ``n`` ``(K, B)`` (the running regulariser integrals), and ``steps``.  Integrates
    ``icnf.tspan`` in either mode: no steer variate is drawn."""
    check_saveat(saveat, icnf.tspan)
    prob = inference_prob(icnf, mode, xs, *args, eps=eps, tspan=icnf.tspan)
    fsol, pv, info = solve_path(icnf, prob, saveat)
    icnf.last_stats = prob.stats
    logpx, regs = _post(icnf, mode, fsol)
    return logpx, regs, _path_rows(icnf, _mode_id(mode), pv, info)


def generate_path(icnf: ICNF, mode, ps, st=None, n: int = 1, *, saveat, ys=None, z0=None, eps=None):
    """``generate`` with the path of the particles from the base draw to the samples: returns ``(xs, logq, path)``.  ``saveat``
    runs from ``tspan[1]`` to ``tspan[0]`` (sampling integrates the reversed span).  ``xs`` (``nvars x n``) and ``logq`` are what
    ``generate(..., with_logp=True)`` computes: the first rows of the final state and ``logpdf(basedist, z0) + dlogp``.
    ``path`` as for ``inference_path``, plus ``logq`` ``(K, n)``: ``logpdf(basedist, z0) + dlogp(tau_k)``, the log-density of
    the intermediate distribution at the particle (TestMode exact, TrainMode the Hutchinson estimate for the ``eps`` used; a
    non-default base through ``basedist.logpdf``).  No steer variate is drawn."""
    t0, t1 = icnf.tspan
    check_saveat(saveat, (t1, t0))
    prob = generate_prob(icnf, mode, ps, st, n, ys=ys, z0=z0, eps=eps, tspan=icnf.tspan)
    n_in = icnf.nvars + n_augment_input(icnf)
    z0v = prob.u0.view()[:n_in, :]
    fsol, pv, info = solve_path(icnf, prob, saveat)
    icnf.last_stats = prob.stats
    rows = _path_rows(icnf, _mode_id(mode), pv, info)
    host = fsol.torch is None
    if icnf.basedist is not None:                      # float64 on the host, rounded once
        lp0 = np.asarray(icnf.basedist.logpdf(z0v if host else z0v.cpu().numpy()), dtype=np.float32)
        if not host:
            lp0 = fsol.torch.from_numpy(lp0).to(fsol.arr.device)
    else:
        log2pi = np.float32(1.8378770664093453)
        lp0 = -0.5 * ((z0v * z0v).sum(0) + n_in * log2pi)
    fv = fsol.view()
    rows["logq"] = lp0[None, :] + rows["dlogp"]
    return fv[:icnf.nvars, :], lp0 + fv[n_in, :], rows
