"""Ensemble flow paths: the paths of M members, and the vector-Jacobian product of a cotangent of those paths, in ONE launch
(include/cnfhip_ensemble_path.h).  ``path.py`` / ``path_vjp.py`` are the single-model calls; ``ensemble.py`` the ensemble calls
without a path.  A path loss over M members -- snapshot matching on M folds, annealed reverse-KL over ``logq(tau_k)`` along a
temperature ladder, kinetic penalties of M restarts -- is otherwise a loop of M small launches.

Everything follows ``ensemble.py``: ``_refusal`` with the same messages, raised before anything is drawn or a handle exists;
device tensors only; the draws in ``inference_many`` / ``generate_many``'s order; consecutive launches above the capacity
(``info["calls"]``); a member whose part of a launch gave up is run again alone (``info["rerun"]``).  As the single-model path
calls, these integrate ``icnf.tspan`` (sampling: reversed) for every member and draw no steer variate: ``counts``, ``lambdas``,
``reltol``, ``abstol``, ``t1`` and ``t0`` are not keywords here.

``saveat`` is ``(K,)`` -- one set of save times for all members -- or ``(M, K)`` -- member m's own ``saveat[m]``.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _lib
from .base_icnf import ICNF, _is_torch, _mode_id, _solve_opts, n_augment_input
from .ensemble import _capacity, _cot_many, _cot_pair_many, _finish, _launch, _refusal, _settle_density, _settle_sampling, member_twin
from .path import check_saveat, generate_path, inference_path
from .path_vjp import generate_path_vjp, inference_path_vjp

_LOG2PI = np.float32(1.8378770664093453)


def ensemble_path_capacity(icnf: ICNF, mode, B: int) -> int:
    """The largest M one ``inference_path_many`` / ``generate_path_many`` launch takes for this model, mode and batch size
    (cnf_ensemble_path_capacity); 0: no ensemble form."""
    return _capacity(icnf, mode, "cnf_ensemble_path_capacity", B)


def ensemble_path_vjp_capacity(icnf: ICNF, mode, B: int) -> int:
    """The largest M one ``inference_path_vjp_many`` / ``generate_path_vjp_many`` launch takes (cnf_ensemble_path_vjp_capacity:
    the smaller of the two directions'); 0: no ensemble form."""
    return _capacity(icnf, mode, "cnf_ensemble_path_vjp_capacity", B)


def ensemble_path_steps(icnf: ICNF, member: int):
    """``(t_n, h_n)`` of the steps ``member`` accepted in the last ensemble path CALL on this model (cnf_ensemble_path_steps; the
    index counts within that call): two float32 vectors, or ``None`` when there is none or the member gave up."""
    l, h = _lib.lib(), icnf.handle()
    n = l.cnf_ensemble_path_steps(h, int(member), None, None, 0)
    if n < 0:
        return None
    t, hs = np.empty(max(n, 1), dtype=np.float32), np.empty(max(n, 1), dtype=np.float32)
    l.cnf_ensemble_path_steps(h, int(member), t.ctypes.data, hs.ctypes.data, n)
    return t[:n], hs[:n]


def _no_bases(who, bases):
    """The ensemble path calls take no ``bases=`` (a base per member: include/cnfhip_ensemble_base.h): refused before anything is
    drawn or asks for a device."""
    if bases is not None:
        raise NotImplementedError(f"{who}: the ensemble path calls take no bases= (score the members with inference_many / "
                                  "inference_vjp_many, or one member at a time on a model constructed with basedist=)")


def check_saveat_many(saveat, tspan, M):
    """``saveat`` as float32 ``(K,)`` -- one set for all members -- or ``(M, K)`` -- one per member --, every set checked by
    ``check_saveat`` against ``tspan``; ``ValueError`` otherwise (a member's index is named).  Touches no device."""
    try:
        sv = np.asarray(saveat, dtype=np.float32)
    except (TypeError, ValueError) as e:
        raise ValueError(f"saveat must be a sequence of times: {e}") from None
    if sv.ndim <= 1:
        return check_saveat(sv, tspan)
    if sv.ndim != 2 or sv.shape[0] != M:
        raise ValueError(f"saveat must be (K,) or (M = {M}, K), got {sv.shape}")
    rows = []
    for i in range(M):
        try:
            rows.append(check_saveat(sv[i], tspan))
        except ValueError as e:
            raise ValueError(f"saveat of member {i}: {e}") from None
    return np.ascontiguousarray(np.stack(rows))


def _sum_axis(t, dim):
    """The sum over ``dim`` by a fixed tree of elementwise additions (neighbours pairwise, an odd last entry carried): the same
    bits whatever the other axes are -- a member of M gets what it gets alone, which a library reduction, free to split its
    work by the number of outputs, does not promise -- in log2 of the length many operations."""
    import torch
    t = t.movedim(dim, 0)
    while t.shape[0] > 1:
        n = t.shape[0] // 2
        pair = t[0:2 * n:2] + t[1:2 * n:2]
        t = pair if t.shape[0] == 2 * n else torch.cat([pair, t[2 * n:]], dim=0)
    return t[0]


def _path_rows_many(train, n_in, pth, sv, steps):
    """The slices [M][K][B][D] -> the single call's dict with a leading member axis."""
    pv = pth.permute(0, 1, 3, 2)
    rows = {"t": sv, "z": pv[:, :, :n_in, :], "dlogp": pv[:, :, n_in, :], "steps": steps}
    if train:
        rows["E"], rows["n"] = pv[:, :, n_in + 1, :], pv[:, :, n_in + 2, :]
    return rows


def _saveat_ptr(sv, lo):
    return (sv[lo:] if sv.ndim == 2 else sv).ctypes.data


def _member_saveat(sv, i):
    return sv[i] if sv.ndim == 2 else sv


def _named(i, fn):
    """``fn()`` on the single-model route; a failure names the member."""
    try:
        return fn()
    except _lib.CNFError as e:
        raise _lib.CNFError(e.status, f"ensemble member {i}: {e}") from None


def _path_cot_given(icnf, who, path_cot, names, M, K, B, train):
    """The dict of row cotangents with member axes, checked: the entries that were given (``ValueError`` otherwise).  Host
    logic only.  ``names``: key -> state row."""
    if path_cot is None:
        return {}
    if not isinstance(path_cot, dict) or any(k not in names for k in path_cot):
        raise ValueError(f"{who}: path_cot is a dict with any of {sorted(names)}")
    n_in = icnf.nvars + n_augment_input(icnf)
    D = n_in + (3 if train else 1)
    given = {k: v for k, v in path_cot.items() if v is not None}
    for k, v in given.items():
        if not _is_torch(v):
            raise ValueError(f"{who}: path_cot[{k!r}] must be a device tensor")
        if names[k] >= D:
            raise ValueError(f"{who}: path_cot[{k!r}] has no meaning in TestMode (the row is not integrated)")
        want = (M, K, n_in, B) if k == "z" else (M, K, B)
        if tuple(v.shape) != want:
            raise ValueError(f"{who}: path_cot[{k!r}] must be {want}, got {tuple(v.shape)}")
    return given


def _path_cot_many(given, names, M, K, B, n_in, train, dev):
    """... -> ``[M][K][B][D]`` (None: nothing given)."""
    import torch
    if not given:
        return None
    D = n_in + (3 if train else 1)
    pc = torch.zeros((M, K, B, D), dtype=torch.float32, device=dev)
    for k, v in given.items():
        v = v.detach().to(device=dev, dtype=torch.float32)
        if k == "z":
            pc[:, :, :, :n_in] = v.permute(0, 1, 3, 2)
        else:
            pc[:, :, :, names[k]] = v
    return pc


# ---------------------------------------------------------------------------------------
# the plain calls
# ---------------------------------------------------------------------------------------
def inference_path_many(icnf: ICNF, mode, xs, ps, st=None, *, saveat, eps=None, bases=None):
    """``inference_path`` of M members in ONE launch (cnf_inference_path_many).  ``xs`` (M, nvars, B), or (nvars, B) shared by all
    members; ``ps`` (M, n_params); ``eps`` (M, n_in, B; TrainMode) given or drawn in ``inference_many``'s order, without a steer
    variate; ``saveat`` (K,) or (M, K), from ``tspan[0]`` to ``tspan[1]``.  Returns ``(logpx (M, B), (E, n, A), path, info)``:
    ``path`` is ``inference_path``'s dict with a leading member axis -- ``z`` (M, K, n_in, B), ``dlogp`` (M, K, B), in TrainMode
    ``E``, ``n`` --, ``t`` as it was given and ``steps`` a list of M ``(t_n, h_n)``.  ``logpx`` and the regularisers are
    ``inference_many``'s for the same inputs, bit for bit.  ``info`` as ``inference_many``'s (``launches`` is 1); a member whose
    part of the launch gave up is run again with ``inference_path`` on a twin of the model (``info["rerun"]``)."""
    _no_bases("inference_path_many", bases)
    import torch
    who = "inference_path_many"
    box = {}

    def saveat_check(M, B):
        box["sv"] = check_saveat_many(saveat, icnf.tspan, M)
        return ()

    s = _settle_density(icnf, mode, xs, ps, eps, None, who, "inference_path", "cnf_ensemble_path_capacity", cot_rows=saveat_check,
                        steer=False)
    sv = box["sv"]
    l, h = _lib.lib(), icnf.handle()
    m, M, B, dev, xr, pr, er = s.m, s.M, s.B, s.dev, s.xr, s.pr, s.er
    K, D = int(sv.shape[-1]), s.n_in + (3 if s.train else 1)
    opts = _solve_opts(icnf, icnf.tspan)
    logpx, regs = torch.empty((M, B), dtype=torch.float32, device=dev), torch.empty((M, 3, B), dtype=torch.float32, device=dev)
    pth = torch.empty((M, K, B, D), dtype=torch.float32, device=dev)
    losses = np.empty(M, dtype=np.float32)
    info, steps = _launch(icnf, s, B, lambda lo, n, status, stats: l.cnf_inference_path_many(
        h, m, n, pr[lo].data_ptr(), xr[lo].data_ptr(), er[lo].data_ptr() if er is not None else None, B, C.byref(opts), None,
        logpx[lo].data_ptr(), regs[lo].data_ptr(), losses[lo:].ctypes.data, status, stats, 0, s.stream, _saveat_ptr(sv, lo), K,
        1 if sv.ndim == 2 else 0, pth[lo].data_ptr()), ensemble_path_steps, "t1", None, losses=losses,
        eps=er.permute(0, 2, 1) if er is not None else None)

    def rerun(i, model, k):
        from .ensemble import member_loss_from_sums
        twin = member_twin(icnf)
        try:
            lp, rg, pa = _named(i, lambda: inference_path(twin, mode, xr[i].t(), pr[i], st, saveat=_member_saveat(sv, i),
                                                          eps=er[i].t() if s.train else None))
            stats_i = dict(twin.last_stats)
        finally:
            twin.close()
        logpx[i].copy_(lp)
        regs[i].copy_(torch.stack(list(rg)))
        pth[i, :, :, :s.n_in].copy_(pa["z"].permute(0, 2, 1))
        pth[i, :, :, s.n_in].copy_(pa["dlogp"])
        if s.train:
            pth[i, :, :, s.n_in + 1].copy_(pa["E"])
            pth[i, :, :, s.n_in + 2].copy_(pa["n"])
        sums = torch.stack([logpx[i].sum(), regs[i, 0].sum(), regs[i, 1].sum(), regs[i, 2].sum(),
                            torch.tensor(float(B), device=dev)])
        losses[i] = member_loss_from_sums(mode, sums, info["lambdas"][i])
        return stats_i, pa["steps"]

    _finish(icnf, info, steps, None, rerun)
    icnf.last_stats = info["stats"][0]
    return logpx, (regs[:, 0], regs[:, 1], regs[:, 2]), _path_rows_many(s.train, s.n_in, pth, sv, info["steps"]), info


def _logq_path(zr, dlogp, n_in):
    """``logpdf(N(0, I), z0) + dlogp(tau_k)`` for [M][n][n_in] base draws and (M, K, n) rows."""
    lp0 = -0.5 * (_sum_axis(zr * zr, 2) + n_in * _LOG2PI)
    return lp0[:, None, :] + dlogp


def generate_path_many(icnf: ICNF, mode, ps, st=None, n: int = 1, *, saveat, z0=None, eps=None, bases=None):
    """``generate_path`` of M members in one launch and the column kernel (cnf_generate_path_many).  ``ps`` (M, n_params);
    ``z0`` / ``eps`` (M, n_in, n) given or drawn in ``generate_many``'s order, without a steer variate; ``saveat`` (K,) or (M, K),
    from ``tspan[1]`` to ``tspan[0]``.  Returns ``(xs (M, nvars, n), logq (M, n), path, info)``: ``xs`` and ``logq`` are
    ``generate_many(with_logp=True)``'s, bit for bit; ``path`` as ``inference_path_many``'s plus ``logq`` (M, K, n).  ``info`` as
    ``generate_many``'s (``z0``, ``eps``: the inputs used); a member whose part of the launch gave up is run again with
    ``generate_path`` on a twin of the model."""
    _no_bases("generate_path_many", bases)
    import torch
    who = "generate_path_many"
    box = {}
    t0, t1 = icnf.tspan

    def saveat_check(M, nn):
        box["sv"] = check_saveat_many(saveat, (t1, t0), M)
        return ()

    s = _settle_sampling(icnf, mode, ps, n, z0, eps, None, who, "generate_path", "cnf_ensemble_path_capacity", cot_pair=saveat_check,
                         steer=False)
    sv = box["sv"]
    l, h = _lib.lib(), icnf.handle()
    m, M, n, n_in, dev, pr, zr, er = s.m, s.M, s.n, s.n_in, s.dev, s.pr, s.zr, s.er
    K, D = int(sv.shape[-1]), n_in + (3 if s.train else 1)
    opts = _solve_opts(icnf, (t1, t0))                     # reverse(tspan)
    xo, lq = torch.empty((M, n, icnf.nvars), dtype=torch.float32, device=dev), torch.empty((M, n), dtype=torch.float32, device=dev)
    pth = torch.empty((M, K, n, D), dtype=torch.float32, device=dev)
    info, steps = _launch(icnf, s, n, lambda lo, k, status, stats: l.cnf_generate_path_many(
        h, m, k, pr[lo].data_ptr(), zr[lo].data_ptr(), er[lo].data_ptr() if s.train else None, n, C.byref(opts), None,
        xo[lo].data_ptr(), lq[lo].data_ptr(), status, stats, 0, s.stream, _saveat_ptr(sv, lo), K, 1 if sv.ndim == 2 else 0,
        pth[lo].data_ptr()), ensemble_path_steps, "t0", None, z0=zr.permute(0, 2, 1), eps=er.permute(0, 2, 1))
    icnf.last_ensemble_info = info                         # (published before a failed member raises: it says which)

    def rerun(i, model, k):
        twin = member_twin(icnf)
        try:
            x_i, lq_i, pa = _named(i, lambda: generate_path(twin, mode, pr[i], st, n, saveat=_member_saveat(sv, i), z0=zr[i].t(),
                                                            eps=er[i].t()))
            stats_i = dict(twin.last_stats)
        finally:
            twin.close()
        xo[i].copy_(torch.as_tensor(x_i, device=dev).t())
        lq[i].copy_(torch.as_tensor(lq_i, device=dev))
        pth[i, :, :, :n_in].copy_(pa["z"].permute(0, 2, 1))
        pth[i, :, :, n_in].copy_(pa["dlogp"])
        if s.train:
            pth[i, :, :, n_in + 1].copy_(pa["E"])
            pth[i, :, :, n_in + 2].copy_(pa["n"])
        return stats_i, pa["steps"]

    _finish(icnf, info, steps, None, rerun)
    path = _path_rows_many(s.train, n_in, pth, sv, info["steps"])
    path["logq"] = _logq_path(zr, path["dlogp"], n_in)
    return xo.permute(0, 2, 1), lq, path, info


# ---------------------------------------------------------------------------------------
# the vector-Jacobian products
# ---------------------------------------------------------------------------------------
def inference_path_vjp_many(icnf: ICNF, mode, xs, ps, st=None, *, saveat, cot=None, path_cot=None, eps=None, with_x=False, bases=None):
    """``inference_path_vjp`` of M members in ONE launch and one of the partial sums (cnf_inference_path_vjp_many).  ``xs``
    (M, nvars, B) or (nvars, B) shared; ``ps`` (M, n_params); ``saveat`` (K,) or (M, K); ``cot = (g_logpx, (g_E, g_n, g_A))``,
    each (M, B) or None, or None for no cotangent of the outputs; ``path_cot``: a dict with any of ``z`` (M, K, n_in, B),
    ``dlogp`` (M, K, B) and in TrainMode ``E``, ``n`` (M, K, B).  Returns ``(logpx (M, B), (E, n, A), path, grads (M, n_params)[,
    grad_x (M, nvars, B)], info)``, member m's as ``inference_path_vjp`` gives them for it alone -- with M = 1 the very same
    launch.  A member whose part of the launch gave up is run again with ``inference_path_vjp`` on a twin of the model
    (``info["rerun"]``); if that raises, the error names the member."""
    _no_bases("inference_path_vjp_many", bases)
    import torch
    who = "inference_path_vjp_many"
    box = {}

    names = dict(zip(("z", "dlogp", "E", "n"), (0,) + tuple(icnf.nvars + n_augment_input(icnf) + r for r in range(3))))

    def checks(M, B):
        box["sv"] = check_saveat_many(saveat, icnf.tspan, M)
        rows = _cot_many(cot, M, B) if cot is not None else ()
        box["pc"] = _path_cot_given(icnf, who, path_cot, names, M, int(box["sv"].shape[-1]), B, _mode_id(mode) == _lib.MODE_TRAIN)
        return tuple(rows) + tuple(box["pc"].values())

    s = _settle_density(icnf, mode, xs, ps, eps, None, who, "inference_record and inference_pullback", "cnf_ensemble_path_vjp_capacity",
                        cot_rows=checks, steer=False)
    sv = box["sv"]
    l, h = _lib.lib(), icnf.handle()
    m, M, B, n_in, dev, xr, pr, er = s.m, s.M, s.B, s.n_in, s.dev, s.xr, s.pr, s.er
    K, D = int(sv.shape[-1]), n_in + (3 if s.train else 1)
    cm = None
    if cot is not None:
        cm = torch.zeros((M, 4, B), dtype=torch.float32, device=dev)
        for i, r in enumerate(s.cot[:4]):
            if r is not None:
                cm[:, i].copy_(r.detach())
    pc = _path_cot_many(box["pc"], names, M, K, B, n_in, s.train, dev)
    opts = _solve_opts(icnf, icnf.tspan)
    logpx, regs = torch.empty((M, B), dtype=torch.float32, device=dev), torch.empty((M, 3, B), dtype=torch.float32, device=dev)
    pth = torch.empty((M, K, B, D), dtype=torch.float32, device=dev)
    grads = torch.empty((M, pr.shape[1]), dtype=torch.float32, device=dev)
    gz = torch.empty((M, B, n_in), dtype=torch.float32, device=dev) if with_x else None
    icnf._record = None                                    # (the call ends whatever was recorded on the handle)
    info, steps = _launch(icnf, s, B, lambda lo, n, status, stats: l.cnf_inference_path_vjp_many(
        h, m, n, pr[lo].data_ptr(), xr[lo].data_ptr(), er[lo].data_ptr() if er is not None else None, B, C.byref(opts),
        _saveat_ptr(sv, lo), K, 1 if sv.ndim == 2 else 0, cm[lo].data_ptr() if cm is not None else None,
        pc[lo].data_ptr() if pc is not None else None, logpx[lo].data_ptr(), regs[lo].data_ptr(), pth[lo].data_ptr(),
        grads[lo].data_ptr(), gz[lo].data_ptr() if with_x else None, status, stats, s.stream), ensemble_path_steps, "t1", None,
        eps=er.permute(0, 2, 1) if er is not None else None)
    gx = gz[:, :, :icnf.nvars].permute(0, 2, 1).contiguous() if with_x else None

    def rerun(i, model, k):
        twin = member_twin(icnf)
        try:
            cot_i = (cm[i, 0], (cm[i, 1], cm[i, 2], cm[i, 3])) if cm is not None else None
            pc_i = None
            if pc is not None:
                pc_i = {"z": pc[i, :, :, :n_in].permute(0, 2, 1), "dlogp": pc[i, :, :, n_in]}
                if s.train:
                    pc_i["E"], pc_i["n"] = pc[i, :, :, n_in + 1], pc[i, :, :, n_in + 2]
            res = _named(i, lambda: inference_path_vjp(twin, mode, xr[i].t(), pr[i], None, saveat=_member_saveat(sv, i), cot=cot_i,
                                                       path_cot=pc_i, eps=er[i].t() if s.train else None, with_x=with_x))
        finally:
            twin.close()
        logpx[i].copy_(res[0])
        regs[i].copy_(torch.stack(list(res[1])))
        pa = res[2]
        pth[i, :, :, :n_in].copy_(pa["z"].permute(0, 2, 1))
        pth[i, :, :, n_in].copy_(pa["dlogp"])
        if s.train:
            pth[i, :, :, n_in + 1].copy_(pa["E"])
            pth[i, :, :, n_in + 2].copy_(pa["n"])
        grads[i].copy_(res[3])
        if with_x:
            gx[i].copy_(res[4])
        return dict(res[-1]["stats"]), res[-1]["steps"]

    _finish(icnf, info, steps, None, rerun)
    icnf._record = None
    icnf.last_stats = info["stats"][0]
    out = (logpx, (regs[:, 0], regs[:, 1], regs[:, 2]), _path_rows_many(s.train, n_in, pth, sv, info["steps"]), grads)
    return out + ((gx, info) if with_x else (info,))


def generate_path_vjp_many(icnf: ICNF, mode, ps, st=None, n: int = 1, *, saveat, cot=None, path_cot=None, z0=None, eps=None,
                           with_z0=False, bases=None):
    """``generate_path_vjp`` of M members in ONE launch, one of the partial sums and the column kernels
    (cnf_generate_path_vjp_many).  ``ps`` (M, n_params); ``saveat`` (K,) or (M, K) from ``tspan[1]`` to ``tspan[0]``;
    ``cot = (g_x, g_logq)`` as ``generate_vjp_many`` takes it (None: no cotangent of the outputs); ``path_cot``: a dict with any of
    ``z`` (M, K, n_in, n) and ``logq`` (M, K, n) -- it goes to the dlogp row, and its sum over k joins ``g_logq`` in the
    ``-(...) z0`` tail of ``grad_z0``, added here on the host side where ``generate_path_vjp`` adds it.  The two host-side sums
    (over k of that tail, over the rows of ``logpdf(z0)`` in ``path["logq"]``) are fixed trees of additions (``_sum_axis``), so that
    member m's bits do not depend on M; ``generate_path_vjp`` leaves them to ``torch.sum``, so with M = 1 ``grad_z0`` under a
    ``logq`` path cotangent and ``path["logq"]`` agree with it to rounding, every other output bit for bit.  Returns ``(xs (M, nvars, n), logq
    (M, n), path, grads (M, n_params)[, grad_z0 (M, n_in, n)], info)``.  Re-runs and failures as ``inference_path_vjp_many``
    (with ``generate_path_vjp``)."""
    _no_bases("generate_path_vjp_many", bases)
    import torch
    who = "generate_path_vjp_many"
    box = {}
    t0, t1 = icnf.tspan

    names = {"z": 0, "logq": icnf.nvars + n_augment_input(icnf)}

    def checks(M, nn):
        box["sv"] = check_saveat_many(saveat, (t1, t0), M)
        pair = _cot_pair_many(icnf, cot, M, nn) if cot is not None and any(c is not None for c in cot) else (None, None)
        box["pc"] = _path_cot_given(icnf, who, path_cot, names, M, int(box["sv"].shape[-1]), nn, _mode_id(mode) == _lib.MODE_TRAIN)
        return tuple(pair) + tuple(box["pc"].values())

    s = _settle_sampling(icnf, mode, ps, n, z0, eps, None, who, "generate_record and generate_pullback", "cnf_ensemble_path_vjp_capacity",
                         cot_pair=checks, steer=False)
    sv = box["sv"]
    l, h = _lib.lib(), icnf.handle()
    m, M, n, n_in, dev, pr, zr, er = s.m, s.M, s.n, s.n_in, s.dev, s.pr, s.zr, s.er
    K, D = int(sv.shape[-1]), n_in + (3 if s.train else 1)
    g_x, g_l = s.cot[0], s.cot[1]
    cz = cl = None
    if g_x is not None:                                    # [M][n][n_in], zeros on the rows that were not given
        cz = torch.zeros((M, n, n_in), dtype=torch.float32, device=dev)
        cz[:, :, :g_x.shape[1]] = g_x.detach().permute(0, 2, 1)
    if g_l is not None:
        cl = g_l.detach().to(torch.float32).contiguous()
    pc = _path_cot_many(box["pc"], names, M, K, n, n_in, s.train, dev)
    opts = _solve_opts(icnf, (t1, t0))                     # reverse(tspan)
    xo, lq = torch.empty((M, n, icnf.nvars), dtype=torch.float32, device=dev), torch.empty((M, n), dtype=torch.float32, device=dev)
    pth = torch.empty((M, K, n, D), dtype=torch.float32, device=dev)
    grads = torch.empty((M, pr.shape[1]), dtype=torch.float32, device=dev)
    gz = torch.empty((M, n, n_in), dtype=torch.float32, device=dev) if with_z0 else None
    icnf._record = None                                    # (the call ends whatever was recorded on the handle)
    info, steps = _launch(icnf, s, n, lambda lo, k, status, stats: l.cnf_generate_path_vjp_many(
        h, m, k, pr[lo].data_ptr(), zr[lo].data_ptr(), er[lo].data_ptr() if s.train else None, n, C.byref(opts), _saveat_ptr(sv, lo), K,
        1 if sv.ndim == 2 else 0, cz[lo].data_ptr() if cz is not None else None, cl[lo].data_ptr() if cl is not None else None,
        pc[lo].data_ptr() if pc is not None else None, xo[lo].data_ptr(), lq[lo].data_ptr(), pth[lo].data_ptr(), grads[lo].data_ptr(),
        gz[lo].data_ptr() if with_z0 else None, status, stats, s.stream), ensemble_path_steps, "t0", None,
        z0=zr.permute(0, 2, 1), eps=er.permute(0, 2, 1))
    icnf.last_ensemble_info = info
    tail = with_z0 and "logq" in box["pc"]
    if tail:
        # logq(tau_k) = logpdf(N(0, I), z0) + dlogp(tau_k): the first term's part of the cotangent, -(sum_k g_k) z0
        gz -= _sum_axis(pc[:, :, :, n_in], 1)[:, :, None] * zr

    def rerun(i, model, k):
        twin = member_twin(icnf)
        try:
            cot_i = (cz[i].t() if cz is not None else None, cl[i] if cl is not None else None) if (cz is not None or cl is not None) else None
            pc_i = None
            if pc is not None:
                pc_i = {"z": pc[i, :, :, :n_in].permute(0, 2, 1), "logq": pc[i, :, :, n_in] if "logq" in box["pc"] else None}
            res = _named(i, lambda: generate_path_vjp(twin, mode, pr[i], None, n, saveat=_member_saveat(sv, i), cot=cot_i, path_cot=pc_i,
                                                      z0=zr[i].t(), eps=er[i].t(), with_z0=with_z0))
        finally:
            twin.close()
        xo[i].copy_(res[0].t())
        lq[i].copy_(res[1])
        pa = res[2]
        pth[i, :, :, :n_in].copy_(pa["z"].permute(0, 2, 1))
        pth[i, :, :, n_in].copy_(pa["dlogp"])
        if s.train:
            pth[i, :, :, n_in + 1].copy_(pa["E"])
            pth[i, :, :, n_in + 2].copy_(pa["n"])
        grads[i].copy_(res[3])
        if with_z0:
            gz[i].copy_(res[4].t())                        # (the single call has added its own tail)
        return dict(res[-1]["stats"]), res[-1]["steps"]

    _finish(icnf, info, steps, None, rerun)
    icnf._record = None
    icnf.last_stats = info["stats"][0]
    path = _path_rows_many(s.train, n_in, pth, sv, info["steps"])
    path["logq"] = _logq_path(zr, path["dlogp"], n_in)
    out = (xo.permute(0, 2, 1), lq, path, grads)
    return out + ((gz.permute(0, 2, 1), info) if with_z0 else (info,))


# ---------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _autograd_inference_many():
    import torch

    class _InferencePathMany(torch.autograd.Function):
        @staticmethod
        def forward(ctx, icnf, mode, xs, ps, eps, saveat):
            logpx, (E, n, A), path, info = inference_path_many(icnf, mode, xs.detach(), ps.detach(), None, saveat=saveat, eps=eps)
            icnf.last_forward_info = info
            ctx.icnf, ctx.mode, ctx.saveat = icnf, mode, saveat
            ctx.train = "E" in path
            ctx.xs, ctx.ps, ctx.eps = xs.detach(), ps.detach().clone(), eps
            ctx.set_materialize_grads(False)
            outs = [logpx, E.clone(), n.clone(), A.clone(), path["z"].clone(), path["dlogp"].clone()]
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
            res = inference_path_vjp_many(icnf, ctx.mode, ctx.xs, ctx.ps, None, saveat=ctx.saveat, cot=(g_logpx, (g_E, g_n, g_A)),
                                          path_cot=pc, eps=ctx.eps, with_x=bool(need_x))
            # (the backward launch's own outputs: compared with the forward's in the tests)
            icnf.last_backward_logpx, icnf.last_backward_path, icnf.last_backward_info = res[0], res[2], res[-1]
            gx = None
            if need_x:
                gx = res[4] if ctx.xs.dim() == 3 else res[4].sum(dim=0)    # (a shared data set collects every member's)
            return None, None, gx, res[3] if need_ps else None, None, None

    return _InferencePathMany


def differentiable_inference_path_many(icnf: ICNF, mode, xs, ps, st=None, *, saveat, eps=None, bases=None):
    """``inference_path_many`` as a differentiable function of ``ps`` (M, n_params) and, when it requires grad, ``xs``: returns
    ``(logpx, (E, n, A), path)`` attached to the autograd graph, ``path`` a dict with ``t``, ``z`` (M, K, n_in, B), ``dlogp``
    (M, K, B) and in TrainMode ``E``, ``n``.  The forward is the one-launch ``inference_path_many`` with the probes settled once;
    the backward is ONE ``inference_path_vjp_many`` with the same draws (``icnf.last_forward_info`` / ``last_backward_info``
    keep the two calls' ``info``).  As for ``differentiable_inference_path``, the backward launch solves again."""
    _no_bases("differentiable_inference_path_many", bases)
    box = {}

    def saveat_check(M, B):
        box["sv"] = check_saveat_many(saveat, icnf.tspan, M)
        return ()

    s = _settle_density(icnf, mode, xs.detach() if _is_torch(xs) else xs, ps, eps, None, "differentiable_inference_path_many",
                        "differentiable_inference_path", cot_rows=saveat_check, steer=False)
    eps = s.er.permute(0, 2, 1) if s.er is not None else None
    outs = _autograd_inference_many().apply(icnf, mode, xs, ps, eps, box["sv"])
    path = {"t": box["sv"], "z": outs[4], "dlogp": outs[5]}
    if len(outs) > 6:
        path["E"], path["n"] = outs[6], outs[7]
    return outs[0], (outs[1], outs[2], outs[3]), path


@functools.lru_cache(maxsize=None)
def _autograd_generate_many():
    import torch

    class _GeneratePathMany(torch.autograd.Function):
        @staticmethod
        def forward(ctx, icnf, mode, ps, z0, eps, saveat):
            n = z0.shape[2]
            xs, logq, path, info = generate_path_many(icnf, mode, ps.detach(), None, n, saveat=saveat, z0=z0.detach(), eps=eps)
            icnf.last_forward_info = info
            ctx.icnf, ctx.mode, ctx.saveat = icnf, mode, saveat
            ctx.train = "E" in path
            ctx.ps, ctx.z0, ctx.eps = ps.detach().clone(), z0.detach(), eps
            ctx.set_materialize_grads(False)
            outs = [xs.clone(), logq, path["z"].clone(), path["logq"]]
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
                raise NotImplementedError("differentiable_generate_path_many: E_path and n_path are not outputs of sampling (no cotangent)")
            res = generate_path_vjp_many(icnf, ctx.mode, ctx.ps, None, ctx.z0.shape[2], saveat=ctx.saveat,
                                         cot=(g_x, g_logq) if (g_x is not None or g_logq is not None) else None,
                                         path_cot={"z": g_z, "logq": g_lq}, z0=ctx.z0, eps=ctx.eps, with_z0=bool(need_z0))
            icnf.last_backward_xs, icnf.last_backward_logq, icnf.last_backward_path, icnf.last_backward_info = res[0], res[1], res[2], res[-1]
            return None, None, res[3] if need_ps else None, res[4].contiguous() if need_z0 else None, None, None

    return _GeneratePathMany


def differentiable_generate_path_many(icnf: ICNF, mode, ps, st=None, n: int = 1, *, saveat, z0=None, eps=None, bases=None):
    """``generate_path_many`` as a differentiable function of ``ps`` (M, n_params) and of a ``z0`` (M, n_in, n) that requires grad:
    returns ``(xs, logq, path)`` attached to the autograd graph, ``path`` a dict with ``t``, ``z`` (M, K, n_in, n), ``logq``
    (M, K, n) and in TrainMode ``E``, ``n`` (running integrals: no outputs of sampling, they take no cotangent).  The forward is
    the one-launch ``generate_path_many`` with the draws kept; the backward is ONE ``generate_path_vjp_many``."""
    _no_bases("differentiable_generate_path_many", bases)
    box = {}
    t0, t1 = icnf.tspan

    def saveat_check(M, nn):
        box["sv"] = check_saveat_many(saveat, (t1, t0), M)
        return ()

    s = _settle_sampling(icnf, mode, ps, n, z0.detach() if _is_torch(z0) else z0, eps, None, "differentiable_generate_path_many",
                         "differentiable_generate_path", cot_pair=saveat_check, steer=False)
    if not (z0 is not None and z0.requires_grad):          # (a z0 that asks for a gradient stays the caller's tensor)
        z0 = s.zr.permute(0, 2, 1)
    outs = _autograd_generate_many().apply(icnf, mode, ps, z0, s.er.permute(0, 2, 1), box["sv"])
    path = {"t": box["sv"], "z": outs[2], "logq": outs[3]}
    if len(outs) > 4:
        path["E"], path["n"] = outs[4], outs[5]
    return outs[0], outs[1], path
