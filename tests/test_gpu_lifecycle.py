"""The life of a handle's buffers on the MI355X: every device and pinned allocation of a handle is grown, reused without a
reallocation, and freed, and nothing computed depends on which of these happened.  One handle is driven through B = 32, 200
and 32 again on each route; every result is compared BIT FOR BIT with that of a fresh handle built for that B alone on the same
inputs (the routes here reduce in a fixed order).  The smallest networks that reach each buffer."""
import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib, configs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = dict(configs.README_TOLERANCES)
BS = (32, 200, 32)                       # growth, then reuse within capacity
TRAIN, TEST = cnf.TrainMode(), cnf.TestMode()

WAVE_NET = ((4, 8, 4), ("tanh", "identity"))                  # k_solve_wave and its in-launch gradient
DEEP_NET = ((6, 24, 24, 6), ("tanh", "tanh", "identity"))     # the LDS-plan MFMA kernels / the generic ones


def _model(net, nvars, naugs=0, n_cond=0, kernel="auto", sol_kwargs=None, basedist=None):
    dims, acts = net
    dims = (dims[0] + n_cond,) + tuple(dims[1:])
    nn = cnf.Chain(*[cnf.Dense(i, o, a) for i, o, a in zip(dims[:-1], dims[1:], acts)])
    return cnf.construct(cnf.CondRNODE if n_cond else cnf.RNODE, nn, nvars, naugs, compute_mode=cnf.HIPVecJacMatrixMode(kernel),
                         lambda3=1e-2 if naugs else 0.0, sol_kwargs=sol_kwargs or TOL, rng=0, basedist=basedist)


def _inputs(ic, B, host=False):
    """xs, eps, ys (None unless conditional), ps, and a cotangent of the four outputs: seeded by the model and B alone."""
    rng = np.random.default_rng(1000 * ic.nn.dims[1] + B)
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    n_in = ic.nvars + ic.naugmented
    out = dict(xs=f32(ic.nvars, B), eps=f32(n_in, B), ys=f32(ic.n_cond, B) if ic.n_cond else None, cot=f32(4, B))
    prng = np.random.default_rng(7)
    out["ps"] = (0.3 * prng.standard_normal(ic.nn.n_params_internal)).astype(np.float32)
    if not host:
        out = {k: None if v is None else torch.from_numpy(v).cuda() for k, v in out.items()}
    return out


def _np(x):
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in _np(y)]
    if x is None:
        return []
    return [x.detach().cpu().numpy().copy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float32).copy()]


def _args(ic, d):
    return (d["xs"], d["ys"], d["ps"], {}) if ic.n_cond else (d["xs"], d["ps"], {})


def _same(got, ref, what):
    assert len(got) == len(ref) and len(got) > 0, what
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and np.isfinite(g).all(), (what, i)
        print(f"{what}[{i}]: max |diff| {np.abs(g - r).max() if g.size else 0.0:.3e}")
        assert np.array_equal(g, r), (what, i, float(np.abs(g - r).max()))


def _lifecycle(make, run, what, batches=BS):
    """`run(ic, B)` (a list of arrays) on ONE handle over `batches`, each against a fresh handle's (computed once per B)."""
    grown, fresh = make(), {}
    try:
        for B in batches:
            if B not in fresh:
                ic = make()
                try:
                    fresh[B] = run(ic, B)
                finally:
                    ic.close()
            _same(run(grown, B), fresh[B], f"{what}, B = {B}")
    finally:
        grown.close()
    return fresh


# ---- the wave routes: inference, the in-launch gradients, submit / collect ----------------------------------------------------
def _run_wave(ic, B):
    d = _inputs(ic, B)
    a = _args(ic, d)
    out = _np(cnf.inference(ic, TRAIN, *a, eps=d["eps"]))
    assert ic.last_stats["kernel_used"] == _lib.KERNEL_MFMA and ic.last_stats["launches"] == 1
    out += _np(cnf.inference(ic, TEST, *a))
    out += _np(cnf.loss_and_grad(ic, TRAIN, *a, eps=d["eps"], with_x=True))
    assert ic.last_stats["launches"] == 2                    # the solve with its gradient, the sum of the waves' partials
    out += _np(cnf.loss_and_grad(ic, TEST, *a, with_x=True))
    sub = cnf.loss_and_grad_submit(ic, TRAIN, *a, eps=d["eps"])
    cnf.loss_and_grad_collect(ic)
    torch.cuda.synchronize()
    return out + _np(sub)


def test_wave_routes():
    _lifecycle(lambda: _model(WAVE_NET, 4), _run_wave, "wave")


# ---- the LDS-plan MFMA solve and k_adj_mfma; more steps than the trajectory store first holds ----------------------------------
def _run_mfma_fixed(ic, B):
    d = _inputs(ic, B)
    out = _np(cnf.loss_and_grad(ic, TRAIN, *_args(ic, d), eps=d["eps"], with_x=True))
    assert ic.last_stats["kernel_used"] == _lib.KERNEL_MFMA
    assert len(ic.last_steps) == 80                          # > 64 slots: the store overflowed, grew, and the solve ran again
    return out


def test_mfma_gradient_through_a_trajectory_that_outgrows_its_store():
    _lifecycle(lambda: _model(DEEP_NET, 4, 2, sol_kwargs=dict(adaptive=False, dt=1.0 / 80)), _run_mfma_fixed, "mfma, 80 steps")


# ---- the generic routes on the same network ----------------------------------------------------------------------------------
def _run_generic(ic, B):
    d = _inputs(ic, B)
    a = _args(ic, d)
    out = _np(cnf.loss_and_grad(ic, TEST, *a, with_x=True))                    # k_adj_test and its scratch
    assert ic.last_stats["kernel_used"] == _lib.KERNEL_GENERIC
    for mode in (TRAIN, TEST):                                                  # the per-sample cotangent buffer
        out += _np(cnf.inference_record(ic, mode, *a, eps=d["eps"] if mode is TRAIN else None))
        out += _np(cnf.inference_pullback(ic, d["cot"], with_x=True))
    return out


def test_generic_routes():
    _lifecycle(lambda: _model(DEEP_NET, 4, 2, kernel="generic"), _run_generic, "generic")


def test_generic_record_pullback_then_a_larger_record():
    """record -> pullback -> larger-B record -> pullback on one handle, and the smaller record is gone afterwards."""
    ic, ref = _model(DEEP_NET, 4, 2, kernel="generic"), {}
    for B in (32, 200):
        f = _model(DEEP_NET, 4, 2, kernel="generic")
        d = _inputs(f, B)
        ref[B] = _np(cnf.inference_record(f, TRAIN, *_args(f, d), eps=d["eps"])) + _np(cnf.inference_pullback(f, d["cot"], with_x=True))
        f.close()
    for B in (32, 200):
        d = _inputs(ic, B)
        got = _np(cnf.inference_record(ic, TRAIN, *_args(ic, d), eps=d["eps"]))
        got += _np(cnf.inference_pullback(ic, d["cot"], with_x=True))
        got2 = _np(cnf.inference_pullback(ic, d["cot"], with_x=True))          # (a record may be pulled back more than once)
        _same(got, ref[B], f"record / pullback, B = {B}")
        _same(got2, got[-2:], f"second pullback, B = {B}")
    with pytest.raises(cnf.CNFError):
        cnf.inference_pullback(ic, _inputs(ic, 32)["cot"])
    ic.close()


# ---- a conditional model: the conditioning at two batch sizes, in both orders --------------------------------------------------
def _run_cond(ic, B):
    d = _inputs(ic, B)
    a = _args(ic, d)
    out = _np(cnf.inference(ic, TRAIN, *a, eps=d["eps"])) + _np(cnf.inference(ic, TEST, *a))
    return out + _np(cnf.loss_and_grad(ic, TRAIN, *a, eps=d["eps"], with_x=True))


@pytest.mark.parametrize("kernel", ["auto", "generic"])
def test_conditional_model(kernel):
    _lifecycle(lambda: _model(WAVE_NET, 4, n_cond=2, kernel=kernel), lambda ic, B: _run_cond(ic, B), f"cond, {kernel}")
    _lifecycle(lambda: _model(WAVE_NET, 4, n_cond=2, kernel=kernel), lambda ic, B: _run_cond(ic, B), f"cond, {kernel}, shrinking first",
               batches=(200, 32, 200))


# ---- the base distribution: set, cleared, set again with a dense covariance ----------------------------------------------------
def _set_base(ic, dist):
    h, l = ic.handle(), _lib.lib()
    if dist is None:
        _lib.check(l.cnf_set_basedist(h, 0, None, None, None, 0.0), h)
    else:
        _lib.check(l.cnf_set_basedist(h, dist.kind, dist.mean.ctypes.data, dist.whiten.ctypes.data, dist.chol.ctypes.data, dist.logconst), h)


def _run_base(ic, B):
    d = _inputs(ic, B)
    a = _args(ic, d)
    return _np(cnf.inference(ic, TRAIN, *a, eps=d["eps"])) + _np(cnf.loss_and_grad(ic, TRAIN, *a, eps=d["eps"], with_x=True))


def test_base_distribution_set_cleared_and_set_again():
    rng = np.random.default_rng(5)
    q = np.linalg.qr(rng.standard_normal((4, 4)))[0]
    diag = cnf.DiagNormal(rng.standard_normal(4), rng.uniform(0.5, 2.0, 4))
    dense = cnf.MvNormal(rng.standard_normal(4), q @ np.diag(rng.uniform(0.2, 5.0, 4)) @ q.T)
    ic = _model(WAVE_NET, 4, basedist=diag)                  # (its handle is created with the diagonal base)
    for i, (dist, B) in enumerate(((diag, 32), (None, 32), (dense, 32), (dense, 200), (None, 200), (diag, 32))):
        if i > 0:
            _set_base(ic, dist)
            ic.basedist = dist
        f = _model(WAVE_NET, 4, basedist=dist)
        ref = _run_base(f, B)
        f.close()
        _same(_run_base(ic, B), ref, f"basedist {dist!r}, B = {B}")
    ic.close()


# ---- host arrays: the *_host entry points and the staging area ------------------------------------------------------------------
def _run_host(ic, B):
    d = _inputs(ic, B, host=True)
    a = _args(ic, d)
    out = _np(cnf.inference(ic, TRAIN, *a, eps=d["eps"])) + _np(cnf.inference(ic, TEST, *a))
    out += _np(cnf.loss_and_grad(ic, TRAIN, *a, eps=d["eps"], with_x=True))
    return out + _np(cnf.loss_and_grad(ic, TEST, *a, with_x=True))


@pytest.mark.parametrize("n_cond", [0, 2])
def test_host_entry_points(n_cond):
    _lifecycle(lambda: _model(WAVE_NET, 4, n_cond=n_cond), _run_host, f"host arrays, n_cond = {n_cond}")


# ---- destroy and create again ----------------------------------------------------------------------------------------------------
def test_destroy_and_recreate():
    """The handle that grew every buffer of the MFMA and generic gradient paths is destroyed; a new one of the same model works."""
    ic = _model(DEEP_NET, 4, 2)
    fresh = _model(DEEP_NET, 4, 2)
    d = _inputs(fresh, 32)
    ref = _np(cnf.inference(fresh, TRAIN, *_args(fresh, d), eps=d["eps"]))
    fresh.close()
    for B in (32, 200):
        g = _inputs(ic, B)
        a = _args(ic, g)
        cnf.loss_and_grad(ic, TRAIN, *a, eps=g["eps"])
        cnf.loss_and_grad(ic, TEST, *a)
        cnf.inference_record(ic, TRAIN, *a, eps=g["eps"])
        cnf.inference_pullback(ic, g["cot"])
        cnf.inference(ic, TRAIN, *_args(ic, _inputs(ic, B, host=True)), eps=g["eps"].cpu().numpy())
    ic.close()
    assert ic._handle is None
    _same(_np(cnf.inference(ic, TRAIN, *_args(ic, d), eps=d["eps"])), ref, "after destroy and re-create")     # (a new handle, made on demand)
    ic.close()
