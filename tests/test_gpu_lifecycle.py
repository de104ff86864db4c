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


# ---- what a call leaves behind for the calls that may follow it -----------------------------------------------------------------
def _probe(ic, d, B, seen):
    """The five follow-up calls at batch B, in this order: cnf_grad_x, cnf_grad_ys, base_logpdf_pullback (which change nothing),
    then inference_pullback and generate_pullback (an accepted one is a backward pass: it leaves its own d / d u(t0) and d / d ys
    behind).  Returns the accepted ones as a string of their letters; `seen` remembers every accepted result under what it
    must be a result OF (the caller's label), and a second result under one label must repeat the first bit for bit."""
    l, h = _lib.lib(), ic.handle()
    st = torch.cuda.current_stream().cuda_stream
    ok, got = "", {}
    gx, gy = torch.empty(B * ic.nvars, device="cuda"), torch.empty(B * ic.n_cond, device="cuda")
    for key, rc, out in (("x", l.cnf_grad_x(h, gx.data_ptr(), B, st), gx.view(B, ic.nvars).t()),
                         ("y", l.cnf_grad_ys(h, gy.data_ptr(), B, st), gy.view(B, ic.n_cond).t())):
        assert rc in (_lib.OK, _lib.ERR_BAD_ARG), (key, rc)
        if rc == _lib.OK:
            got[key] = _np(out)
    w = torch.full((B,), -1.0 / B, device="cuda")
    for key, call in (("b", lambda: cnf.base_logpdf_pullback(ic, w)),
                      ("i", lambda: cnf.inference_pullback(ic, d["cot"], with_ys=True)[0]),
                      ("g", lambda: cnf.generate_pullback(ic, (d["cot"][:ic.nvars], d["cot"][3]), with_ys=True)[0])):
        try:
            got[key] = _np(call())
        except cnf.CNFError as e:
            assert e.status == _lib.ERR_BAD_ARG, (key, e.status)
    for key, v in got.items():
        ok += key
        label = d["labels"].get(key)
        if label in seen:
            _same(v, seen[label], f"{label} again")
        elif label is not None:
            seen[label] = v
    return ok


@pytest.mark.parametrize("mode", [TRAIN, TEST], ids=["train", "test"])
def test_what_each_call_leaves_behind(mode):
    """One handle through every event that begins or ends a piece of what the gradient calls leave on it, and after each event
    which of the five follow-up calls it accepts (x: cnf_grad_x, y: cnf_grad_ys, b: base_logpdf_pullback, i: inference_pullback,
    g: generate_pullback; every other answer must be ERR_BAD_ARG).  The expected strings are the table of csrc/cnf_record.h.
    Besides the nine events there are two re-recordings (marked +), so that set_params and set_cond find something to end."""
    n = 4
    base = cnf.LearnableNormal(torch.linspace(-0.2, 0.3, n).cuda(), std=torch.linspace(0.7, 1.4, n).cuda())
    ic = _model(WAVE_NET, n, n_cond=2, kernel="generic", basedist=base)
    B, B2 = 5, 7
    d, d2 = _inputs(ic, B), _inputs(ic, B2)
    eps = lambda dd: dd["eps"] if mode is TRAIN else None
    seen = {}

    def record(dd):
        return cnf.inference_record(ic, mode, *_args(ic, dd), eps=eps(dd))

    def rearm():
        record(d)
        cnf.inference_pullback(ic, d["cot"], with_ys=True)

    def check(event, want, dd, nB, **labels):
        dd["labels"] = labels
        got = _probe(ic, dd, nB, seen)
        print(f"after {event}, B = {nB}: accepted '{got}', expected '{want}'")
        assert got == want, (event, nB, got, want)

    out = cnf.loss_and_grad(ic, mode, *_args(ic, d), eps=eps(d), with_x=True, with_ys=True)
    seen["gx of the loss"], seen["gy of the loss"] = _np(out[2]), _np(out[3])
    check("1 loss_and_grad", "xyb", d, B, x="gx of the loss", y="gy of the loss", b="base at the final state")
    record(d)                    # a solve ends the LOSS record, not what the backward pass left; the pullback is a new backward pass
    check("2 inference_record", "xybi", d, B, x="gx of the loss", y="gy of the loss", b="base at the final state", i="pullback")
    out = cnf.inference_pullback(ic, d["cot"], with_x=True, with_ys=True)
    _same(_np(out[0]), seen["pullback"], "3 inference_pullback against the probe's")
    seen["gx of the pullback"], seen["gy of the pullback"] = _np(out[1]), _np(out[2])
    check("3 inference_pullback", "xybi", d, B, x="gx of the pullback", y="gy of the pullback", b="base at the final state", i="pullback")
    gen = dict(ys=d["ys"], z0=d["xs"], eps=eps(d))
    cnf.generate_record(ic, mode, d["ps"], None, B, **gen)
    check("4 generate_record", "bg", d, B, b="base at z0", g="sampling pullback")
    out = cnf.generate_pullback(ic, (d["cot"][:n], d["cot"][3]), with_ys=True)
    _same(_np(out[0]), seen["sampling pullback"], "5 generate_pullback against the probe's")
    seen["gy of the sampling pullback"] = _np(out[1])
    check("5 generate_pullback", "ybg", d, B, y="gy of the sampling pullback", b="base at z0", g="sampling pullback")
    cnf.inference(ic, mode, *_args(ic, d), eps=eps(d))
    check("6 inference", "y", d, B, y="gy of the sampling pullback")
    rearm()                      # +
    d["ps"] = d["ps"].clone()    # (another tensor with the same values: uploaded again)
    ic.set_params(d["ps"])
    check("7 set_params", "xy", d, B, x="gx of the pullback", y="gy of the pullback")
    rearm()                      # +
    d["ys"] = d["ys"].clone()
    ic.set_cond(d["ys"], B)
    check("8 set_cond", "xy", d, B, x="gx of the pullback", y="gy of the pullback")
    d2["ps"] = d["ps"]
    record(d2)                   # (within the capacity the first call reserved: nothing is cleared)
    check("9 a larger record, the smaller batch", "xy", d, B, x="gx of the pullback", y="gy of the pullback")
    check("9 a larger record, its own batch", "bi", d2, B2, b="base at the larger final state", i="larger pullback")
    check("9 ... and after its pullback", "xybi", d2, B2, b="base at the larger final state", i="larger pullback")
    ic.close()
