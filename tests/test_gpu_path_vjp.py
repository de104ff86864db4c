"""Differentiable flow paths on the device: ``inference_path_vjp`` / ``generate_path_vjp`` (cnf_inference_path_vjp,
cnf_generate_path_vjp: the PATH forms of the per-sample-cotangent gradient kernel) and the two autograd functions over them.

Reference: tests/path_vjp_ref.py replaying, in float64, the steps the call itself accepted (``info["steps"]``), so whichever
bracket the device used for a save time is the one checked.  Gradients are held with ``vjp_ref.assert_vjp`` unchanged
(``rtol = max(1e-4, 8 floor)`` per parameter block and for grad_x / grad_z0, the floor from the float32 run of the same
reference); the path, ``logpx`` / ``xs`` and ``logq`` at the bar of tests/test_gpu_path.py (helpers.assert_parity with the dlogp
row as ``trace_row``, widened by tests/envelope.py's rule only where the float32 replay itself misses it).  The save times are
fractions of the steps a first call reports, turned into times here.

Measured on the MI355X: of the 540 block checks of the case sweep 529 keep ``rtol`` = 1e-4, the device off by at most 1.1e-5 of the
block's scale; the other 11 are the stiff 16-48-16 case that rejects attempts, sampling direction, where the float32 reference
itself is off by up to 9.3e-5 (a cotangent on ``logq`` alone: ``grad_z0`` is the difference of two larger terms), the bar widens to
at most 7.5e-4 under the cap of 1e-3 and the device is off by 7.9e-5.  The worst path slice is at 0.52 of its bar.  Without a path
cotangent the gradients are the ensemble vjp's of one member to 0 .. 3.0e-7 of their scale; the backward launch's path differs
from ``inference_path``'s by at most 1.1e-6 and its ``logq`` path from ``generate_path``'s by at most 1.9e-6 (absolute).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import envelope as Env
from tests import helpers
from tests import path_vjp_ref as R
from tests import vjp_ref as V
from tests.helpers import assert_parity, make_icnf, parity_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
BY = {c.name: c for c in R.CASES}


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _mode(train):
    return cnf.TrainMode() if train else cnf.TestMode()


def _icnf(case, **kw):
    sol = dict(case.sol_kw)
    sol.update(kw)
    return make_icnf(cnf, case.cfg, jvp=case.jvp, kernel="mfma", sol_kwargs=sol)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return R.inputs(BY[name])


def _span(case, sampling):
    return (case.cfg.tspan[1], case.cfg.tspan[0]) if sampling else case.cfg.tspan


def _pc_dev(pc):
    return None if pc is None else {k: _dev(v) for k, v in pc.items()}


def _state_path(path, train):
    """The dict of rows the calls return -> K x D x B numpy."""
    rows = [_np(path["z"]), _np(path["dlogp"])[:, None, :]]
    if train:
        rows += [_np(path["E"])[:, None, :], _np(path["n"])[:, None, :]]
    return np.concatenate(rows, axis=1)


def _call(icnf, case, sampling, sv, cot, pc):
    """One ``*_path_vjp`` call -> dict of numpy results."""
    flat, xs, z0, eps = _inputs(case.name)
    mode = _mode(case.train)
    if sampling:
        c = None if cot is None else (_dev(cot[0]), _dev(cot[1]))
        x, lq, path, g, gin, info = cnf.generate_path_vjp(icnf, mode, _dev(flat), {}, case.B, saveat=sv, cot=c, path_cot=_pc_dev(pc),
                                                           z0=_dev(z0), eps=_dev(eps), with_z0=True)
        out = {"x": _np(x), "logq": _np(lq), "logq_path": _np(path["logq"])}
    else:
        c = None if cot is None else (_dev(cot[0]), (_dev(cot[1]), _dev(cot[2]), _dev(cot[3])))
        lp, rg, path, g, gin, info = cnf.inference_path_vjp(icnf, mode, _dev(xs), _dev(flat), {}, saveat=sv, cot=c, path_cot=_pc_dev(pc),
                                                             eps=_dev(eps) if case.train else None, with_x=True)
        out = {"logpx": _np(lp), "regs": np.stack([_np(r) for r in rg])}
    out.update(path=_state_path(path, case.train), grad=_np(g), gin=_np(gin), info=info, steps=info["steps"])
    assert info["stats"]["launches"] == (4 if sampling else 2), info["stats"]
    assert len(info["steps"][0]) == info["stats"]["naccept"] > 0
    return out


def _reference(case, sampling, sv, cot, pc, steps, dtype):
    flat, xs, z0, eps = _inputs(case.name)
    e = eps if case.train else None
    ts, hs = steps
    if sampling:
        cz, cl = cot if cot is not None else (None, None)
        z, lq, path, lqp, g, gin = R.generate(case.cfg, flat, z0, e, cz, cl, pc, ts, hs, sv, case.train, dtype)
        return {"x": z[:case.cfg.nvars], "logq": lq, "logq_path": lqp, "path": path, "grad": g, "gin": gin}
    out, path, g, gin = R.inference(case.cfg, flat, xs, e, cot, pc, ts, hs, sv, case.train, dtype)
    return {"logpx": out[0], "regs": out[1:], "path": path, "grad": g, "gin": gin}


def _check_path(got, ref, r32, n_in, what):
    """Every slice at the bar of tests/test_gpu_path.py."""
    K = len(ref)
    worst = max(parity_err(got[k], ref[k], trace_row=n_in) for k in range(K))
    rtol = helpers.RTOL
    if worst > 1.0:
        floor = helpers.RTOL * max(parity_err(r32[k], ref[k], trace_row=n_in) for k in range(K))
        rtol = Env.rtol_of(floor)
        print(f"{what}: {worst:.2f} x the default bar; float32 floor {floor:.3g} -> rtol {rtol:.3g}")
        assert rtol <= Env.RTOL_CAP, (what, floor)
    print(f"{what}: worst slice {worst:.3f} x the default bar")
    for k in range(K):
        assert_parity(got[k], ref[k], f"{what} slice {k}", rtol=rtol, trace_row=n_in)


def _check(case, sampling, got, sv, cot, pc, what, grads=True):
    r64 = _reference(case, sampling, sv, cot, pc, got["steps"], np.float64)
    r32 = _reference(case, sampling, sv, cot, pc, got["steps"], np.float32)
    n_in = case.cfg.n_in
    _check_path(got["path"], r64["path"], r32["path"], n_in, what)
    if sampling:
        assert_parity(got["x"], r64["x"], f"{what} xs")
        assert_parity(got["logq"], r64["logq"], f"{what} logq")
        assert_parity(got["logq_path"], r64["logq_path"], f"{what} logq along the path")
    else:
        assert_parity(got["logpx"], r64["logpx"], f"{what} logpx")
        if case.train:
            assert_parity(got["regs"], r64["regs"], f"{what} regs")
    if grads:
        V.assert_vjp(got["grad"], got["gin"], (r64["grad"], r64["gin"]), (r32["grad"], r32["gin"]), case.cfg.net, what)
    return r64


@pytest.mark.parametrize("sampling", [False, True], ids=["inference", "sampling"])
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_every_cotangent_set_matches_the_float64_adjoint_on_the_calls_own_steps(case, sampling):
    icnf = _icnf(case)
    span = _span(case, sampling)
    assert cnf.path_vjp_max_batch(icnf, _mode(case.train)) >= case.B
    first = _call(icnf, case, sampling, np.asarray([span[1]], np.float32), None, None)       # the steps, for the save times
    ts, hs = first["steps"]
    assert not first["grad"].any() and not first["gin"].any()                                 # (no cotangent at all: zeros)
    if "rejects" in case.name:
        assert first["info"]["stats"]["nreject"] >= 1, first["info"]["stats"]
    sv = R.save_times(case, ts, hs, span, "mixed")
    names = R.cot_sets(case, sampling)
    assert names[0] == "terminal" and names[-1] == "all" and len(names) >= 4
    for name in names:
        cot, pc = R.path_cotangents(case, len(sv), sampling, name)
        got = _call(icnf, case, sampling, sv, cot, pc)
        assert np.array_equal(got["steps"][0], ts) and np.array_equal(got["steps"][1], hs)    # (the cotangents move no step)
        kinds = {k for k, _, _ in R.brackets(span, got["steps"][0], got["steps"][1], sv)}
        assert kinds == {R.START, R.END, R.INTERIOR}, kinds
        _check(case, sampling, got, sv, cot, pc, f"path vjp {case.name} {'sampling' if sampling else 'inference'} cot {name}")
    # more save times than steps, and the end alone
    for which in ("k40", "end"):
        svk = R.save_times(case, ts, hs, span, which)
        cot, pc = R.path_cotangents(case, len(svk), sampling, "all")
        got = _call(icnf, case, sampling, svk, cot, pc)
        _check(case, sampling, got, svk, cot, pc, f"path vjp {case.name} {'sampling' if sampling else 'inference'} {which}")
    helpers.note(f"path vjp {case.name} {'sampling' if sampling else 'inference'}: {len(ts)} steps, "
                 f"{first['info']['stats']['nreject']} rejected")
    icnf.close()


def _block_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) / V.scale(b)


@pytest.mark.parametrize("name", ["path-readme-vjp-B33", "path-regr-test-B17", "path-regr-jvp-B33"])
def test_without_a_path_cotangent_it_is_the_ensemble_vjp_of_one_member(name):
    """``path_cot=None`` gives what ``inference_vjp_many`` / ``generate_vjp_many`` give for M = 1 -- another instantiation of the
    same kernel on the same forward half: the same accepted steps, outputs at the parity bar, gradients at 1e-4 of their scale."""
    case = BY[name]
    icnf = _icnf(case)
    flat, xs, z0, eps = _inputs(name)
    mode = _mode(case.train)
    e = _dev(eps)[None] if case.train else None
    worst = 0.0
    for sampling in (False, True):
        span = _span(case, sampling)
        cot, _ = R.path_cotangents(case, 1, sampling, "terminal")
        got = _call(icnf, case, sampling, np.asarray([span[1]], np.float32), cot, None)
        if sampling:
            x, lq, g, gz, info = cnf.generate_vjp_many(icnf, mode, _dev(flat)[None], {}, case.B, (_dev(cot[0])[None], _dev(cot[1])[None]),
                                                       z0=_dev(z0)[None], eps=_dev(eps)[None], with_z0=True, with_steps=True)
            assert_parity(got["x"], _np(x[0]), f"{name} xs"); assert_parity(got["logq"], _np(lq[0]), f"{name} logq")
        else:
            lp, rg, g, gz, info = cnf.inference_vjp_many(icnf, mode, _dev(xs)[None], _dev(flat)[None], {},
                                                         (_dev(cot[0])[None], tuple(_dev(c)[None] for c in cot[1:])), eps=e, with_x=True,
                                                         with_steps=True)
            assert_parity(got["logpx"], _np(lp[0]), f"{name} logpx")
        assert np.array_equal(info["steps"][0], got["steps"][1])
        worst = max(worst, _block_err(got["grad"], _np(g[0])), _block_err(got["gin"], _np(gz[0])))
    helpers.note(f"path vjp without a path cotangent vs the ensemble vjp, {name}: gradients differ by {worst:.2e} of their scale")
    assert worst <= V.RTOL, worst
    icnf.close()


def test_a_z_cotangent_at_t_end_is_generate_vjp_manys_g_x():
    case = BY["path-regr-vjp-B17-rejects"]
    icnf = _icnf(case)
    flat, xs, z0, eps = _inputs(case.name)
    span = _span(case, True)
    (cz, _), _ = R.path_cotangents(case, 1, True, "terminal")
    got = _call(icnf, case, True, np.asarray([span[1]], np.float32), None, {"z": cz[None]})
    x, lq, g, gz, info = cnf.generate_vjp_many(icnf, _mode(True), _dev(flat)[None], {}, case.B, (_dev(cz)[None], None), z0=_dev(z0)[None],
                                               eps=_dev(eps)[None], with_z0=True, with_steps=True)
    assert np.array_equal(info["steps"][0], got["steps"][1])
    assert np.array_equal(got["path"][0][:case.cfg.nvars], got["x"])       # the slice at t_end is the final state, bit for bit
    err = max(_block_err(got["grad"], _np(g[0])), _block_err(got["gin"], _np(gz[0])))
    helpers.note(f"path vjp: z cotangent at t_end vs generate_vjp_many's g_x: {err:.2e} of the gradient's scale")
    assert err <= V.RTOL, err
    icnf.close()


@pytest.mark.parametrize("name", ["path-readme-vjp-B33", "path-regr-test-B17"])
def test_autograd_is_one_path_vjp_launch(name):
    """``torch.autograd.grad`` of ``sum(w z_path) + sum(v dlogp_path) + sum(c logpx)`` through ``differentiable_inference_path`` is
    ONE ``inference_path_vjp`` with those cotangents -- the same launch on the same inputs, so to rounding of nothing: 1e-6 --,
    likewise for sampling into ``ps`` and a ``z0`` that requires grad; and the path of the backward launch agrees with the
    forward's (``inference_path`` / ``generate_path``: the plain PATH form, whose evaluations use the exp2 / rcp tanh) at the
    parity bar -- DESIGN 4.4 has the measured figure."""
    case = BY[name]
    icnf = _icnf(case)
    flat, xs, z0, eps = _inputs(name)
    mode = _mode(case.train)
    n_in = case.cfg.n_in
    first = _call(icnf, case, False, np.asarray([case.cfg.tspan[1]], np.float32), None, None)
    sv = R.save_times(case, *first["steps"], case.cfg.tspan, "mixed")
    cot, pc = R.path_cotangents(case, len(sv), False, "all")
    pc = {k: v for k, v in pc.items() if k in ("z", "dlogp")}
    cot = cot * np.array([1, 0, 0, 0], np.float32)[:, None]
    pt, xt = _dev(flat).requires_grad_(True), _dev(xs).requires_grad_(True)
    lp, regs, path = cnf.differentiable_inference_path(icnf, mode, xt, pt, {}, saveat=sv, eps=_dev(eps) if case.train else None)
    obj = (_dev(pc["z"]) * path["z"]).sum() + (_dev(pc["dlogp"]) * path["dlogp"]).sum() + (_dev(cot[0]) * lp).sum()
    g_ps, g_xs = torch.autograd.grad(obj, (pt, xt))
    got = _call(icnf, case, False, sv, cot, pc)
    err = max(_block_err(_np(g_ps), got["grad"]), _block_err(_np(g_xs), got["gin"]))
    assert err <= 1e-6, err
    fwd = np.concatenate([_np(path["z"]), _np(path["dlogp"])[:, None, :]], axis=1)
    diff = float(np.abs(fwd - got["path"][:, :n_in + 1]).max())
    helpers.note(f"path vjp {name}: the backward launch's path differs from inference_path's by at most {diff:.2e} (absolute)")
    for k in range(len(sv)):
        assert_parity(got["path"][k][:n_in + 1], fwd[k], f"{name}: backward launch's path vs inference_path's, slice {k}", trace_row=n_in)
    assert_parity(got["logpx"], _np(lp), f"{name}: backward launch's logpx vs the forward's")
    # sampling: into ps and a z0 that requires grad
    span = _span(case, True)
    first = _call(icnf, case, True, np.asarray([span[1]], np.float32), None, None)
    sv = R.save_times(case, *first["steps"], span, "mixed")
    (cz, cl), pc = R.path_cotangents(case, len(sv), True, "all")
    pt, zt = _dev(flat).requires_grad_(True), _dev(z0).requires_grad_(True)
    x, lq, path = cnf.differentiable_generate_path(icnf, mode, pt, {}, case.B, saveat=sv, z0=zt, eps=_dev(eps))
    obj = (_dev(pc["z"]) * path["z"]).sum() + (_dev(pc["logq"]) * path["logq"]).sum() + (_dev(cl) * lq).sum() + \
        (_dev(cz[:case.cfg.nvars]) * x).sum()
    g_ps, g_z0 = torch.autograd.grad(obj, (pt, zt))
    czx = np.zeros_like(cz)
    czx[:case.cfg.nvars] = cz[:case.cfg.nvars]
    got = _call(icnf, case, True, sv, (czx, cl), pc)
    err = max(_block_err(_np(g_ps), got["grad"]), _block_err(_np(g_z0), got["gin"]))
    assert err <= 1e-6, err
    diff = float(np.abs(_np(path["logq"]) - got["logq_path"]).max())
    helpers.note(f"path vjp {name}: the backward launch's logq path differs from generate_path's by at most {diff:.2e} (absolute)")
    assert_parity(got["logq_path"], _np(path["logq"]), f"{name}: backward launch's logq path vs generate_path's")
    assert_parity(got["x"], _np(x), f"{name}: backward launch's xs vs the forward's")
    icnf.close()


def test_edges_batch_above_the_capacity_and_a_solve_that_stops():
    case = BY["path-readme-vjp-B33"]
    icnf = _icnf(case)
    T = _mode(True)
    flat, xs, z0, eps = _inputs(case.name)
    cap = cnf.path_vjp_max_batch(icnf, T)
    assert cap >= 64 and cap % 16 == 0
    B = cap + 1
    t0, t1 = icnf.tspan
    before = icnf.rng.bit_generator.state
    with pytest.raises(NotImplementedError):
        cnf.inference_path_vjp(icnf, T, torch.zeros((1, B), device="cuda"), _dev(flat), {}, saveat=[t0, t1])
    with pytest.raises(NotImplementedError):
        cnf.generate_path_vjp(icnf, T, _dev(flat), {}, B, saveat=[t1, t0])
    assert icnf.rng.bit_generator.state == before
    # the C ABI: refused with nothing enqueued (the gradient buffer keeps its zeros), for B above the capacity and for the
    # generic kernel
    l, h = _lib.lib(), icnf.handle()
    n_in, D, K = 2, 5, 2
    g = torch.zeros(flat.size, device="cuda")

    def raw(B, opts):
        s = np.asarray([t0, t1], np.float32)
        x, e = torch.zeros(B, device="cuda"), torch.zeros(B * n_in, device="cuda")
        lp, rg, pth = torch.zeros(B, device="cuda"), torch.zeros(3 * B, device="cuda"), torch.zeros(K * B * D, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = l.cnf_inference_path_vjp(h, _lib.MODE_TRAIN, _dev(flat).data_ptr(), x.data_ptr(), e.data_ptr(), B, C.byref(opts),
                                      s.ctypes.data, K, None, None, lp.data_ptr(), rg.data_ptr(), pth.data_ptr(), g.data_ptr(), None,
                                      None, st)
        torch.cuda.synchronize()
        return rc, lp, pth

    opts = cnf.base_icnf._solve_opts(icnf, icnf.tspan)
    assert raw(B, opts)[0] == _lib.ERR_UNSUPPORTED and not g.any()
    generic = _lib.cnf_solve_opts.from_buffer_copy(opts)
    generic.kernel = _lib.KERNEL_GENERIC
    assert raw(32, generic)[0] == _lib.ERR_UNSUPPORTED and not g.any()
    assert l.cnf_path_vjp_steps(h, None, None, 0) == -1
    # a solve that maxiters stops: the error, NaN outputs, zero gradients
    short = _lib.cnf_solve_opts.from_buffer_copy(opts)
    short.maxiters = 2
    g.fill_(1.0)
    rc, lp, pth = raw(32, short)
    assert rc == _lib.ERR_MAXITERS
    assert not g.any() and bool(torch.isnan(lp).all()) and bool(torch.isnan(pth).all())
    assert l.cnf_path_vjp_steps(h, None, None, 0) == -1
    rc, lp, pth = raw(32, opts)
    assert rc == _lib.OK and bool(torch.isfinite(pth).all()) and l.cnf_path_vjp_steps(h, None, None, 0) > 0
    icnf.close()
    stopped = _icnf(case, maxiters=2)
    with pytest.raises(cnf.CNFError) as e:
        cnf.inference_path_vjp(stopped, T, _dev(xs), _dev(flat), {}, saveat=[t0, t1], eps=_dev(eps))
    assert e.value.status == _lib.ERR_MAXITERS
    stopped.close()
