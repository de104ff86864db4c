"""Differentiable ensembles on the device: ``inference_vjp_many`` (cnf_inference_vjp_many, the CW form of the ensemble gradient
kernel), ``differentiable_inference_many`` and ``EnsembleDist.log_prob``.

Reference: tests/ensemble_vjp_ref.py -- ``vjp_ref.vjp64`` replaying for every member the steps that member itself accepted on
the device (cnf_ensemble_steps), held with ``vjp_ref.assert_vjp`` unchanged (``rtol = max(1e-4, 8 floor)`` per parameter block
and for grad_x, the floor from ``vjp32``: tests/test_ensemble_vjp_host.py shows it is under a quarter of the bar on every case);
``logpx`` and the regularisers at tests/helpers.py's parity bar.  Everything else is exact: zeros, permutations, isolation,
repetition and splits are compared bit for bit.

Measured on the MI355X (the numbers also go to parity_report.json's notes).  The loss cotangent against
``loss_and_grad_many``: the accepted steps are the same bit for bit; the largest gradient difference is 6.5e-07 of the gradient's
scale (16-48-16, VJP; 3.1e-07 JVP, 6.1e-08 on 2-6-2) and 0 -- the same bits -- in TestMode, at B = 1 and on the 6-9-6 identity
network (bar 1e-4).  The backward launch's ``logpx`` against the forward's: NOT bit-identical -- the forward is the plain
ensemble form, whose evaluations use the exp2 / rcp tanh, the backward launch the gradient form, whose forward half uses the
2-ulp tanh its adjoint differentiates --; largest difference 3.3e-06 (weighted loss, 2-6-2) and 3.8e-06 (stacking, 16-48-16,
|logpx| ~ 20), a few percent of the parity bar.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from continuousnf.jl_amd import ensemble as ens_mod
from oracle import cnf_oracle as O
from tests import ensemble_vjp_ref as R
from tests import helpers
from tests import vjp_ref as V
from tests.helpers import assert_parity, make_icnf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
M = R.M
BY_NAME = {c.name: c for c in R.CASES}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _mode(train):
    return cnf.TrainMode() if train else cnf.TestMode()


def _icnf(case, **kw):
    return make_icnf(cnf, case.cfg, jvp=case.jvp, kernel="mfma", sol_kwargs=dict(case.sol_kw), **kw)


def _cot_arg(c):
    """(M, 4, B) numpy -> the tuple ``inference_vjp_many`` takes."""
    return _dev(c[:, 0]), (_dev(c[:, 1]), _dev(c[:, 2]), _dev(c[:, 3]))


def _vjp(icnf, case, ps, xs, eps, cot, t1="case", **kw):
    """-> (logpx (M, B), regs (M, 3, B), grads, grad_x (M, nvars, B), info), numpy."""
    t1 = (np.asarray(case.t1, np.float32) if case.t1 is not None else None) if isinstance(t1, str) else t1
    lp, rg, g, gx, info = cnf.inference_vjp_many(icnf, _mode(case.train), _dev(xs), _dev(ps), {}, _cot_arg(cot),
                                                 eps=_dev(eps) if case.train else None, t1=t1, with_x=True, with_steps=True, **kw)
    return lp.cpu().numpy(), torch.stack(list(rg), dim=1).cpu().numpy(), g.cpu().numpy(), gx.cpu().numpy(), info


@functools.lru_cache(maxsize=None)
def _reference(name, m, cot_key, dts, variant="plain"):
    """One member's float64 / float32 reference, computed once per (case, member, cotangent, steps)."""
    case = BY_NAME[name]
    ps, xs, eps = _inputs(name, variant)
    return R.reference(case, m, ps, xs, eps, _COTS[cot_key], list(dts))


_COTS = {}


def _ref(case, m, cot, dts, variant="plain"):
    key = (case.name, m, variant, cot.tobytes())
    _COTS[key] = cot
    return _reference(case.name, m, key, tuple(float(d) for d in dts), variant)


@functools.lru_cache(maxsize=None)
def _inputs(name, variant="plain"):
    case = BY_NAME[name]
    ps, xs, eps = R.inputs(case)
    if variant == "zero-norms":
        # member 0: eps = 0 in some columns (|eps'J| = 0 there); member 1: a zero last layer (zdot = 0: |zdot| = 0, and z_aug
        # stays 0: |z_aug| = 0); member 2: both
        cfg = case.cfg
        nw1 = cfg.net.dims[0] * cfg.net.dims[1] + cfg.net.dims[1]
        eps[0][:, : max(1, case.B // 4)] = 0
        eps[2][:, ::2] = 0
        ps[1][nw1:] = 0
        ps[2][nw1:] = 0
    return ps, xs, eps


def _check_member(case, m, lp, rg, g, gx, cot, dts, what, variant="plain"):
    out, r64, r32 = _ref(case, m, cot, dts, variant)
    assert_parity(lp, out[0], f"{what} logpx")
    if case.train:
        assert_parity(rg, out[1:], f"{what} regs")
    return out, r64, r32


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_each_member_and_cotangent_matches_the_float64_adjoint_on_its_own_steps(case):
    icnf = _icnf(case)
    assert cnf.ensemble_vjp_capacity(icnf, _mode(case.train), case.B) >= M
    ps, xs, eps = _inputs(case.name)
    cots = [R.cotangents(case, m) for m in range(M)]
    for name in cots[0]:
        cot = np.stack([cots[m][name] for m in range(M)])
        lp, rg, g, gx, info = _vjp(icnf, case, ps, xs, eps, cot)
        assert info["launches"] == 2 and info["calls"] == 1 and not info["rerun"], info
        assert (info["status"] == _lib.OK).all()
        for m in range(M):
            what = f"ensemble vjp {case.name} member {m} cot {name}"
            assert len(info["steps"][m]) == info["stats"][m]["naccept"] > 0, what
            _, r64, r32 = _check_member(case, m, lp[m], rg[m], g[m], gx[m], cot[m], info["steps"][m], what)
            V.assert_vjp(g[m], gx[m], r64, r32, case.cfg.net, what)
    if "rejects" in case.name:
        assert info["stats"][0]["nreject"] >= 1, info["stats"]
    if case.t1 is not None:
        assert [s["t_final"] for s in info["stats"]] == [float(np.float32(t)) for t in case.t1]
    helpers.note(f"ensemble vjp {case.name}: steps {[s['naccept'] for s in info['stats']]}, rejected "
                 f"{[s['nreject'] for s in info['stats']]}, {info['launches']} launches")
    icnf.close()


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_loss_cotangent_is_loss_and_grad_many(case):
    """The cotangent of the built-in loss against ``loss_and_grad_many`` on the same inputs: the losses recomputed from logpx and
    the regularisers agree (1e-5 max(1, |loss|), the bar of tests/test_gpu_ensemble.py), the gradients at the whole-gradient bar
    1e-4; the two terminal cotangents round differently ((z + ..) / B against (-g) z + ..), so bit equality is not asked for."""
    icnf = _icnf(case)
    ps, xs, eps = _inputs(case.name)
    t1 = np.asarray(case.t1, np.float32) if case.t1 is not None else None
    cot = np.stack([V.loss_cotangent(R.member_cfg(case, m), case.B, case.train) for m in range(M)]).astype(np.float32)
    lp, rg, g, gx, info = _vjp(icnf, case, ps, xs, eps, cot)
    val, grad, linfo = cnf.loss_and_grad_many(icnf, _mode(case.train), _dev(xs), _dev(ps), {}, eps=_dev(eps) if case.train else None,
                                              t1=t1, with_steps=True)
    grad = grad.cpu().numpy()
    worst = 0.0
    for m in range(M):
        assert np.array_equal(info["steps"][m], linfo["steps"][m])         # (one forward half: the same accepted steps)
        mine = O.loss(case.cfg, lp[m].astype(np.float64), tuple(r.astype(np.float64) for r in rg[m]), case.train)
        assert abs(mine - val[m]) <= 1e-5 * max(1.0, abs(val[m])), (case.name, m, mine, val[m])
        scale = np.abs(grad[m]).max() + np.sqrt(np.mean(grad[m].astype(np.float64) ** 2))
        err = np.abs(g[m] - grad[m]).max() / scale
        worst = max(worst, err)
        assert np.isfinite(g[m]).all() and err <= 1e-4, (case.name, m, err)
    print(f"loss cotangent vs loss_and_grad_many, {case.name}: largest gradient difference {worst:.2e} of the gradient's scale")
    helpers.note(f"ensemble vjp {case.name}: loss cotangent vs loss_and_grad_many, largest gradient difference {worst:.2e} of its scale")
    icnf.close()


def test_exact_zeros():
    case = BY_NAME["readme-vjp-B33"]
    icnf = _icnf(case)
    ps, xs, eps = _inputs(case.name)
    rng = np.random.default_rng(5)
    cot = (rng.standard_normal((M, 4, case.B)) / case.B).astype(np.float32)
    # a zero cotangent for one member: exactly zero gradient and grad_x, its outputs what they are
    z = cot.copy()
    z[1] = 0
    lp0, rg0, g0, gx0, _ = _vjp(icnf, case, ps, xs, eps, cot)
    lp, rg, g, gx, _ = _vjp(icnf, case, ps, xs, eps, z)
    assert not g[1].any() and not gx[1].any() and g[0].any() and gx[2].any()
    assert np.array_equal(lp, lp0) and np.array_equal(rg, rg0)
    # a one-hot sample: exactly zero grad_x columns for the other samples (a column in another tile than the first)
    j = 20
    hot = np.zeros_like(cot)
    hot[:, :, j] = [0.3, -0.2, 0.1, 0.05]
    _, _, g, gx, _ = _vjp(icnf, case, ps, xs, eps, hot)
    assert np.abs(gx[:, :, j]).min() > 0 and g.any(axis=1).all()
    assert not np.delete(gx, j, axis=2).any()
    icnf.close()


def test_rows_the_handle_does_not_integrate_ignore_their_cotangent():
    rng = np.random.default_rng(6)
    # TestMode: rows 1-3; lambda3 = 0 (no augmentation): row 3; lambda1 = lambda2 = 0: rows 1 and 2
    no12 = R.Case("readme-no-E-n", O.Cfg(O.Net((2, 6, 2), R.TANH2), 1, 1, 0.0, 0.0, 1e-2), 17, seed=31)
    BY_NAME[no12.name] = no12
    for case, dead in ((BY_NAME["regr-test-B17"], (1, 2, 3)), (BY_NAME["noaug-vjp-B1"], (3,)), (no12, (1, 2))):
        icnf = _icnf(case)
        ps, xs, eps = _inputs(case.name)
        cot = (rng.standard_normal((M, 4, case.B)) / case.B).astype(np.float32)
        other = cot.copy()
        other[:, list(dead)] = rng.standard_normal((M, len(dead), case.B)).astype(np.float32)
        a, b = _vjp(icnf, case, ps, xs, eps, cot), _vjp(icnf, case, ps, xs, eps, other)
        for u, v in zip(a[:4], b[:4]):
            assert np.array_equal(u, v), (case.name, dead)
        assert a[2].any()
        icnf.close()


@pytest.mark.parametrize("name", ["readme-vjp-B33", "regr-jvp-B33"])
def test_zero_norms_stay_finite_and_within_the_bar(name):
    """eps = 0 in some columns and a zero last layer: |eps'J|, |zdot| and |z_aug| are exactly 0 there; the unit vector of 0 is 0."""
    case = BY_NAME[name]
    icnf = _icnf(case)
    ps, xs, eps = _inputs(name, "zero-norms")
    cot = np.stack([R.cotangents(case, m)["all"] for m in range(M)])
    lp, rg, g, gx, info = _vjp(icnf, case, ps, xs, eps, cot, t1=None)
    assert np.isfinite(lp).all() and np.isfinite(rg).all() and np.isfinite(g).all() and np.isfinite(gx).all()
    nt1 = R.Case(**{**case.__dict__, "t1": None})
    for m in range(M):
        what = f"zero norms {name} member {m}"
        out, r64, r32 = R.reference(nt1, m, ps, xs, eps, cot[m], list(info["steps"][m]))
        assert_parity(lp[m], out[0], f"{what} logpx")
        assert_parity(rg[m], out[1:], f"{what} regs")
        whole = V.scale(r64[0])
        for bname, err, floor, rtol, s, ok in V.report(g[m], gx[m], r64, r32, case.cfg.net):
            if s > 0:
                assert ok, (what, bname, err, rtol)
            else:       # a block (or grad_x) the reference has exactly zero: nothing of its own to scale by -- the whole gradient's bar
                sl = V.param_blocks(case.cfg.net).get(bname)
                got = gx[m] if sl is None else g[m][sl]
                assert np.abs(got).max() <= V.RTOL * whole, (what, bname, np.abs(got).max(), whole)
    icnf.close()


def test_offsets_are_exact(monkeypatch):
    """Permuting the members permutes everything bit for bit; one member's cotangent, data or parameters moves no bit of
    another's result; calls repeat; a split above the capacity is the parts called separately."""
    case = BY_NAME["regr-vjp-B17-rejects"]
    icnf = _icnf(case)
    ps, xs, eps = _inputs(case.name)
    cot = np.stack([R.cotangents(case, m)["all"] for m in range(M)])
    base = _vjp(icnf, case, ps, xs, eps, cot)
    again = _vjp(icnf, case, ps, xs, eps, cot)
    for u, v in zip(base[:4], again[:4]):
        assert np.array_equal(u, v)
    perm = [2, 0, 1]
    p = _vjp(icnf, case, ps[perm], xs[perm], eps[perm], cot[perm])
    for u, v in zip(base[:4], p[:4]):
        assert np.array_equal(u[perm], v)
    for i, k in enumerate(perm):
        assert np.array_equal(p[4]["steps"][i], base[4]["steps"][k])
    for what in ("cot", "xs", "ps"):
        c2, x2, p2 = cot.copy(), xs.copy(), ps.copy()
        if what == "cot":
            c2[1] = c2[1] * 1.5 + 0.01
        elif what == "xs":
            x2[1] = x2[1] * 1.5 + 0.25
        else:
            p2[1] = p2[1] * 0.9
        b = _vjp(icnf, case, p2, x2, eps, c2)
        for m in (0, 2):
            for u, v in zip(base[:4], b[:4]):
                assert np.array_equal(u[m], v[m]), (what, m)
            assert np.array_equal(b[4]["steps"][m], base[4]["steps"][m])
        assert not np.array_equal(b[2][1], base[2][1]), what
    # the split: a capacity of two members per launch
    monkeypatch.setattr(ens_mod, "_device_capacity", lambda *a: 2)
    s = _vjp(icnf, case, ps, xs, eps, cot)
    assert s[4]["calls"] == 2 and s[4]["launches"] == 2
    for u, v in zip(base[:4], s[:4]):
        assert np.array_equal(u, v)
    for m in range(M):
        assert np.array_equal(s[4]["steps"][m], base[4]["steps"][m])
    icnf.close()


def test_a_nonfinite_member_is_reported_alone():
    case = BY_NAME["regr-jvp-B33"]
    icnf = _icnf(case)
    ps, xs, eps = _inputs(case.name)
    cot = np.stack([R.cotangents(case, m)["all"] for m in range(M)])
    base = _vjp(icnf, case, ps, xs, eps, cot)
    bad = xs.copy()
    bad[1, 0, 3] = np.nan
    with pytest.raises(cnf.CNFError, match="member 1") as e:
        _vjp(icnf, case, ps, bad, eps, cot)
    assert e.value.status == _lib.ERR_NONFINITE
    # the C ABI: the other members of that very launch are what they are beside a finite member 1
    l, h = _lib.lib(), icnf.handle()
    B, n_in = case.B, case.cfg.n_in
    xr, er, pr, cr = _dev(bad.transpose(0, 2, 1)), _dev(eps.transpose(0, 2, 1)), _dev(ps), _dev(cot)
    g, lp, rg = torch.full_like(pr, 7.0), torch.zeros((M, B), device="cuda"), torch.zeros((M, 3, B), device="cuda")
    gz = torch.full((M, B, n_in), 7.0, device="cuda")
    status = np.empty(M, dtype=np.int32)
    opts = cnf.base_icnf._solve_opts(icnf, icnf.tspan)
    _lib.check(l.cnf_inference_vjp_many(h, _lib.MODE_TRAIN, M, pr.data_ptr(), xr.data_ptr(), er.data_ptr(), B, C.byref(opts), None,
                                        cr.data_ptr(), lp.data_ptr(), rg.data_ptr(), g.data_ptr(), gz.data_ptr(), status.ctypes.data,
                                        None, None), h)
    assert status.tolist() == [_lib.OK, _lib.ERR_NONFINITE, _lib.OK]
    g, gz, lp, rg = g.cpu().numpy(), gz.cpu().numpy(), lp.cpu().numpy(), rg.cpu().numpy()
    assert not g[1].any() and not gz[1].any() and np.isnan(lp[1]).all() and np.isnan(rg[1]).all()
    for m in (0, 2):
        assert np.array_equal(lp[m], base[0][m]) and np.array_equal(rg[m], base[1][m]) and np.array_equal(g[m], base[2][m])
        assert np.array_equal(gz[m][:, :case.cfg.nvars].T, base[3][m])
    icnf.close()


def test_members_that_give_up_are_rerun():
    """poll_limit = 1 (the knob of the existing fallback tests: a bounded wait, not a fault): with three tiles per member the
    meetings run out; the members are run again one at a time with inference_record + inference_pullback and are correct."""
    case = BY_NAME["regr-jvp-B33"]
    icnf = _icnf(case)
    ps, xs, eps = _inputs(case.name)
    cot = np.stack([R.cotangents(case, m)["all"] for m in range(M)])
    icnf.set_solve_wait(poll_limit=1)
    try:
        lp, rg, g, gx, info = _vjp(icnf, case, ps, xs, eps, cot)
    finally:
        icnf.set_solve_wait(poll_limit=0x7fffffff)
    assert info["rerun"], info
    for m in range(M):
        what = f"rerun members, member {m}"
        _, r64, r32 = _check_member(case, m, lp[m], rg[m], g[m], gx[m], cot[m], info["steps"][m], what)
        V.assert_vjp(g[m], gx[m], r64, r32, case.cfg.net, what)
    again = _vjp(icnf, case, ps, xs, eps, cot)
    assert not again[4]["rerun"]
    icnf.close()


def test_a_member_beyond_its_step_store_is_rerun():
    """More accepted steps than WV_GCAP = 1024: that member alone hands over to the recorded route -- its result is that route's,
    bit for bit --; the member with half the span stays in the launch and meets the reference."""
    case = R.Case("beyond-the-store", O.Cfg(O.Net((6, 12, 6), R.TANH2), 6, 0, 1e-2, 1e-2, 0.0), 20, seed=41,
                  sol_kw=dict(adaptive=False, dt=1 / 1100), t1=(1.0, 0.5, 0.5))
    BY_NAME[case.name] = case
    icnf = _icnf(case)
    ps, xs, eps = _inputs(case.name)
    ps, xs, eps = ps[:2], xs[:2], eps[:2]
    cot = np.stack([R.cotangents(case, m)["all"] for m in range(2)])
    t1 = np.asarray(case.t1[:2], np.float32)
    lp, rg, g, gx, info = _vjp(icnf, case, ps, xs, eps, cot, t1=t1)
    assert info["rerun"] == [0] and info["stats"][0]["naccept"] == 1100 and info["stats"][1]["naccept"] == 550, info["stats"]
    what = "beyond the step store, member 1"
    _, r64, r32 = _check_member(case, 1, lp[1], rg[1], g[1], gx[1], cot[1], info["steps"][1], what)
    V.assert_vjp(g[1], gx[1], r64, r32, case.cfg.net, what)
    twin = _icnf(case)
    lp0, rg0 = cnf.inference_record(twin, cnf.TrainMode(), _dev(xs[0]), _dev(ps[0]), {}, eps=_dev(eps[0]), tspan=(0.0, 1.0))
    g0, gx0 = cnf.inference_pullback(twin, _dev(cot[0]), with_x=True)
    assert np.array_equal(lp0.cpu().numpy(), lp[0]) and np.array_equal(g0.cpu().numpy(), g[0]) and np.array_equal(gx0.cpu().numpy(), gx[0])
    assert np.array_equal(np.asarray(twin.last_steps, np.float32), info["steps"][0])
    icnf.close(); twin.close()


def test_the_handle_afterwards_is_what_it_was_and_refusals():
    case = BY_NAME["regr-vjp-B17-rejects"]
    ps, xs, eps = _inputs(case.name)
    cot = np.stack([R.cotangents(case, m)["all"] for m in range(M)])
    mine = O.glorot_params(case.cfg.net, np.random.default_rng(85), np.float32, 0.5)
    T = cnf.TrainMode()

    def own(icnf):
        v, g = cnf.loss_and_grad(icnf, T, _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
        lp, _ = cnf.inference(icnf, T, _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
        vm, gm, _ = cnf.loss_and_grad_many(icnf, T, _dev(xs), _dev(ps), {}, eps=_dev(eps))
        return v, g.cpu().numpy(), lp.cpu().numpy(), vm, gm.cpu().numpy()

    fresh = _icnf(case)
    want = own(fresh)
    fresh.close()
    icnf = _icnf(case)
    info = _vjp(icnf, case, ps, xs, eps, cot)[4]
    assert info["launches"] == 2 and all(s["launches"] == 2 for s in info["stats"])
    for a, b in zip(want, own(icnf)):
        assert np.array_equal(a, b)
    # straight after the call, with nothing uploaded in between: the handle's own parameters are where they were
    again = _icnf(case)
    again.set_params(mine)
    _vjp(again, case, ps, xs, eps, cot)
    lp, _ = cnf.inference(again, T, _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
    assert np.array_equal(lp.cpu().numpy(), want[2])
    # a record ends, as with every gradient call
    cnf.inference_record(again, T, _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
    _vjp(again, case, ps, xs, eps, cot)
    with pytest.raises(cnf.CNFError) as e:
        cnf.inference_pullback(again, _dev(cot[0]))
    assert e.value.status == _lib.ERR_BAD_ARG
    # more members than a launch takes: the C ABI refuses with nothing enqueued
    l, h = _lib.lib(), again.handle()
    cap = cnf.ensemble_vjp_capacity(again, T, case.B)
    assert cap > 0
    one = [_dev(a[:1]) for a in (ps, xs.transpose(0, 2, 1), eps.transpose(0, 2, 1), cot)]
    g = torch.zeros(ps.shape[1], device="cuda")
    lpb, rgb = torch.zeros(case.B, device="cuda"), torch.zeros(3 * case.B, device="cuda")
    status = np.zeros(cap + 1, dtype=np.int32)
    opts = cnf.base_icnf._solve_opts(again, again.tspan)
    s = l.cnf_inference_vjp_many(h, _lib.MODE_TRAIN, cap + 1, one[0].data_ptr(), one[1].data_ptr(), one[2].data_ptr(), case.B,
                                 C.byref(opts), None, one[3].data_ptr(), lpb.data_ptr(), rgb.data_ptr(), g.data_ptr(), None,
                                 status.ctypes.data, None, None)
    assert s == _lib.ERR_UNSUPPORTED and not g.any()
    icnf.close(); again.close()
    # what has no ensemble form is refused before anything is drawn, and has capacity 0: loss_and_grad_many's refusals
    lay = lambda dims: [cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])]
    models = [
        cnf.construct(cnf.CondRNODE, cnf.Chain(*lay((4, 6, 2))), 1, 1, rng=5),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((2, 6, 2))), 1, 1, rng=5, basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2)),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((2, 6, 2))), 1, 1, rng=5, compute_mode=cnf.HIPVecJacMatrixMode("generic")),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((32, 128, 128, 32))), 32, 0, rng=5),
    ]
    for ic in models:
        before = ic.rng.bit_generator.state
        x = torch.zeros((2, ic.nvars, 16), device="cuda")
        p = torch.zeros((2, ic.nn.n_params_internal), device="cuda")
        with pytest.raises(NotImplementedError):
            cnf.inference_vjp_many(ic, T, x, p, {}, (torch.zeros((2, 16), device="cuda"), None))
        with pytest.raises(NotImplementedError):
            cnf.loss_and_grad_many(ic, T, x, p, {})
        assert cnf.ensemble_vjp_capacity(ic, T, 16) == 0 == cnf.ensemble_capacity(ic, T, 16)
        assert ic.rng.bit_generator.state == before
        ic.close()


def _backward_check(case, icnf, ps, xs, eps, cot, g_ps, g_xs, fwd_logpx, what, shared):
    """The autograd gradients against the reference for the cotangent ``cot`` (M, 4, B) the objective has, on the steps of the
    backward launch; that launch's logpx against the forward's."""
    back = icnf.last_backward_logpx.cpu().numpy()
    same = np.array_equal(back, fwd_logpx)
    assert_parity(back, fwd_logpx, f"{what}: backward launch's logpx vs the forward's")
    helpers.note(f"{what}: the backward launch's logpx is {'bit-identical to' if same else 'NOT bit-identical to'} the forward's "
                 f"(largest difference {np.abs(back - fwd_logpx).max():.2e})")
    print(f"{what}: backward logpx bit-identical to the forward's: {same}")
    gx_sum = 0
    for m in range(M):
        dts = cnf.ensemble_steps(icnf, m)
        _, r64, r32 = _ref(case, m, cot[m], dts)
        if shared:
            V.assert_vjp(g_ps[m], None, r64, r32, case.cfg.net, f"{what} member {m}")
            gx_sum = gx_sum + np.stack([r64[1], r32[1]])
        else:
            V.assert_vjp(g_ps[m], g_xs[m], r64, r32, case.cfg.net, f"{what} member {m}")
    if shared:
        s = V.scale(gx_sum[0])
        floor = np.abs(gx_sum[1].astype(np.float64) - gx_sum[0]).max() / s
        rtol = max(V.RTOL, V.FLOOR_FACTOR * floor)
        assert rtol <= V.RTOL_CAP and np.abs(g_xs - gx_sum[0]).max() <= rtol * s, (what, floor)


def test_differentiable_inference_many_weighted_loss():
    """torch.autograd.grad of a weighted (Bayesian-bootstrap) loss: every member sees its own per-sample weights."""
    case = BY_NAME["readme-vjp-B33"]
    icnf = _icnf(case)
    ps, xs, eps = _inputs(case.name)
    t1 = np.asarray(case.t1, np.float32)
    cfg, B = case.cfg, case.B
    w = np.random.default_rng(8).exponential(size=(M, B)).astype(np.float32)
    w /= w.sum(axis=1, keepdims=True)
    pt, xt, wt = _dev(ps).requires_grad_(), _dev(xs).requires_grad_(), _dev(w)
    logpx, (E, n, A) = cnf.differentiable_inference_many(icnf, cnf.TrainMode(), xt, pt, {}, eps=_dev(eps), t1=t1)
    loss = (wt * (-logpx + cfg.lam1 * E + cfg.lam2 * n + cfg.lam3 * A)).sum()
    g_ps, g_xs = torch.autograd.grad(loss, (pt, xt))
    cot = np.stack([-w, cfg.lam1 * w, cfg.lam2 * w, cfg.lam3 * w], axis=1).astype(np.float32)
    _backward_check(case, icnf, ps, xs, eps, cot, g_ps.cpu().numpy(), g_xs.cpu().numpy(), logpx.detach().cpu().numpy(),
                    "weighted loss", False)
    icnf.close()


def test_stacking_objective_and_log_prob():
    """-mean_b logsumexp_m(log w_m + logpdf_m(x_b)) with w = softmax(logits): gradients w.r.t. the members' parameters, the
    shared data and the mixture's logits; ``EnsembleDist.log_prob`` is ``logpdf`` in value."""
    case = BY_NAME["regr-test-B17"]
    icnf = _icnf(case)
    ps, xs, _ = _inputs(case.name)
    B = case.B
    logits = np.asarray([0.3, -0.2, 0.5])
    pt, xt = _dev(ps).requires_grad_(), _dev(xs[0]).requires_grad_()
    lt = torch.tensor(logits, dtype=torch.float32, device="cuda", requires_grad=True)
    d = cnf.EnsembleDist(icnf, cnf.TestMode(), pt, {}, weights=torch.softmax(lt, 0))
    lp = d.log_prob(xt)
    obj = -lp.mean()
    g_ps, g_xs, g_l = torch.autograd.grad(obj, (pt, xt, lt))
    fwd = cnf.inference_many(icnf, cnf.TestMode(), xt.detach(), pt.detach(), {})[0].cpu().numpy()
    # log_prob equals logpdf in value (two spellings of one logsumexp: the parity bar)
    assert_parity(lp.detach().cpu().numpy(), d.logpdf(xt.detach()).cpu().numpy(), "EnsembleDist.log_prob vs logpdf")
    # the reference: the float64 logpdf of every member on the steps of the backward launch, the objective in float64 autograd
    steps = [cnf.ensemble_steps(icnf, m) for m in range(M)]
    zero = np.zeros((4, B), np.float32)
    ref_lp = np.stack([_ref(case, m, zero, steps[m])[0][0] for m in range(M)])
    rl = torch.tensor(ref_lp, dtype=torch.float64, requires_grad=True)
    rlog = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    robj = -torch.logsumexp(rl + torch.log_softmax(rlog, 0)[:, None], dim=0).mean()
    c_lp, c_log = torch.autograd.grad(robj, (rl, rlog))
    assert abs(float(obj.detach()) - float(robj.detach())) <= 1e-5 * max(1.0, abs(float(robj)))
    cot = np.zeros((M, 4, B), np.float32)
    cot[:, 0] = c_lp.numpy()
    _backward_check(case, icnf, ps, xs, None, cot, g_ps.cpu().numpy(), g_xs.cpu().numpy(), fwd, "stacking objective", True)
    # d obj / d logits_k = w_k - mean_b r_kb with r = softmax_m(log w_m + logpdf_m): every entry of the softmax's Jacobian is at
    # most 1/4, so an error of the members' logpdf within the parity bar moves it by at most M / 4 times that bar
    bar = 0.25 * M * float((helpers.RTOL * np.abs(ref_lp) + helpers.ATOL * max(1.0, np.sqrt(np.mean(ref_lp ** 2)))).max())
    c_log = c_log.numpy()
    assert np.abs(g_l.cpu().numpy() - c_log).max() <= bar, (g_l, c_log, bar)
    icnf.close()
