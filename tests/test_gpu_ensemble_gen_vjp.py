"""Differentiable ensemble sampling on the device: ``generate_vjp_many`` (cnf_generate_vjp_many, the sampling form of the
ensemble gradient kernel), ``differentiable_generate_many`` and ``reverse_kl_many``.

Reference: tests/ensemble_gen_vjp_ref.py -- ``gen_vjp_ref.vjp64`` replaying for every member the steps that member itself
accepted on the device (cnf_ensemble_steps), held with ``vjp_ref.assert_vjp`` unchanged, grad_z0 in the place of grad_x
(``rtol = max(1e-4, 8 floor)`` per parameter block and for grad_z0, capped at 1e-3, the floor from ``vjp32``:
tests/test_ensemble_gen_vjp_host.py shows it is under a quarter of the bar on every case); ``xs`` and ``logq`` at
tests/helpers.py's parity bar.  Everything else is exact: zeros, permutations, isolation, repetition and splits are compared bit
for bit.  The differences that are measured and not asserted against a number chosen in advance -- the one-launch result against
the one-model pair's, the gradient launch's ``xs`` / ``logq`` against ``generate_many``'s -- are printed and go to
parity_report.json's notes.

Measured on the MI355X.  Against ``generate_record`` + ``generate_pullback`` of each member: the two solves do not accept the
same step sequences (two kernels, two tanh); over the seven cases the results differ by at most 9.4e-07 (xs), 2.4e-06 (logq),
1.1e-05 (grads) and 1.1e-05 (grad_z0) of the respective scale, the largest on the case with reltol = 1e-4 whose stiff member
rejects attempts.  The gradient launch's ``xs`` / ``logq`` against ``generate_many``'s on the same draws: NOT bit-identical -- the
forward is the plain ensemble form, whose evaluations use the exp2 / rcp tanh, the gradient launch's forward half the 2-ulp
tanh its adjoint differentiates --; largest difference 1.0e-06 in xs and 1.9e-06 in logq (|logq| up to 31), a few percent of
the parity bar.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from continuousnf.jl_amd import ensemble as ens_mod
from oracle import cnf_oracle as O
from tests import ensemble_gen_vjp_ref as R
from tests import gen_vjp_ref as GR
from tests import helpers
from tests import vjp_ref as V
from tests.helpers import assert_parity, make_icnf
from tests.test_gpu_inference_vjp import _block_bar

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
M = R.M
BY_NAME = {c.name: c for c in R.CASES}
LAUNCHES = 4                       # the solve with its adjoint, the partial sums, the column kernels: (x, logq) and the z0 tail


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _mode(train):
    return cnf.TrainMode() if train else cnf.TestMode()


def _icnf(case, **kw):
    return make_icnf(cnf, case.cfg, jvp=case.jvp, kernel="mfma", sol_kwargs=dict(case.sol_kw), **kw)


def _t0(case):
    return np.asarray(case.t1, np.float32) if case.t1 is not None else None


def _vjp(icnf, case, ps, z0, eps, cot, t0="case", **kw):
    """-> (xs (M, nvars, B), logq (M, B), grads, grad_z0 (M, n_in, B), info), numpy.  ``cot = (g_x, g_logq)``, numpy or None."""
    t0 = _t0(case) if isinstance(t0, str) else t0
    xs, lq, g, gz, info = cnf.generate_vjp_many(icnf, _mode(case.train), _dev(ps), {}, case.B, (_dev(cot[0]), _dev(cot[1])),
                                                z0=_dev(z0), eps=_dev(eps), t0=t0, with_z0=True, with_steps=True, **kw)
    return _np(xs), _np(lq), _np(g), _np(gz), info


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return R.inputs(BY_NAME[name])


_COTS = {}


@functools.lru_cache(maxsize=None)
def _reference(name, m, cot_key, dts):
    """One member's float64 / float32 reference, computed once per (case, member, cotangent, steps)."""
    ps, z0, eps = _inputs(name)
    return R.reference(BY_NAME[name], m, ps, z0, eps, _COTS[cot_key], list(dts))


def _ref(case, m, cot, dts):
    """``cot = (cot_z, cot_logq)`` of ONE member."""
    key = (case.name, m) + tuple(None if c is None else c.tobytes() for c in cot)
    _COTS[key] = cot
    return _reference(case.name, m, key, tuple(abs(float(d)) for d in dts))


def _member_cot(cot, m):
    return tuple(None if c is None else c[m] for c in cot)


def _check_member(case, m, xs, lq, g, gz, cot, dts, what):
    """One member's outputs against its reference on the steps ``dts``: parity of (xs, logq), assert_vjp of (grads, grad_z0)."""
    (z64, q64), r64, r32 = _ref(case, m, cot, dts)
    assert_parity(xs, z64[:case.cfg.nvars], f"{what} xs")
    assert_parity(lq, q64, f"{what} logq")
    V.assert_vjp(g, gz, r64, r32, case.cfg.net, what)
    return r64


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_each_member_and_cotangent_matches_the_float64_adjoint_on_its_own_steps(case):
    icnf = _icnf(case)
    assert cnf.ensemble_generate_vjp_capacity(icnf, _mode(case.train), case.B) >= M
    ps, z0, eps = _inputs(case.name)
    cots = [R.cotangents(case, m) for m in range(M)]
    assert sorted(cots[0]) == ["both", "logq", "x", "z-all-rows"]
    for name in cots[0]:
        cot = R.stack_cot(case, cots, name)
        xs, lq, g, gz, info = _vjp(icnf, case, ps, z0, eps, cot)
        assert info["launches"] == LAUNCHES and info["calls"] == 1 and not info["rerun"], info
        assert (info["status"] == _lib.OK).all()
        assert xs.shape == (M, case.cfg.nvars, case.B) and lq.shape == (M, case.B) and gz.shape == (M, case.cfg.n_in, case.B)
        for m in range(M):
            what = f"ensemble generate vjp {case.name} member {m} cot {name}"
            steps = info["steps"][m]
            assert len(steps) == info["stats"][m]["naccept"] > 0, what
            # sampling runs over reverse(tspan): every step has the sign of tspan[0] - tspan[1]
            assert (np.sign(steps) == np.sign(case.cfg.tspan[0] - case.cfg.tspan[1])).all(), (what, steps)
            _check_member(case, m, xs[m], lq[m], g[m], gz[m], _member_cot(cot, m), steps, what)
    if "rejects" in case.name:
        assert info["stats"][0]["nreject"] >= 1, info["stats"]
    if case.t1 is not None:
        assert info["t0"].tolist() == [float(np.float32(t)) for t in case.t1]
    assert all(s["t_final"] == float(np.float32(case.cfg.tspan[0])) for s in info["stats"]), info["stats"]
    helpers.note(f"ensemble generate vjp {case.name}: steps {[s['naccept'] for s in info['stats']]}, rejected "
                 f"{[s['nreject'] for s in info['stats']]}, {info['launches']} launches")
    icnf.close()


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_against_generate_record_and_generate_pullback_of_each_member(case):
    """The one-model pair on the same z0, eps, span and cotangent: each side is held to the float64 reference on ITS OWN accepted
    steps at the bar; their mutual difference is printed and noted, not asserted."""
    icnf = _icnf(case)
    ps, z0, eps = _inputs(case.name)
    cot = R.stack_cot(case, [R.cotangents(case, m) for m in range(M)], "z-all-rows")
    xs, lq, g, gz, info = _vjp(icnf, case, ps, z0, eps, cot)
    icnf.close()
    mode, t0 = _mode(case.train), _t0(case)
    worst = dict(xs=0.0, logq=0.0, grads=0.0, grad_z0=0.0)
    same_steps = []
    for m in range(M):
        what = f"{case.name} member {m}"
        cm = _member_cot(cot, m)
        _check_member(case, m, xs[m], lq[m], g[m], gz[m], cm, info["steps"][m], f"one launch, {what}")
        one = _icnf(case)
        span = (case.cfg.tspan[0], float(t0[m]) if t0 is not None else case.cfg.tspan[1])
        x1, q1 = cnf.generate_record(one, mode, _dev(ps[m]), {}, case.B, z0=_dev(z0[m]), eps=_dev(eps[m]), tspan=span)
        steps1 = np.asarray(one.last_steps, np.float32)
        g1, gz1 = cnf.generate_pullback(one, (_dev(cm[0]), _dev(cm[1])), with_z0=True)
        x1, q1, g1, gz1 = _np(x1), _np(q1), _np(g1), _np(gz1)
        one.close()
        _check_member(case, m, x1, q1, g1, gz1, cm, steps1, f"record + pullback, {what}")
        same_steps.append(bool(np.array_equal(steps1, info["steps"][m])))
        for k, a, b in (("xs", xs[m], x1), ("logq", lq[m], q1), ("grads", g[m], g1), ("grad_z0", gz[m], gz1)):
            worst[k] = max(worst[k], float(np.abs(a.astype(np.float64) - b).max() / max(V.scale(b), 1e-300)))
    txt = (f"generate_vjp_many vs generate_record + generate_pullback, {case.name}: largest difference over its scale "
           + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; same accepted steps per member: {same_steps}")
    print(txt)
    helpers.note(txt)


def test_offsets_are_exact(monkeypatch):
    """Calls repeat; permuting the members permutes every output and the step lists bit for bit; one member's cotangent, z0 or
    parameters moves no bit of another's result; a split above the capacity is the unsplit call."""
    case = BY_NAME["gen-regr-vjp-B17-rejects"]
    icnf = _icnf(case)
    ps, z0, eps = _inputs(case.name)
    cot = R.stack_cot(case, [R.cotangents(case, m) for m in range(M)], "z-all-rows")
    base = _vjp(icnf, case, ps, z0, eps, cot)
    again = _vjp(icnf, case, ps, z0, eps, cot)
    for u, v in zip(base[:4], again[:4]):
        assert np.array_equal(u, v)
    perm = [2, 0, 1]
    p = _vjp(icnf, case, ps[perm], z0[perm], eps[perm], (cot[0][perm], cot[1][perm]))
    for u, v in zip(base[:4], p[:4]):
        assert np.array_equal(u[perm], v)
    for i, k in enumerate(perm):
        assert np.array_equal(p[4]["steps"][i], base[4]["steps"][k])
    for what in ("cot", "z0", "ps"):
        c2, z2, p2 = (cot[0].copy(), cot[1].copy()), z0.copy(), ps.copy()
        if what == "cot":
            c2[0][1] = c2[0][1] * 1.5 + 0.01
            c2[1][1] = c2[1][1] * 0.5 - 0.01
        elif what == "z0":
            z2[1] = z2[1] * 1.5 + 0.25
        else:
            p2[1] = p2[1] * 0.9
        b = _vjp(icnf, case, p2, z2, eps, c2)
        for m in (0, 2):
            for u, v in zip(base[:4], b[:4]):
                assert np.array_equal(u[m], v[m]), (what, m)
            assert np.array_equal(b[4]["steps"][m], base[4]["steps"][m])
        assert not np.array_equal(b[2][1], base[2][1]), what
    # the split: a capacity of two members per launch
    monkeypatch.setattr(ens_mod, "_device_capacity", lambda *a: 2)
    s = _vjp(icnf, case, ps, z0, eps, cot)
    assert s[4]["calls"] == 2 and s[4]["launches"] == LAUNCHES
    for u, v in zip(base[:4], s[:4]):
        assert np.array_equal(u, v)
    for m in range(M):
        assert np.array_equal(s[4]["steps"][m], base[4]["steps"][m])
    icnf.close()


def test_exact_zeros():
    case = BY_NAME["gen-readme-vjp-B33"]
    icnf = _icnf(case)
    ps, z0, eps = _inputs(case.name)
    rng = np.random.default_rng(5)
    n_in, B = case.cfg.n_in, case.B
    cot = ((rng.standard_normal((M, n_in, B)) / B).astype(np.float32), (rng.standard_normal((M, B)) / B).astype(np.float32))
    # a zero cotangent for one member: exactly zero gradient and grad_z0, every member's outputs what they are
    z = (cot[0].copy(), cot[1].copy())
    z[0][1] = 0
    z[1][1] = 0
    xs0, lq0, g0, gz0, _ = _vjp(icnf, case, ps, z0, eps, cot)
    xs, lq, g, gz, _ = _vjp(icnf, case, ps, z0, eps, z)
    assert not g[1].any() and not gz[1].any() and g[0].any() and gz[2].any()
    assert np.array_equal(xs, xs0) and np.array_equal(lq, lq0)
    assert np.array_equal(g[0], g0[0]) and np.array_equal(gz[2], gz0[2])
    # a one-hot sample (a column in another tile than the first): exactly zero grad_z0 columns for the other samples -- with a
    # cotangent on the state rows alone, on logq alone (grad_z0 has the -g_logq z0 tail) and on both
    j = 20
    for rows in ("z", "logq", "both"):
        hot = (np.zeros_like(cot[0]) if rows != "logq" else None, np.zeros_like(cot[1]) if rows != "z" else None)
        if hot[0] is not None:
            hot[0][:, :, j] = [0.3, -0.2]
        if hot[1] is not None:
            hot[1][:, j] = 0.7
        _, _, g, gz, _ = _vjp(icnf, case, ps, z0, eps, hot)
        assert np.abs(gz[:, :, j]).min() > 0 and g.any(axis=1).all(), rows
        assert not np.delete(gz, j, axis=2).any(), rows
    icnf.close()


@pytest.mark.parametrize("name", ["gen-readme-vjp-B33", "gen-regr-test-B17"])
def test_forward_outputs_against_generate_many(name):
    """``xs`` / ``logq`` of the gradient launch and of ``generate_many(with_logp=True)`` on the same draws: both pass the parity
    bar against float64 on their own steps; their difference is printed and noted (the two forms evaluate tanh differently, as
    in the density direction: DESIGN 4.4)."""
    case = BY_NAME[name]
    icnf = _icnf(case)
    ps, z0, eps = _inputs(name)
    cot = R.stack_cot(case, [R.cotangents(case, m) for m in range(M)], "both")
    xs, lq, _, _, info = _vjp(icnf, case, ps, z0, eps, cot)
    fx, fq = cnf.generate_many(icnf, _mode(case.train), _dev(ps), {}, case.B, z0=_dev(z0), eps=_dev(eps), t0=_t0(case), with_logp=True,
                               with_steps=True)
    fx, fq = _np(fx), _np(fq)
    finfo = icnf.last_ensemble_info
    for m in range(M):
        (z64, q64), _, _ = _ref(case, m, _member_cot(cot, m), info["steps"][m])
        assert_parity(xs[m], z64[:case.cfg.nvars], f"gradient launch {name} member {m} xs")
        assert_parity(lq[m], q64, f"gradient launch {name} member {m} logq")
        rows = finfo["steps"][m]
        acc = rows[rows[:, 3] == 1.0, 1]
        cfg = R.member_cfg(case, m)
        f64 = lambda a: np.asarray(a, np.float64)
        z, q, _, _ = GR.forward(cfg, f64(ps[m]), f64(z0[m]), f64(eps[m]) if case.train else None, [abs(float(d)) for d in acc],
                                train=case.train)
        assert_parity(fx[m], z[:case.cfg.nvars], f"generate_many {name} member {m} xs")
        assert_parity(fq[m], q, f"generate_many {name} member {m} logq")
    same = np.array_equal(xs, fx) and np.array_equal(lq, fq)
    txt = (f"generate_vjp_many vs generate_many, {name}: xs / logq are {'bit-identical' if same else 'NOT bit-identical'}; largest "
           f"difference xs {np.abs(xs - fx).max():.2e}, logq {np.abs(lq - fq).max():.2e} (|logq| up to {np.abs(fq).max():.1f})")
    print(txt)
    helpers.note(txt)
    icnf.close()


def _target(nvars, seed=31):
    """A diagonal Gaussian target per member: mean and sigma, (M, nvars) each."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((M, nvars)), rng.uniform(0.5, 2.0, (M, nvars))


@pytest.mark.parametrize("name", ["gen-readme-vjp-B33", "gen-regr-test-B17"])
def test_autograd_of_reverse_kl_many(name):
    """``reverse_kl_many`` to Gaussian targets, backward into ``ps`` and a ``z0`` that requires grad: the gradients are
    ``generate_vjp_many`` called with the cotangents autograd produced (g_logq = 1 / n, g_x = (xs - mu) / sigma^2 / n), bit for
    bit, and each member's is, at the bar, ``reverse_kl`` of that member through ``differentiable_generate``."""
    case = BY_NAME[name]
    icnf = _icnf(case)
    ps, z0, eps = _inputs(name)
    B, nvars = case.B, case.cfg.nvars
    mode, t0 = _mode(case.train), _t0(case)
    mu, sig = _target(nvars)
    mu_d, sig_d = _dev(mu)[:, :, None], _dev(sig)[:, :, None]
    target = lambda x: -0.5 * (((x - mu_d) / sig_d) ** 2).sum(1)
    pt, zt = _dev(ps).requires_grad_(), _dev(z0).requires_grad_()
    losses = cnf.reverse_kl_many(icnf, mode, pt, {}, B, target, z0=zt, eps=_dev(eps), t0=t0)
    assert tuple(losses.shape) == (M,)
    g_ps, g_z0 = torch.autograd.grad(losses.sum(), (pt, zt))
    back_x, back_q = _np(icnf.last_backward_xs), _np(icnf.last_backward_logq)
    # forward = generate_many on the same draws
    fx, fq = cnf.generate_many(icnf, mode, _dev(ps), {}, B, z0=_dev(z0), eps=_dev(eps), t0=t0, with_logp=True)
    want = (fq - target(fx)).mean(dim=1)
    assert np.array_equal(_np(losses), _np(want))
    assert_parity(back_x, _np(fx), f"{name}: backward launch's xs vs the forward's")
    assert_parity(back_q, _np(fq), f"{name}: backward launch's logq vs the forward's")
    helpers.note(f"differentiable_generate_many {name}: the backward launch's outputs differ from the forward's by at most "
                 f"xs {np.abs(back_x - _np(fx)).max():.2e}, logq {np.abs(back_q - _np(fq)).max():.2e}")
    # ... the direct call with the cotangents autograd produced: the same objective differentiated w.r.t. the forward's outputs
    xl, ql = fx.clone().requires_grad_(), fq.clone().requires_grad_()
    cot = tuple(_np(c) for c in torch.autograd.grad((ql - target(xl)).mean(dim=1).sum(), (xl, ql)))
    assert np.array_equal(cot[1], np.full((M, B), np.float32(1.0 / B)))
    assert_parity(cot[0], _np((fx - mu_d) / sig_d ** 2 / B), f"{name}: g_x is (xs - mu) / sigma^2 / n")
    _, _, g, gz, info = _vjp(icnf, case, ps, z0, eps, cot)
    assert np.array_equal(_np(g_ps), g) and np.array_equal(_np(g_z0), gz)
    for m in range(M):
        _check_member(case, m, back_x[m], back_q[m], g[m], gz[m], _member_cot(cot, m), info["steps"][m], f"autograd {name} member {m}")
    # a loss without one of the two outputs: the other's cotangent is None
    xs2, logq2 = cnf.differentiable_generate_many(icnf, mode, pt, {}, B, z0=zt, eps=_dev(eps), t0=t0)
    (g_only_q,) = torch.autograd.grad(logq2.sum(), (pt,))
    _, _, gq, _, _ = _vjp(icnf, case, ps, z0, eps, (None, np.ones((M, B), np.float32)))
    assert np.array_equal(_np(g_only_q), gq)
    icnf.close()
    # ... and the per-member reverse_kl through differentiable_generate
    for m in range(M):
        one = _icnf(case)
        one.tspan = (case.cfg.tspan[0], float(t0[m]) if t0 is not None else case.cfg.tspan[1])
        p1, z1 = _dev(ps[m]).requires_grad_(), _dev(z0[m]).requires_grad_()
        tm = lambda x, m=m: -0.5 * (((x - mu_d[m]) / sig_d[m]) ** 2).sum(0)
        out = cnf.reverse_kl(one, mode, p1, {}, B, tm, z0=z1, eps=_dev(eps[m]) if case.train else None)
        a, b = torch.autograd.grad(out, (p1, z1))
        one.close()
        assert abs(float(out.detach()) - float(losses[m].detach())) <= 1e-5 * max(1.0, abs(float(out.detach())))
        _block_bar(g[m], _np(a), case.cfg.net, f"reverse_kl_many vs reverse_kl, {name} member {m}", V.RTOL, gz[m], _np(b))


def test_a_nonfinite_member_is_reported_alone():
    case = BY_NAME["gen-regr-jvp-B33"]
    icnf = _icnf(case)
    ps, z0, eps = _inputs(case.name)
    cot = R.stack_cot(case, [R.cotangents(case, m) for m in range(M)], "z-all-rows")
    base = _vjp(icnf, case, ps, z0, eps, cot)
    bad = z0.copy()
    bad[1, 0, 3] = np.nan
    with pytest.raises(cnf.CNFError, match="member 1") as e:
        _vjp(icnf, case, ps, bad, eps, cot)
    assert e.value.status == _lib.ERR_NONFINITE
    # the C ABI: the other members of that very launch are what they are beside a finite member 1
    l, h = _lib.lib(), icnf.handle()
    B, n_in, nv = case.B, case.cfg.n_in, case.cfg.nvars
    zr, er, pr = _dev(bad.transpose(0, 2, 1)), _dev(eps.transpose(0, 2, 1)), _dev(ps)
    cz, cl = _dev(cot[0].transpose(0, 2, 1)), _dev(cot[1])
    g, xo, lq = torch.full_like(pr, 7.0), torch.zeros((M, B, nv), device="cuda"), torch.zeros((M, B), device="cuda")
    gz = torch.full((M, B, n_in), 7.0, device="cuda")
    status = np.empty(M, dtype=np.int32)
    opts = cnf.base_icnf._solve_opts(icnf, (icnf.tspan[1], icnf.tspan[0]))
    _lib.check(l.cnf_generate_vjp_many(h, _lib.MODE_TRAIN, M, pr.data_ptr(), zr.data_ptr(), er.data_ptr(), B, C.byref(opts), None,
                                       cz.data_ptr(), cl.data_ptr(), xo.data_ptr(), lq.data_ptr(), g.data_ptr(), gz.data_ptr(),
                                       status.ctypes.data, None, None), h)
    assert status.tolist() == [_lib.OK, _lib.ERR_NONFINITE, _lib.OK]
    g, gz, xo, lq = _np(g), _np(gz), _np(xo), _np(lq)
    assert not g[1].any() and not gz[1].any() and np.isnan(xo[1]).all() and np.isnan(lq[1]).all()
    for m in (0, 2):
        assert np.array_equal(xo[m].T, base[0][m]) and np.array_equal(lq[m], base[1][m]) and np.array_equal(g[m], base[2][m])
        assert np.array_equal(gz[m].T, base[3][m])
    icnf.close()


def test_members_that_give_up_are_rerun():
    """poll_limit = 1 (the knob of the existing fallback tests: a bounded wait, not a fault): with three tiles per member the
    meetings run out; the members are run again one at a time with generate_record + generate_pullback and are correct; a second
    call needs no rerun."""
    case = BY_NAME["gen-regr-jvp-B33"]
    icnf = _icnf(case)
    ps, z0, eps = _inputs(case.name)
    cot = R.stack_cot(case, [R.cotangents(case, m) for m in range(M)], "z-all-rows")
    icnf.set_solve_wait(poll_limit=1)
    try:
        xs, lq, g, gz, info = _vjp(icnf, case, ps, z0, eps, cot)
    finally:
        icnf.set_solve_wait(poll_limit=0x7fffffff)
    assert info["rerun"], info
    for m in range(M):
        _check_member(case, m, xs[m], lq[m], g[m], gz[m], _member_cot(cot, m), info["steps"][m], f"rerun members, member {m}")
    again = _vjp(icnf, case, ps, z0, eps, cot)
    assert not again[4]["rerun"]
    icnf.close()


def test_a_member_beyond_its_step_store_is_rerun():
    """More accepted steps than WV_GCAP = 1024: that member alone hands over to the recorded route -- its result is that route's,
    bit for bit --; the member with half the span stays in the launch and meets the reference."""
    case = R.Case("gen-beyond-the-store", O.Cfg(O.Net((6, 12, 6), R.TANH2), 6, 0, 1e-2, 1e-2, 0.0), 20, seed=41,
                  sol_kw=dict(adaptive=False, dt=1 / 1100), t1=(1.0, 0.5, 0.5))
    BY_NAME[case.name] = case
    icnf = _icnf(case)
    ps, z0, eps = _inputs(case.name)
    cots = [R.cotangents(case, m) for m in range(2)]
    cot = R.stack_cot(case, cots, "both")
    t0 = np.asarray(case.t1[:2], np.float32)
    xs, lq, g, gz, info = cnf.generate_vjp_many(icnf, cnf.TrainMode(), _dev(ps[:2]), {}, case.B, (_dev(cot[0]), _dev(cot[1])),
                                                z0=_dev(z0[:2]), eps=_dev(eps[:2]), t0=t0, with_z0=True, with_steps=True)
    xs, lq, g, gz = _np(xs), _np(lq), _np(g), _np(gz)
    assert info["rerun"] == [0] and info["stats"][0]["naccept"] == 1100 and info["stats"][1]["naccept"] == 550, info["stats"]
    _check_member(case, 1, xs[1], lq[1], g[1], gz[1], _member_cot(cot, 1), info["steps"][1], "beyond the step store, member 1")
    twin = _icnf(case)
    x0, q0 = cnf.generate_record(twin, cnf.TrainMode(), _dev(ps[0]), {}, case.B, z0=_dev(z0[0]), eps=_dev(eps[0]), tspan=(0.0, 1.0))
    g0, gz0 = cnf.generate_pullback(twin, (_dev(cot[0][0]), _dev(cot[1][0])), with_z0=True)
    assert np.array_equal(_np(x0), xs[0]) and np.array_equal(_np(q0), lq[0])
    assert np.array_equal(_np(g0), g[0]) and np.array_equal(_np(gz0), gz[0])
    assert np.array_equal(np.asarray(twin.last_steps, np.float32), info["steps"][0])
    icnf.close(); twin.close()


def test_the_handle_afterwards_is_what_it_was_and_refusals():
    case = BY_NAME["gen-regr-vjp-B17-rejects"]
    ps, z0, eps = _inputs(case.name)
    xs_data = np.random.default_rng(86).standard_normal((case.cfg.nvars, case.B)).astype(np.float32)
    cot = R.stack_cot(case, [R.cotangents(case, m) for m in range(M)], "both")
    mine = O.glorot_params(case.cfg.net, np.random.default_rng(85), np.float32, 0.5)
    T = cnf.TrainMode()

    def own(icnf):
        lp, _ = cnf.inference(icnf, T, _dev(xs_data), mine, {}, eps=_dev(eps[0]))
        gx = cnf.generate(icnf, T, mine, {}, case.B, z0=_dev(z0[0]), eps=_dev(eps[0]))
        v, g = cnf.loss_and_grad(icnf, T, _dev(xs_data), mine, {}, eps=_dev(eps[0]))
        return _np(lp), _np(gx), v, _np(g)

    fresh = _icnf(case)
    want = own(fresh)
    fresh.close()
    icnf = _icnf(case)
    before = own(icnf)
    info = _vjp(icnf, case, ps, z0, eps, cot)[4]
    assert info["launches"] == LAUNCHES and all(s["launches"] == LAUNCHES for s in info["stats"])
    for a, b, c in zip(want, before, own(icnf)):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # straight after the call, with nothing uploaded in between: the handle's own parameters are where they were
    again = _icnf(case)
    again.set_params(mine)
    _vjp(again, case, ps, z0, eps, cot)
    lp, _ = cnf.inference(again, T, _dev(xs_data), mine, {}, eps=_dev(eps[0]))
    assert np.array_equal(_np(lp), want[0])
    # a record ends, as with every gradient call
    cnf.generate_record(again, T, mine, {}, case.B, z0=_dev(z0[0]), eps=_dev(eps[0]))
    _vjp(again, case, ps, z0, eps, cot)
    with pytest.raises(cnf.CNFError) as e:
        cnf.generate_pullback(again, (None, _dev(cot[1][0])))
    assert e.value.status == _lib.ERR_BAD_ARG
    # cnf_ensemble_steps answers for this call
    assert all(len(cnf.ensemble_steps(again, m)) > 0 for m in range(M))
    # more members than a launch takes, and the generic kernel: the C ABI refuses with nothing enqueued
    l, h = _lib.lib(), again.handle()
    cap = cnf.ensemble_generate_vjp_capacity(again, T, case.B)
    assert cap > 0
    one = [_dev(a[:1]) for a in (ps, z0.transpose(0, 2, 1), eps.transpose(0, 2, 1), cot[1])]
    g = torch.zeros(ps.shape[1], device="cuda")
    xb, qb = torch.zeros(case.B * case.cfg.nvars, device="cuda"), torch.zeros(case.B, device="cuda")
    status = np.zeros(cap + 1, dtype=np.int32)
    opts = cnf.base_icnf._solve_opts(again, (again.tspan[1], again.tspan[0]))

    def raw(members, o):
        return l.cnf_generate_vjp_many(h, _lib.MODE_TRAIN, members, one[0].data_ptr(), one[1].data_ptr(), one[2].data_ptr(), case.B,
                                       C.byref(o), None, None, one[3].data_ptr(), xb.data_ptr(), qb.data_ptr(), g.data_ptr(), None,
                                       status.ctypes.data, None, None)

    assert raw(cap + 1, opts) == _lib.ERR_UNSUPPORTED and not g.any()
    generic = _lib.cnf_solve_opts.from_buffer_copy(opts)                   # (a copy: the model keeps the struct it hands out)
    generic.kernel = _lib.KERNEL_GENERIC
    assert raw(1, generic) == _lib.ERR_UNSUPPORTED and not g.any()
    assert raw(1, opts) == _lib.OK and g.any() and status[0] == _lib.OK
    icnf.close(); again.close()
    # what has no ensemble form is refused before anything is drawn, and has capacity 0: generate_many's refusals
    lay = lambda dims: [cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])]
    models = [
        cnf.construct(cnf.CondRNODE, cnf.Chain(*lay((4, 6, 2))), 1, 1, rng=5),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((2, 6, 2))), 1, 1, rng=5, basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2)),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((2, 6, 2))), 1, 1, rng=5, compute_mode=cnf.HIPVecJacMatrixMode("generic")),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((32, 128, 128, 32))), 32, 0, rng=5),
    ]
    for ic in models:
        before = ic.rng.bit_generator.state
        p = torch.zeros((2, ic.nn.n_params_internal), device="cuda")
        with pytest.raises(NotImplementedError):
            cnf.generate_vjp_many(ic, T, p, {}, 16, (None, torch.zeros((2, 16), device="cuda")))
        with pytest.raises(NotImplementedError):
            cnf.reverse_kl_many(ic, T, p, {}, 16, lambda x: x.sum(1))
        assert cnf.ensemble_generate_vjp_capacity(ic, T, 16) == 0
        assert ic.rng.bit_generator.state == before
        ic.close()


def test_draws_follow_generate_many():
    """With nothing given, the base draws, probes and steered start times are ``generate_many``'s for the same seed: host
    generator and ``HIPRNG``."""
    case = BY_NAME["gen-readme-vjp-B33"]
    ps, _, _ = _inputs(case.name)
    B = 5
    gl = torch.full((M, B), 1.0 / B, device="cuda")
    for make_rng in (lambda: 7, lambda: cnf.HIPRNG(7)):
        a = make_icnf(cnf, case.cfg, kernel="mfma", rng=make_rng())
        b = make_icnf(cnf, case.cfg, kernel="mfma", rng=make_rng())
        a.steer_rate = b.steer_rate = 0.2
        fx, fq = cnf.generate_many(a, cnf.TrainMode(), _dev(ps), {}, B, with_logp=True)
        ia = a.last_ensemble_info
        xs, lq, _, ib = cnf.generate_vjp_many(b, cnf.TrainMode(), _dev(ps), {}, B, (None, gl))
        assert np.array_equal(_np(ia["z0"]), _np(ib["z0"])) and np.array_equal(_np(ia["eps"]), _np(ib["eps"]))
        assert np.array_equal(ia["t0"], ib["t0"]) and len(set(ib["t0"].tolist())) == M
        assert_parity(_np(xs), _np(fx), "drawn inputs: xs vs generate_many")
        assert_parity(_np(lq), _np(fq), "drawn inputs: logq vs generate_many")
        a.close(); b.close()
