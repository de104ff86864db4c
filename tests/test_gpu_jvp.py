"""Forward-mode derivatives on the device: ``inference_jvp`` / ``generate_jvp`` / ``loss_jvp`` (cnf_inference_jvp,
cnf_generate_jvp; k_tangent_wave, csrc/cnf_tangent.hip).

Reference: tests/jvp_ref.py, the analytic float64 tangent replaying the steps the device itself accepted (``info["steps"]``),
held with the project's bar unchanged -- ``max|err| <= rtol (max|ref| + rms ref)`` per tangent array, ``rtol = max(1e-4, 8 floor)
<= 1e-3``, the floor from the float32 run of the same reference (tests/test_jvp_ref_host.py shows it at 1e-6 on every case, so
the bar is 1e-4 throughout).  The primal outputs, the independence of the directions and the state of the handle afterwards are
compared bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import jvp_ref as J
from tests import vjp_ref as V
from tests.helpers import make_icnf
from tests.test_jvp_ref_host import stiff_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
B0 = 20                                                    # two tiles, the second with four live columns
CASES = [(n, m) for n in J.MAIN_NETS for m in J.MODES]
IDS = [f"{n}-{m}" for n, m in CASES]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _mode(train):
    return cnf.TrainMode() if train else cnf.TestMode()


class Model:
    def __init__(self, net, mode, B, cfg=None, inputs=None, sol_kw=None):
        self.cfg = cfg or J.case_cfg(net, mode)
        self.train = mode != "test"
        self.flat, self.xs, self.z0, eps, self.dps, self.dxs, self.dz0 = inputs or J.case_inputs(net, mode, B)
        self.eps = eps if self.train else None
        # (a one-layer network has no MFMA kernel to ask for: "auto" takes it to the wave kernels through its appended identity)
        kernel = "auto" if len(self.cfg.net.acts) == 1 else "mfma"
        self.ic = make_icnf(cnf, self.cfg, jvp=mode == "jvp", kernel=kernel, sol_kwargs=dict(sol_kw or {}))
        self.T = _mode(self.train)

    def inference_jvp(self, d_ps=None, d_xs=None, **kw):
        return cnf.inference_jvp(self.ic, self.T, _dev(self.xs), _dev(self.flat), {}, d_ps=_dev(d_ps), d_xs=_dev(d_xs), eps=_dev(self.eps), **kw)

    def generate_jvp(self, d_ps=None, d_z0=None, **kw):
        return cnf.generate_jvp(self.ic, self.T, _dev(self.flat), {}, self.z0.shape[1], d_ps=_dev(d_ps), d_z0=_dev(d_z0), z0=_dev(self.z0),
                                eps=_dev(self.eps), **kw)


@functools.lru_cache(maxsize=None)
def _model(net, mode, B=B0):
    return Model(net, mode, B)


def _dts(info):
    t, h = info["steps"]
    assert len(h) == info["stats"]["naccept"] >= 1
    return [abs(float(x)) for x in h]


def _check_inference(m, tan, info, d_ps, d_xs, what):
    """every direction's four tangent rows against the float64 replay of the device's own steps"""
    dts = _dts(info)
    d = torch.stack([tan[0], tan[1][0], tan[1][1], tan[1][2]], dim=-2)        # (R, 4, B)
    R = d.shape[0]
    for r in range(R):
        a, b = (None if d_ps is None else d_ps[r]), (None if d_xs is None else d_xs[r])
        _, t64 = J.inference_jvp64(m.cfg, m.flat, m.xs, m.eps, a, b, dts, m.train)
        _, t32 = J.inference_jvp32(m.cfg, m.flat, m.xs, m.eps, a, b, dts, m.train)
        for i, name in enumerate(("d_logpx", "d_E", "d_n", "d_A")):
            J.assert_tangent(_np(d[r, i]), t64[i], t32[i], f"{what} r={r} {name}")


def _check_generate(m, tan, info, d_ps, d_z0, what):
    dts = _dts(info)
    dz, dl = info["d_z"], tan[1]
    for r in range(dz.shape[0]):
        a, b = (None if d_ps is None else d_ps[r]), (None if d_z0 is None else d_z0[r])
        _, (z64, l64) = J.generate_jvp64(m.cfg, m.flat, m.z0, m.eps, a, b, dts, m.train)
        _, (z32, l32) = J.generate_jvp32(m.cfg, m.flat, m.z0, m.eps, a, b, dts, m.train)
        J.assert_tangent(_np(dz[r]), z64, z32, f"{what} r={r} d_z")
        J.assert_tangent(_np(dl[r]), l64, l32, f"{what} r={r} d_logq")
        assert torch.equal(tan[0][r], dz[r][:m.cfg.nvars])


# ---- 1. parity ----
@pytest.mark.parametrize("which", ["ps", "xs", "both"])
@pytest.mark.parametrize("net,mode", CASES, ids=IDS)
def test_inference_tangent_parity(net, mode, which):
    m = _model(net, mode)
    d_ps = m.dps if which != "xs" else None
    d_xs = m.dxs if which != "ps" else None
    _, tan, info = m.inference_jvp(d_ps, d_xs)
    assert info["calls"] == 1
    _check_inference(m, tan, info, d_ps, d_xs, f"inference {net} {mode} {which}")


@pytest.mark.parametrize("which", ["ps", "z0", "both"])
@pytest.mark.parametrize("net,mode", CASES, ids=IDS)
def test_generate_tangent_parity(net, mode, which):
    m = _model(net, mode)
    d_ps = m.dps if which != "z0" else None
    d_z0 = m.dz0 if which != "ps" else None
    _, tan, info = m.generate_jvp(d_ps, d_z0)
    _check_generate(m, tan, info, d_ps, d_z0, f"generate {net} {mode} {which}")


@pytest.mark.parametrize("net,mode", J.EXTRA_CASES, ids=[f"{n}-{m}" for n, m in J.EXTRA_CASES])
def test_the_other_instantiations(net, mode):
    """Two and four hidden tiles (64 hidden units: the instantiations with the most registers) and a real tanh -> identity
    network, whose second layer has a direction: both kinds of direction at once, inference and sampling."""
    m = _model(net, mode)
    _, tan, info = m.inference_jvp(m.dps, m.dxs)
    _check_inference(m, tan, info, m.dps, m.dxs, f"inference {net} {mode}")
    _, tan, info = m.generate_jvp(m.dps, m.dz0)
    _check_generate(m, tan, info, m.dps, m.dz0, f"generate {net} {mode}")


def test_malformed_directions_are_refused_on_the_device_too():
    m = _model("2-6-2", "vjp")
    for kw in (dict(d_ps=m.dps[:, :-1]), dict(d_xs=m.dxs[:, :, :-1]), dict(d_ps=m.dps[:2], d_xs=m.dxs)):
        with pytest.raises(ValueError, match="must be|same number of directions"):
            m.inference_jvp(**kw)
    with pytest.raises(ValueError, match="d_z0 must be"):
        m.generate_jvp(d_z0=m.dz0[:, :1])


def test_more_than_sixteen_tiles():
    m = Model("16-48-16", "vjp", 260)
    _, tan, info = m.inference_jvp(m.dps[:1], m.dxs[:1])
    _check_inference(m, tan, info, m.dps[:1], m.dxs[:1], "inference 16-48-16 vjp B=260")
    _, tan, info = m.generate_jvp(m.dps[:1], m.dz0[:1])
    _check_generate(m, tan, info, m.dps[:1], m.dz0[:1], "generate 16-48-16 vjp B=260")
    m.ic.close()


# ---- 2. the primal half is the plain call's ----
@pytest.mark.parametrize("net,mode", CASES, ids=IDS)
def test_primal_outputs_are_the_plain_calls(net, mode):
    m = _model(net, mode)
    lp0, (e0, n0, a0) = cnf.inference(m.ic, m.T, _dev(m.xs), _dev(m.flat), {}, eps=_dev(m.eps))
    s0 = dict(m.ic.last_stats)
    (lp, (e, n, a)), _, info = m.inference_jvp(m.dps, m.dxs)
    assert torch.equal(lp, lp0) and torch.equal(e, e0) and torch.equal(n, n0) and torch.equal(a, a0)
    assert (info["stats"]["naccept"], info["stats"]["nreject"]) == (s0["naccept"], s0["nreject"])
    assert info["launches"] == s0["launches"] + 1 == 2      # the one-launch solve and the tangent launch behind it
    x0, q0 = cnf.generate(m.ic, m.T, _dev(m.flat), {}, B0, z0=_dev(m.z0), eps=_dev(m.eps), with_logp=True)
    s0 = dict(m.ic.last_stats)
    (x, q), _, info = m.generate_jvp(m.dps, m.dz0)
    print(f"{net} {mode}: xs differ by {float((x - x0).abs().max()):.3g}, logq by {float((q - q0).abs().max()):.3g}; "
          f"steps {info['stats']['naccept']}+{info['stats']['nreject']} against {s0['naccept']}+{s0['nreject']}")
    assert torch.equal(x, x0) and torch.equal(q, q0)
    assert (info["stats"]["naccept"], info["stats"]["nreject"]) == (s0["naccept"], s0["nreject"])
    assert info["launches"] == s0["launches"] + 1           # that call's launches and the tangent launch


# ---- 3. the adjoint identity on the device ----
@pytest.mark.parametrize("net,mode", CASES, ids=IDS)
def test_adjoint_identity_with_the_pullbacks(net, mode):
    """sum cot . tangent = <grads, d_ps> + <grad_x, d_xs> with the record / pullback calls on the same inputs; the gap allowed is
    each side's own bar (1e-4 of the scale of every array it is made of) times what multiplies it."""
    m = _model(net, mode)
    rng = np.random.default_rng(31)
    rows = 4 if m.train else 1
    cot = np.zeros((4, B0), np.float32)
    cot[:rows] = rng.standard_normal((rows, B0))
    _, tan, _ = m.inference_jvp(m.dps[:1], m.dxs[:1])
    d = np.stack([_np(tan[0][0]), _np(tan[1][0][0]), _np(tan[1][1][0]), _np(tan[1][2][0])])
    cnf.inference_record(m.ic, m.T, _dev(m.xs), _dev(m.flat), {}, eps=_dev(m.eps))
    g, gx = cnf.inference_pullback(m.ic, _dev(cot), with_x=True)
    lhs = float(np.sum(cot * d))
    rhs = float(np.sum(_np(g) * m.dps[0]) + np.sum(_np(gx) * m.dxs[0]))
    gap = V.RTOL * (sum(V.scale(d[i]) * np.abs(cot[i]).sum() for i in range(4)) +
                    V.scale(_np(g)) * np.abs(m.dps[0]).sum() + V.scale(_np(gx)) * np.abs(m.dxs[0]).sum())
    print(f"{net} {mode} inference: {lhs:.6g} against {rhs:.6g}, gap {abs(lhs - rhs):.2e} of {gap:.2e} allowed")
    assert abs(lhs - rhs) <= gap
    cz = rng.standard_normal(m.z0.shape).astype(np.float32)
    cl = rng.standard_normal(B0).astype(np.float32)
    _, tan, info = m.generate_jvp(m.dps[:1], m.dz0[:1])
    dz, dl = _np(info["d_z"][0]), _np(tan[1][0])
    cnf.generate_record(m.ic, m.T, _dev(m.flat), {}, B0, z0=_dev(m.z0), eps=_dev(m.eps))
    g, gz0 = cnf.generate_pullback(m.ic, (_dev(cz), _dev(cl)), with_z0=True)
    lhs = float(np.sum(cz * dz) + np.sum(cl * dl))
    rhs = float(np.sum(_np(g) * m.dps[0]) + np.sum(_np(gz0) * m.dz0[0]))
    gap = V.RTOL * (V.scale(dz) * np.abs(cz).sum() + V.scale(dl) * np.abs(cl).sum() +
                    V.scale(_np(g)) * np.abs(m.dps[0]).sum() + V.scale(_np(gz0)) * np.abs(m.dz0[0]).sum())
    print(f"{net} {mode} sampling: {lhs:.6g} against {rhs:.6g}, gap {abs(lhs - rhs):.2e} of {gap:.2e} allowed")
    assert abs(lhs - rhs) <= gap


# ---- 4. the directions are independent, and the map is linear ----
@pytest.mark.parametrize("net,mode", [("2-6-2", "vjp"), ("16-48-16", "jvp"), ("16-16", "test")])
def test_directions_are_independent_and_linear(net, mode):
    m = _model(net, mode)
    _, t3, _ = m.inference_jvp(m.dps, m.dxs)
    d3 = torch.stack([t3[0], *t3[1]], dim=-2)
    for r in range(J.R):
        _, t1, _ = m.inference_jvp(m.dps[r:r + 1], m.dxs[r:r + 1])
        assert torch.equal(torch.stack([t1[0], *t1[1]], dim=-2)[0], d3[r]), r
        _, ts, _ = m.inference_jvp(m.dps[r], m.dxs[r])                     # an unstacked direction: no leading axis
        assert ts[0].shape == (B0,) and torch.equal(torch.stack([ts[0], *ts[1]], dim=-2), d3[r])
    lin = _np(d3[0]) + 2.0 * _np(d3[1])                                    # (direction 2 is v_0 + 2 v_1)
    for i in range(4):
        s = V.scale(lin[i])
        assert np.abs(_np(d3[2, i]) - lin[i]).max() <= V.RTOL * s, (i, s)
    _, g3, i3 = m.generate_jvp(m.dps, m.dz0)
    for r in range(J.R):
        _, g1, i1 = m.generate_jvp(m.dps[r:r + 1], m.dz0[r:r + 1])
        assert torch.equal(i1["d_z"][0], i3["d_z"][r]) and torch.equal(g1[1][0], g3[1][r])
    assert np.abs(_np(g3[1][2]) - _np(g3[1][0]) - 2.0 * _np(g3[1][1])).max() <= V.RTOL * V.scale(_np(g3[1][2]))


# ---- 5. rejected attempts ----
def test_rejected_attempts_are_skipped():
    cfg, flat, xs, eps, dps, dxs, kw = stiff_case()
    m = Model(None, "vjp", xs.shape[1], cfg=cfg, inputs=(flat, xs, None, eps, dps, dxs, None), sol_kw=kw)
    _, tan, info = m.inference_jvp(dps, dxs)
    assert info["stats"]["nreject"] > 0, info["stats"]
    _check_inference(m, tan, info, dps, dxs, "rejected attempts")
    m.ic.close()


# ---- 6. the forward-mode gradient as the reference takes it ----
@pytest.mark.parametrize("mode", ["vjp", "test"])
def test_forward_mode_gradient_is_the_reverse_mode_gradient(mode):
    m = Model("2-6-2", mode, 16)
    n = m.flat.size
    loss0, grad = cnf.loss_and_grad(m.ic, m.T, _dev(m.xs), _dev(m.flat), {}, eps=_dev(m.eps))
    loss, dl = cnf.loss_jvp(m.ic, m.T, _dev(m.xs), _dev(m.flat), {}, d_ps=torch.eye(n, device="cuda"), eps=_dev(m.eps))
    assert dl.shape == (n,)
    g = _np(grad)
    err = np.abs(_np(dl) - g).max()
    print(f"2-6-2 {mode}: forward-mode gradient off by {err / V.scale(g):.2e} of the gradient's scale; loss {loss:.7g} against {loss0:.7g}")
    assert err <= V.RTOL * V.scale(g)
    assert abs(loss - float(loss0)) <= 1e-4 * max(1.0, abs(loss))
    m.ic.close()


# ---- 7. the handle afterwards ----
def test_the_handle_is_left_as_it_was():
    m = Model("2-6-2", "vjp", B0)
    xs, ps, eps = _dev(m.xs), _dev(m.flat), _dev(m.eps)
    lp0, r0 = cnf.inference(m.ic, m.T, xs, ps, {}, eps=eps)
    l0, g0 = cnf.loss_and_grad(m.ic, m.T, xs, ps, {}, eps=eps)
    lp0, g0 = lp0.clone(), g0.clone()
    # a record ends with any solve: the pullback behind a tangent call fails exactly as behind a plain inference
    cot = torch.ones(4, B0, device="cuda")
    cnf.inference_record(m.ic, m.T, xs, ps, {}, eps=eps)
    cnf.inference(m.ic, m.T, xs, ps, {}, eps=eps)
    with pytest.raises(cnf.CNFError) as e0:
        cnf.inference_pullback(m.ic, cot)
    cnf.inference_record(m.ic, m.T, xs, ps, {}, eps=eps)
    m.inference_jvp(m.dps, m.dxs)
    with pytest.raises(cnf.CNFError) as e1:
        cnf.inference_pullback(m.ic, cot)
    assert e0.value.status == e1.value.status == _lib.ERR_BAD_ARG
    m.generate_jvp(m.dps, m.dz0)
    lp1, r1 = cnf.inference(m.ic, m.T, xs, ps, {}, eps=eps)
    l1, g1 = cnf.loss_and_grad(m.ic, m.T, xs, ps, {}, eps=eps)
    assert torch.equal(lp0, lp1) and float(l0) == float(l1) and torch.equal(g0, g1)
    m.ic.close()


# ---- the route when the one-launch solve gives up (the knob of the existing fallback tests: a bounded wait, not a fault) ----
def test_fallback_route_files_its_steps():
    m = Model("16-48-16", "vjp", 68)                       # five tiles: one per workgroup, they have to meet
    fb0 = m.ic.solve_fallbacks()
    m.ic.set_solve_wait(0, 1)
    try:
        _, tan, info = m.inference_jvp(m.dps, m.dxs)
    finally:
        m.ic.set_solve_wait(0, 0x7fffffff)
    assert m.ic.solve_fallbacks() == fb0 + 1 and info["launches"] > 2
    _check_inference(m, tan, info, m.dps, m.dxs, "fallback route")
    m.ic.close()


# ---- 8. the raw C calls ----
def _raw_inference(ic, m, xs, eps, B, dps, dxs, R, opts, trace_cap, lp, rg, dout):
    st = _lib.cnf_solve_stats()
    return _lib.lib().cnf_inference_jvp(ic.handle(), m, xs.data_ptr(), eps.data_ptr() if eps is not None else None, B,
                                        dps.data_ptr() if dps is not None else None, dxs.data_ptr() if dxs is not None else None, R,
                                        C.byref(opts) if opts is not None else None, trace_cap, lp.data_ptr(), rg.data_ptr(),
                                        dout.data_ptr(), C.byref(st), None)


def test_raw_calls_refuse_and_leave_the_outputs_alone():
    from continuousnf.jl_amd.base_icnf import _solve_opts
    m = Model("2-6-2", "vjp", B0)
    ic = m.ic
    ic.set_params(_dev(m.flat))
    n = m.flat.size
    xs, eps = _dev(m.xs.T), _dev(m.eps.T)                   # [B][rows]
    dps, dxs = _dev(m.dps), _dev(np.transpose(m.dxs, (0, 2, 1)))
    opts = _solve_opts(ic, (0.0, 1.0))
    mk = lambda *s: torch.full(s, 7.0, device="cuda")
    lp, rg, dout = mk(B0), mk(3 * B0), mk(J.R, 4, B0)
    untouched = lambda: bool((lp == 7).all() and (rg == 7).all() and (dout == 7).all())
    T = _lib.MODE_TRAIN
    assert _raw_inference(ic, T, xs, eps, B0, None, None, J.R, opts, 0, lp, rg, dout) == _lib.ERR_BAD_ARG       # no direction
    assert _raw_inference(ic, T, xs, eps, B0, dps, dxs, 0, opts, 0, lp, rg, dout) == _lib.ERR_BAD_ARG          # R = 0
    assert _raw_inference(ic, T, xs, eps, B0, dps, dxs, 65536, opts, 0, lp, rg, dout) == _lib.ERR_BAD_ARG
    assert _raw_inference(ic, T, xs, None, B0, dps, dxs, J.R, opts, 0, lp, rg, dout) == _lib.ERR_BAD_ARG       # TrainMode without eps
    assert _raw_inference(ic, T, xs, eps, B0, dps, dxs, J.R, None, 0, lp, rg, dout) == _lib.ERR_BAD_ARG
    assert _raw_inference(ic, T, xs, eps, B0, dps, dxs, J.R, opts, -1, lp, rg, dout) == _lib.ERR_BAD_ARG
    assert _raw_inference(ic, T, xs, eps, 0, dps, dxs, J.R, opts, 0, lp, rg, dout) == _lib.ERR_BAD_SHAPE
    assert untouched()
    # more attempts than the trace holds: refused, nothing written; the handle goes on
    assert _raw_inference(ic, T, xs, eps, B0, dps, dxs, J.R, opts, 2, lp, rg, dout) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert untouched() and _lib.lib().cnf_jvp_steps(ic.handle(), None, None, 0) == -1
    assert _raw_inference(ic, T, xs, eps, B0, dps, dxs, J.R, opts, 0, lp, rg, dout) == _lib.OK
    torch.cuda.synchronize()
    assert not untouched() and _lib.lib().cnf_jvp_steps(ic.handle(), None, None, 0) >= 3
    _, tan, _ = m.inference_jvp(m.dps, m.dxs)
    assert torch.equal(dout[:, 0], tan[0])
    ic.close()
    # outside the envelope: a wide network, a conditional one, a non-default base
    wide = cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 80, "tanh"), cnf.Dense(80, 2, "tanh")), 1, 1, rng=5)
    wide.set_params(torch.zeros(wide.nn.n_params, device="cuda"))
    lp, rg, dout = mk(B0), mk(3 * B0), mk(1, 4, B0)
    dp = torch.zeros(1, wide.nn.n_params, device="cuda")
    assert _raw_inference(wide, T, xs, eps, B0, dp, None, 1, opts, 0, lp, rg, dout) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert untouched()
    wide.close()
    based = cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh")), 1, 1, rng=5,
                          basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2))
    based.set_params(_dev(m.flat))
    assert _raw_inference(based, T, xs, eps, B0, dps, None, J.R, opts, 0, lp, rg, mk(J.R, 4, B0)) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((lp == 7).all() and (rg == 7).all())
    based.close()
    cond = cnf.construct(cnf.CondRNODE, cnf.Chain(cnf.Dense(4, 6, "tanh"), cnf.Dense(6, 2, "tanh")), 1, 1, rng=5)
    cond.set_params(torch.zeros(cond.nn.n_params, device="cuda"))
    dpc = torch.zeros(1, cond.nn.n_params, device="cuda")
    assert _raw_inference(cond, T, xs, eps, B0, dpc, None, 1, opts, 0, lp, rg, mk(1, 4, B0)) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((lp == 7).all() and (rg == 7).all())
    cond.close()


def _raw_generate(ic, m, z0, eps, B, dps, dz0, R, opts, trace_cap, z, lq, dz, dlq):
    st = _lib.cnf_solve_stats()
    p = lambda t: t.data_ptr() if t is not None else None
    return _lib.lib().cnf_generate_jvp(ic.handle(), m, p(z0), p(eps), B, p(dps), p(dz0), R, C.byref(opts) if opts is not None else None,
                                       trace_cap, p(z), p(lq), p(dz), p(dlq), C.byref(st), None)


def test_raw_sampling_calls_refuse_and_leave_the_outputs_alone():
    from continuousnf.jl_amd.base_icnf import _solve_opts
    m = Model("2-6-2", "vjp", B0)
    ic = m.ic
    ic.set_params(_dev(m.flat))
    z0, eps = _dev(m.z0.T), _dev(m.eps.T)                   # [B][rows]
    dps, dz0 = _dev(m.dps), _dev(np.transpose(m.dz0, (0, 2, 1)))
    opts = _solve_opts(ic, (1.0, 0.0))                     # reverse(tspan)
    mk = lambda *s: torch.full(s, 7.0, device="cuda")
    z, lq, dz, dlq = mk(B0, 2), mk(B0), mk(J.R, B0, 2), mk(J.R, B0)
    untouched = lambda: all(bool((t == 7).all()) for t in (z, lq, dz, dlq))
    T = _lib.MODE_TRAIN
    steps = lambda: _lib.lib().cnf_jvp_steps(ic.handle(), None, None, 0)
    assert _raw_generate(ic, T, z0, eps, B0, None, None, J.R, opts, 0, z, lq, dz, dlq) == _lib.ERR_BAD_ARG       # no direction
    assert _raw_generate(ic, T, z0, eps, B0, dps, dz0, 0, opts, 0, z, lq, dz, dlq) == _lib.ERR_BAD_ARG          # R = 0
    assert _raw_generate(ic, T, z0, None, B0, dps, dz0, J.R, opts, 0, z, lq, dz, dlq) == _lib.ERR_BAD_ARG       # TrainMode without eps
    assert _raw_generate(ic, T, z0, eps, B0, dps, dz0, J.R, opts, 0, z, lq, dz, None) == _lib.ERR_BAD_ARG       # a null output
    assert _raw_generate(ic, T, z0, eps, B0, dps, dz0, J.R, opts, 65537, z, lq, dz, dlq) == _lib.ERR_BAD_ARG
    assert _raw_generate(ic, T, z0, eps, 0, dps, dz0, J.R, opts, 0, z, lq, dz, dlq) == _lib.ERR_BAD_SHAPE
    assert untouched()
    # more steps than the trace holds: refused, nothing written, no steps on record; the handle goes on
    assert _raw_generate(ic, T, z0, eps, B0, dps, dz0, J.R, opts, 2, z, lq, dz, dlq) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert untouched() and steps() == -1
    assert _raw_generate(ic, T, z0, eps, B0, dps, dz0, J.R, opts, 0, z, lq, dz, dlq) == _lib.OK
    torch.cuda.synchronize()
    assert not untouched() and steps() >= 3
    _, tan, info = m.generate_jvp(m.dps, m.dz0)
    assert torch.equal(dlq, tan[1]) and torch.equal(dz.permute(0, 2, 1), info["d_z"])
    ic.close()
    wide = cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 80, "tanh"), cnf.Dense(80, 2, "tanh")), 1, 1, rng=5)
    wide.set_params(torch.zeros(wide.nn.n_params, device="cuda"))
    z, lq, dz, dlq = mk(B0, 2), mk(B0), mk(1, B0, 2), mk(1, B0)
    dp = torch.zeros(1, wide.nn.n_params, device="cuda")
    assert _raw_generate(wide, T, z0, eps, B0, dp, None, 1, opts, 0, z, lq, dz, dlq) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert untouched() and _lib.lib().cnf_jvp_steps(wide.handle(), None, None, 0) == -1
    wide.close()
