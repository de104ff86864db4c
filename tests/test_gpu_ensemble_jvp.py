"""Ensemble forward-mode on the device: ``inference_jvp_many`` / ``generate_jvp_many`` / ``loss_jvp_many``
(cnf_inference_jvp_many, cnf_generate_jvp_many; the ENS form of k_tangent_wave, csrc/cnf_tangent.hip).

Reference and bars: tests/jvp_ref.py unchanged -- the analytic float64 tangent replaying the steps every MEMBER itself accepted
(``info["steps"][m]``), ``max|err| <= rtol (max|ref| + rms ref)`` per tangent array, ``rtol = max(1e-4, 8 floor) <= 1e-3``, the floor
from the float32 run of the same reference.  tests/test_ensemble_jvp_host.py holds the floors of the members used here (the
seeds 0, 1, 2 of ``J.case_inputs`` at B = 33) under ``J.FLOOR_CAP`` on the host oracle's own steps, so the cap hides nothing.
The primal half, the independence of members and directions and the handle afterwards are compared bit for bit.

The parity nets are ``2-6-2`` vjp, ``16-48-16`` jvp and -- for TestMode -- ``2-6-2`` test and ``6-9-6-id`` test (a real identity
second layer: the ID2 instantiations), once also ``2-64-2`` vjp.  ``16-16`` of ``J.NETS`` is a ONE-layer network: no ensemble
call takes one (``ensemble._refusal``; the appended identity layer lives behind the handle's own parameters), so these calls
refuse it like the others do, and ``test_one_layer_networks_are_refused`` says so.
"""
import functools

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import jvp_ref as J
from tests import vjp_ref as V
from tests.helpers import make_icnf
from tests.test_ensemble_jvp_host import B, M, PARITY, SEEDS, member_inputs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
R = J.R
IDS = [f"{n}-{m}" for n, m in PARITY]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


class Ens:
    """M members of one architecture with the inputs of ``J.case_inputs(net, mode, B, seed=m)``."""

    def __init__(self, net, mode, B=B, seeds=SEEDS, cfg=None, inputs=None, sol_kw=None):
        self.cfg = cfg or J.case_cfg(net, mode)
        self.train = mode != "test"
        self.flat, self.xs, self.z0, eps, self.dps, self.dxs, self.dz0 = inputs or member_inputs(net, mode, B, seeds)
        self.eps = eps if self.train else None
        self.M, self.B = self.flat.shape[0], B
        self.ic = make_icnf(cnf, self.cfg, jvp=mode == "jvp", kernel="mfma", sol_kwargs=dict(sol_kw or {}))
        self.T = cnf.TrainMode() if self.train else cnf.TestMode()

    def inference(self, d_ps=None, d_xs=None, sel=slice(None), cols=slice(None), ic=None, fn=None, **kw):
        c = lambda a: None if a is None else _dev(a[sel][..., cols])
        return (fn or cnf.inference_jvp_many)(ic or self.ic, self.T, c(self.xs), _dev(self.flat[sel]), {}, d_ps=_dev(None if d_ps is None else d_ps[sel]),
                                              d_xs=c(d_xs), eps=c(self.eps), **kw)

    def generate(self, d_ps=None, d_z0=None, sel=slice(None), cols=slice(None), ic=None, **kw):
        c = lambda a: None if a is None else _dev(a[sel][..., cols])
        n = c(self.z0).shape[-1]
        return cnf.generate_jvp_many(ic or self.ic, self.T, _dev(self.flat[sel]), {}, n, d_ps=_dev(None if d_ps is None else d_ps[sel]),
                                     d_z0=c(d_z0), z0=c(self.z0), eps=c(self.eps), **kw)


@functools.lru_cache(maxsize=None)
def _ens(net, mode, B=B):
    return Ens(net, mode, B)


def _dts(info, m):
    t, h = info["steps"][m]
    assert len(h) == info["stats"][m]["naccept"] >= 1
    return [abs(float(x)) for x in h]


def _rows(tan):
    """(d_logpx, (d_E, d_n, d_A)) -> (M, R, 4, B) (stacked) or (M, 4, B)."""
    return torch.stack([tan[0], *tan[1]], dim=-2)


def _check_inference(e, tan, info, d_ps, d_xs, what, cfgs=None, counts=None):
    """every member's, direction's and row's tangent against the float64 replay of the member's own steps"""
    d = _rows(tan)
    assert d.shape == (e.M, R, 4, e.B)
    for m in range(e.M):
        k = e.B if counts is None else int(counts[m])
        dts, cfg = _dts(info, m), (e.cfg if cfgs is None else cfgs[m])
        eps = None if e.eps is None else e.eps[m][:, :k]
        for r in range(R):
            a, b = (None if d_ps is None else d_ps[m, r]), (None if d_xs is None else d_xs[m, r][:, :k])
            _, t64 = J.inference_jvp64(cfg, e.flat[m], e.xs[m][:, :k], eps, a, b, dts, e.train)
            _, t32 = J.inference_jvp32(cfg, e.flat[m], e.xs[m][:, :k], eps, a, b, dts, e.train)
            for i, name in enumerate(("d_logpx", "d_E", "d_n", "d_A")):
                J.assert_tangent(_np(d[m, r, i, :k]), t64[i], t32[i], f"{what} m={m} r={r} {name}")


def _check_generate(e, tan, info, d_ps, d_z0, what):
    dz, dl = info["d_z"], tan[1]
    assert dz.shape == (e.M, R, e.cfg.n_in, e.B) and dl.shape == (e.M, R, e.B)
    for m in range(e.M):
        dts = _dts(info, m)
        eps = None if e.eps is None else e.eps[m]
        for r in range(R):
            a, b = (None if d_ps is None else d_ps[m, r]), (None if d_z0 is None else d_z0[m, r])
            _, (z64, l64) = J.generate_jvp64(e.cfg, e.flat[m], e.z0[m], eps, a, b, dts, e.train)
            _, (z32, l32) = J.generate_jvp32(e.cfg, e.flat[m], e.z0[m], eps, a, b, dts, e.train)
            J.assert_tangent(_np(dz[m, r]), z64, z32, f"{what} m={m} r={r} d_z")
            J.assert_tangent(_np(dl[m, r]), l64, l32, f"{what} m={m} r={r} d_logq")
    assert torch.equal(tan[0], dz[:, :, :e.cfg.nvars])


# ---- 1. parity ----
@pytest.mark.parametrize("which", ["ps", "xs", "both"])
@pytest.mark.parametrize("net,mode", PARITY, ids=IDS)
def test_inference_tangent_parity(net, mode, which):
    e = _ens(net, mode)
    d_ps = e.dps if which != "xs" else None
    d_xs = e.dxs if which != "ps" else None
    _, tan, info = e.inference(d_ps, d_xs)
    assert info["calls"] == 1 and not info["rerun"] and info["launches"] == 2
    _check_inference(e, tan, info, d_ps, d_xs, f"inference {net} {mode} {which}")


@pytest.mark.parametrize("which", ["ps", "z0", "both"])
@pytest.mark.parametrize("net,mode", PARITY, ids=IDS)
def test_generate_tangent_parity(net, mode, which):
    e = _ens(net, mode)
    d_ps = e.dps if which != "z0" else None
    d_z0 = e.dz0 if which != "ps" else None
    _, tan, info = e.generate(d_ps, d_z0)
    assert info["calls"] == 1 and not info["rerun"]
    _check_generate(e, tan, info, d_ps, d_z0, f"generate {net} {mode} {which}")


def test_four_hidden_tiles():
    """``2-64-2`` vjp: the instantiation with the most registers, both kinds of direction at once."""
    e = _ens("2-64-2", "vjp")
    _, tan, info = e.inference(e.dps, e.dxs)
    _check_inference(e, tan, info, e.dps, e.dxs, "inference 2-64-2 vjp")
    _, tan, info = e.generate(e.dps, e.dz0)
    _check_generate(e, tan, info, e.dps, e.dz0, "generate 2-64-2 vjp")


def test_one_layer_networks_are_refused():
    """``16-16`` (J.NETS) is one tanh layer: the single-model tangent takes it through its appended identity layer, the ensemble
    calls do not (that layer lives behind the handle's own parameters) -- refused before a handle is made, as by ``inference_many``."""
    ic = make_icnf(cnf, J.case_cfg("16-16", "test"), kernel="auto")
    n = ic.nn.n_params_internal
    for call in (lambda: cnf.inference_many(ic, cnf.TestMode(), torch.zeros(2, 16, 4), torch.zeros(2, n), {}),
                 lambda: cnf.inference_jvp_many(ic, cnf.TestMode(), torch.zeros(2, 16, 4), torch.zeros(2, n), {}, d_ps=torch.zeros(2, n)),
                 lambda: cnf.generate_jvp_many(ic, cnf.TestMode(), torch.zeros(2, n), {}, 4, d_ps=torch.zeros(2, n))):
        with pytest.raises(NotImplementedError, match="no ensemble form"):
            call()
    assert ic._handle is None


# ---- 2. the primal half is the plain ensemble call's ----
@pytest.mark.parametrize("net,mode", PARITY, ids=IDS)
def test_primal_outputs_are_the_plain_ensemble_calls(net, mode):
    e = _ens(net, mode)
    xs, ps, eps, z0 = _dev(e.xs), _dev(e.flat), _dev(e.eps), _dev(e.z0)
    lp0, (e0, n0, a0), i0 = cnf.inference_many(e.ic, e.T, xs, ps, {}, eps=eps)
    (lp, (ee, nn, aa)), _, info = e.inference(e.dps, e.dxs)
    assert torch.equal(lp, lp0) and torch.equal(ee, e0) and torch.equal(nn, n0) and torch.equal(aa, a0)
    assert np.array_equal(info["losses"], i0["losses"])
    for m in range(M):
        assert (info["stats"][m]["naccept"], info["stats"][m]["nreject"]) == (i0["stats"][m]["naccept"], i0["stats"][m]["nreject"])
    assert info["launches"] == i0["launches"] + 1 == 2
    x0, q0 = cnf.generate_many(e.ic, e.T, ps, {}, B, z0=z0, eps=eps, with_logp=True)
    g0 = e.ic.last_ensemble_info
    (x, q), _, info = e.generate(e.dps, e.dz0)
    assert torch.equal(x, x0) and torch.equal(q, q0) and torch.equal(info["z"][:, :e.cfg.nvars], x0)
    for m in range(M):
        assert (info["stats"][m]["naccept"], info["stats"][m]["nreject"]) == (g0["stats"][m]["naccept"], g0["stats"][m]["nreject"])
    assert info["launches"] == g0["launches"] + 1 == 3


# ---- 3. members and directions are independent ----
@pytest.mark.parametrize("net,mode", [("2-6-2", "vjp"), ("16-48-16", "jvp"), ("6-9-6-id", "test")])
def test_members_and_directions_are_independent(net, mode):
    e = _ens(net, mode)
    p3, t3, i3 = e.inference(e.dps, e.dxs)
    d3 = _rows(t3)
    pg, tg, ig = e.generate(e.dps, e.dz0)
    for m in range(M):
        one = slice(m, m + 1)
        p1, t1, i1 = e.inference(e.dps, e.dxs, sel=one)
        assert torch.equal(p1[0][0], p3[0][m]) and all(torch.equal(a[0], b[m]) for a, b in zip(p1[1], p3[1]))
        assert torch.equal(_rows(t1)[0], d3[m]), m
        assert np.array_equal(i1["steps"][0][1], i3["steps"][m][1])
        q1, g1, j1 = e.generate(e.dps, e.dz0, sel=one)
        assert torch.equal(q1[0][0], pg[0][m]) and torch.equal(q1[1][0], pg[1][m])
        assert torch.equal(j1["d_z"][0], ig["d_z"][m]) and torch.equal(g1[1][0], tg[1][m])
    for r in range(R):
        _, t1, _ = e.inference(e.dps[:, r:r + 1], e.dxs[:, r:r + 1])
        assert torch.equal(_rows(t1)[:, 0], d3[:, r]), r
        _, ts, _ = e.inference(e.dps[:, r], e.dxs[:, r])                   # an unstacked direction: no R axis
        assert ts[0].shape == (M, B) and torch.equal(_rows(ts), d3[:, r])
        _, g1, j1 = e.generate(e.dps[:, r], e.dz0[:, r])
        assert g1[1].shape == (M, B) and g1[0].shape == (M, e.cfg.nvars, B)
        assert torch.equal(j1["d_z"], ig["d_z"][:, r]) and torch.equal(g1[1], tg[1][:, r])
    # members 0 and 1 trade parameters and parameter directions, everything else stays: every array moves at its own stride
    swap = [1, 0, 2]
    sw = Ens.__new__(Ens)
    sw.__dict__.update(e.__dict__)
    sw.flat, dps = e.flat[swap], e.dps[swap]
    ps_, ts_, _ = sw.inference(dps, e.dxs)
    for m in (0, 1):
        lone = Ens.__new__(Ens)
        lone.__dict__.update(e.__dict__)
        lone.flat, lone.xs, lone.eps = sw.flat[m:m + 1], e.xs[m:m + 1], (None if e.eps is None else e.eps[m:m + 1])
        p1, t1, _ = lone.inference(dps[m:m + 1], e.dxs[m:m + 1])
        assert torch.equal(p1[0][0], ps_[0][m]) and torch.equal(_rows(t1)[0], _rows(ts_)[m])
        assert not torch.equal(_rows(ts_)[m], d3[m])
    assert torch.equal(_rows(ts_)[2], d3[2]) and torch.equal(ps_[0][2], p3[0][2])


# ---- 4. heterogeneous members ----
@pytest.mark.parametrize("net,mode", [("2-6-2", "vjp"), ("16-48-16", "jvp")])
def test_heterogeneous_members(net, mode):
    e = _ens(net, mode)
    counts = np.asarray([33, 17, 1], dtype=np.int32)
    abstol, reltol = np.asarray([1e-6, 1e-7, 1e-5], np.float32), np.asarray([1e-3, 1e-4, 1e-2], np.float32)
    t1 = np.asarray([1.0, 0.75, 1.25], np.float32)
    kw = dict(counts=counts, reltol=reltol, abstol=abstol)
    p, t, info = e.inference(e.dps, e.dxs, t1=t1, **kw)
    d = _rows(t)
    pg, tg, ig = e.generate(e.dps, e.dz0, t0=t1, **kw)
    cfgs = []
    for m in range(M):
        k = int(counts[m])
        tw = cnf.member_twin(e.ic, tols=(abstol[m], reltol[m]))
        try:
            p1, t1m, i1 = e.inference(e.dps, e.dxs, sel=slice(m, m + 1), cols=slice(0, k), ic=tw, t1=t1[m:m + 1])
            q1, g1, j1 = e.generate(e.dps, e.dz0, sel=slice(m, m + 1), cols=slice(0, k), ic=tw, t0=t1[m:m + 1])
        finally:
            tw.close()
        assert torch.equal(p1[0][0], p[0][m, :k]) and all(torch.equal(a[0], b[m, :k]) for a, b in zip(p1[1], p[1]))
        assert torch.equal(_rows(t1m)[0], d[m, :, :, :k])
        assert torch.isnan(d[m, :, :, k:]).all() and torch.isnan(p[0][m, k:]).all()
        assert torch.equal(q1[0][0], pg[0][m, :, :k]) and torch.equal(q1[1][0], pg[1][m, :k])
        assert torch.equal(j1["d_z"][0], ig["d_z"][m, :, :, :k]) and torch.equal(g1[1][0], tg[1][m, :, :k])
        assert torch.isnan(ig["d_z"][m, :, :, k:]).all() and torch.isnan(tg[1][m, :, k:]).all()
        c = e.cfg
        cfgs.append(J.O.Cfg(c.net, c.nvars, c.naugs, c.lam1, c.lam2, c.lam3, use_jvp=mode == "jvp", tspan=(0.0, float(t1[m]))))
    _check_inference(e, t, info, e.dps, e.dxs, f"heterogeneous {net} {mode}", cfgs=cfgs, counts=counts)
    # the loss: each member's mean over its own count with its own lambdas
    lam = np.asarray([[1e-2, 1e-2, 1e-2], [0.5, 0.25, 2.0], [1e-3, 3.0, 0.125]], np.float32)
    losses, dl = e.inference(e.dps, e.dxs, t1=t1, lambdas=lam, fn=cnf.loss_jvp_many, **kw)
    assert losses.shape == (M,) and dl.shape == (M, R)
    for m in range(M):
        k = int(counts[m])
        l1, l2, l3 = (float(v) for v in lam[m])
        want = (-p[0][m, :k] + l1 * p[1][0][m, :k] + l2 * p[1][1][m, :k] + l3 * p[1][2][m, :k]).mean()
        wd = (-d[m, :, 0, :k] + l1 * d[m, :, 1, :k] + l2 * d[m, :, 2, :k] + l3 * d[m, :, 3, :k]).mean(dim=-1)
        assert losses[m] == np.float32(want.item()) and torch.equal(dl[m], wd), m


# ---- 5. the adjoint identity, per member ----
@pytest.mark.parametrize("net,mode", PARITY, ids=IDS)
def test_adjoint_identity_with_the_ensemble_pullbacks(net, mode):
    """sum cot . tangent = <grads, d_ps> + <grad_x, d_xs> per member, with ``inference_vjp_many`` / ``generate_vjp_many`` on the same
    inputs; the gap allowed is the single-model test's, unchanged: each side's own bar times what multiplies it."""
    e = _ens(net, mode)
    rng = np.random.default_rng(31)
    rows = 4 if e.train else 1
    cot = np.zeros((M, 4, B), np.float32)
    cot[:, :rows] = rng.standard_normal((M, rows, B))
    xs, ps, eps, z0 = _dev(e.xs), _dev(e.flat), _dev(e.eps), _dev(e.z0)
    _, tan, _ = e.inference(e.dps[:, 0], e.dxs[:, 0])
    dd = _np(_rows(tan))
    c = _dev(cot)
    _, _, g, gx, _ = cnf.inference_vjp_many(e.ic, e.T, xs, ps, {}, (c[:, 0], (c[:, 1], c[:, 2], c[:, 3])), eps=eps, with_x=True)
    cz = rng.standard_normal(e.z0.shape).astype(np.float32)
    cl = rng.standard_normal((M, B)).astype(np.float32)
    _, tg, ig = e.generate(e.dps[:, 0], e.dz0[:, 0])
    _, _, gg, gz0, _ = cnf.generate_vjp_many(e.ic, e.T, ps, {}, B, (_dev(cz), _dev(cl)), z0=z0, eps=eps, with_z0=True)
    for m in range(M):
        d, dp, dx = dd[m], e.dps[m, 0], e.dxs[m, 0]
        lhs = float(np.sum(cot[m] * d))
        rhs = float(np.sum(_np(g[m]) * dp) + np.sum(_np(gx[m]) * dx))
        gap = V.RTOL * (sum(V.scale(d[i]) * np.abs(cot[m, i]).sum() for i in range(4)) +
                        V.scale(_np(g[m])) * np.abs(dp).sum() + V.scale(_np(gx[m])) * np.abs(dx).sum())
        print(f"{net} {mode} member {m} inference: {lhs:.6g} against {rhs:.6g}, gap {abs(lhs - rhs):.2e} of {gap:.2e} allowed")
        assert abs(lhs - rhs) <= gap
        dz, dl, d0 = _np(ig["d_z"][m]), _np(tg[1][m]), e.dz0[m, 0]
        lhs = float(np.sum(cz[m] * dz) + np.sum(cl[m] * dl))
        rhs = float(np.sum(_np(gg[m]) * dp) + np.sum(_np(gz0[m]) * d0))
        gap = V.RTOL * (V.scale(dz) * np.abs(cz[m]).sum() + V.scale(dl) * np.abs(cl[m]).sum() +
                        V.scale(_np(gg[m])) * np.abs(dp).sum() + V.scale(_np(gz0[m])) * np.abs(d0).sum())
        print(f"{net} {mode} member {m} sampling: {lhs:.6g} against {rhs:.6g}, gap {abs(lhs - rhs):.2e} of {gap:.2e} allowed")
        assert abs(lhs - rhs) <= gap


# ---- 6. the forward-mode gradient of all members in one call ----
@pytest.mark.parametrize("mode", ["vjp", "test"])
def test_forward_mode_gradient_is_the_reverse_mode_gradient(mode):
    e = Ens("2-6-2", mode, 16)
    n = e.flat.shape[1]
    xs, ps, eps = _dev(e.xs), _dev(e.flat), _dev(e.eps)
    loss0, grads, _ = cnf.loss_and_grad_many(e.ic, e.T, xs, ps, {}, eps=eps)
    eye = torch.eye(n, device="cuda").expand(M, n, n)
    losses, dl = cnf.loss_jvp_many(e.ic, e.T, xs, ps, {}, d_ps=eye, eps=eps)
    assert dl.shape == (M, n) and losses.shape == (M,)
    for m in range(M):
        g = _np(grads[m])
        err = np.abs(_np(dl[m]) - g).max()
        print(f"2-6-2 {mode} member {m}: forward-mode gradient off by {err / V.scale(g):.2e} of the gradient's scale; "
              f"loss {losses[m]:.7g} against {loss0[m]:.7g}")
        assert err <= V.RTOL * V.scale(g)
        assert abs(float(losses[m]) - float(loss0[m])) <= 1e-4 * max(1.0, abs(float(losses[m])))
    e.ic.close()


# ---- 7. rejected attempts ----
def test_rejected_attempts_are_skipped_by_the_member_that_made_them():
    """Member 0 is the stiff case of the single-model test (tests/test_jvp_ref_host.stiff_case: member 0 of the ensemble case
    "regr-vjp-B17-rejects"); members 1 and 2 are that case's other members with their parameters scaled by 1/4, at which the
    float64 oracle's controller accepts every attempt from the case's first step size on (at 1/2 too; at 1 it rejects one)."""
    from tests import ensemble_vjp_ref as E
    case = next(c for c in E.CASES if c.name == "regr-vjp-B17-rejects")
    ps, xs, eps = E.inputs(case)
    ps[1:] *= np.float32(0.25)
    rng = np.random.default_rng(78)
    d = lambda *s: rng.standard_normal((M, R) + s).astype(np.float32)
    cfg = E.member_cfg(case, 0)
    e = Ens(None, "vjp", case.B, cfg=cfg, inputs=(ps, xs, None, eps, d(ps.shape[1]), d(*xs.shape[1:]), None), sol_kw=case.sol_kw)
    _, tan, info = e.inference(e.dps, e.dxs)
    nrej = [info["stats"][m]["nreject"] for m in range(M)]
    assert nrej[0] > 0 and nrej[1] == nrej[2] == 0, nrej
    _check_inference(e, tan, info, e.dps, e.dxs, "rejected attempts")
    e.ic.close()


# ---- 8. members that give up, more members than one launch takes, a non-finite member ----
def test_members_that_give_up_are_rerun():
    """poll_limit = 1 (the knob of the existing fallback tests: a bounded wait, not a fault): with three tiles per member the
    meetings run out; the tangent launch writes nothing for those members, and they are run again alone."""
    e = Ens("16-48-16", "vjp")
    e.ic.set_solve_wait(poll_limit=1)
    try:
        _, tan, info = e.inference(e.dps, e.dxs)
        _, tg, ig = e.generate(e.dps, e.dz0)
    finally:
        e.ic.set_solve_wait(poll_limit=0x7fffffff)
    assert info["rerun"] and ig["rerun"], (info["rerun"], ig["rerun"])
    _check_inference(e, tan, info, e.dps, e.dxs, "rerun")
    _check_generate(e, tg, ig, e.dps, e.dz0, "rerun")
    _, tan, info = e.inference(e.dps, e.dxs)
    assert not info["rerun"]
    _check_inference(e, tan, info, e.dps, e.dxs, "after the wait was restored")
    e.ic.close()


def test_capacity_split_equals_the_parts():
    ic = make_icnf(cnf, J.case_cfg("2-64-2", "vjp"), kernel="mfma", sol_kwargs=dict(adaptive=False, dt=1 / 3))
    B1 = 2048                                              # 128 tiles per member: a handful of members fill the device
    cap = cnf.ensemble_eval_capacity(ic, cnf.TrainMode(), B1)
    assert 1 <= cap <= 64, cap
    Mc = cap + 1
    rng = np.random.default_rng(5)
    n = ic.nn.n_params_internal
    ps = _dev(np.stack([J.O.glorot_params(J.NETS["2-64-2"].net, rng, np.float32, 0.5) for _ in range(Mc)]))
    xs, eps = _dev(rng.standard_normal((Mc, 1, B1))), _dev(rng.standard_normal((Mc, 2, B1)))
    dps = _dev(rng.standard_normal((Mc, n)))
    call = lambda a, b: cnf.inference_jvp_many(ic, cnf.TrainMode(), xs[a:b], ps[a:b], {}, d_ps=dps[a:b], eps=eps[a:b])
    p, t, info = call(0, Mc)
    assert info["calls"] == 2 and info["launches"] == 2
    (pa, ta, _), (pb, tb, _) = call(0, cap), call(cap, Mc)
    assert torch.equal(p[0], torch.cat([pa[0], pb[0]])) and torch.equal(_rows(t), torch.cat([_rows(ta), _rows(tb)]))
    ic.close()


def test_a_nonfinite_member_is_reported_alone():
    import ctypes as C
    e = Ens("2-6-2", "vjp")
    _, t0, _ = e.inference(e.dps, e.dxs)
    bad = Ens.__new__(Ens)
    bad.__dict__.update(e.__dict__)
    bad.xs = e.xs.copy()
    bad.xs[1, 0, 3] = np.nan
    with pytest.raises(cnf.CNFError, match="member 1") as err:
        bad.inference(e.dps, e.dxs)
    assert err.value.status == _lib.ERR_NONFINITE
    # the C ABI: the other members of that very launch are what they are beside a finite member 1; member 1's rows are NaN
    l, h = _lib.lib(), e.ic.handle()
    tr = lambda a: _dev(np.swapaxes(a, -1, -2))
    xr, er, pr, dp, dx = tr(bad.xs), tr(e.eps), _dev(e.flat), _dev(e.dps), tr(e.dxs)
    lp, rg, dout = torch.zeros(M, B, device="cuda"), torch.zeros(M, 3, B, device="cuda"), torch.zeros(M, R, 4, B, device="cuda")
    ls, status = np.empty(M, dtype=np.float32), np.empty(M, dtype=np.int32)
    opts = cnf.base_icnf._solve_opts(e.ic, e.ic.tspan)
    _lib.check(l.cnf_inference_jvp_many(h, _lib.MODE_TRAIN, M, pr.data_ptr(), xr.data_ptr(), er.data_ptr(), B, dp.data_ptr(), dx.data_ptr(), R,
                                        C.byref(opts), None, 0, lp.data_ptr(), rg.data_ptr(), dout.data_ptr(), ls.ctypes.data,
                                        status.ctypes.data, None, None), h)
    assert status.tolist() == [_lib.OK, _lib.ERR_NONFINITE, _lib.OK] and np.isnan(ls[1])
    assert torch.isnan(dout[1]).all() and torch.isnan(lp[1]).all() and torch.isnan(rg[1]).all()
    want = _rows(t0)
    for m in (0, 2):
        assert torch.equal(dout[m], want[m])
    assert l.cnf_ensemble_jvp_steps(h, 1, None, None, 0) == -1 < l.cnf_ensemble_jvp_steps(h, 0, None, None, 0)
    # more attempts than a member has rows for: CNF_ERR_UNSUPPORTED for that member, nothing of it is written
    xr = tr(e.xs)
    _lib.check(l.cnf_inference_jvp_many(h, _lib.MODE_TRAIN, M, pr.data_ptr(), xr.data_ptr(), er.data_ptr(), B, dp.data_ptr(), dx.data_ptr(), R,
                                        C.byref(opts), None, 1, lp.data_ptr(), rg.data_ptr(), dout.data_ptr(), ls.ctypes.data,
                                        status.ctypes.data, None, None), h)
    assert status.tolist() == [_lib.ERR_UNSUPPORTED] * 3 and torch.isnan(dout).all() and torch.isnan(lp).all()
    # ... and Python runs such members again alone
    _, t1, info = e.inference(e.dps, e.dxs, trace_cap=1)
    assert info["rerun"] == [0, 1, 2]
    _check_inference(e, t1, info, e.dps, e.dxs, "trace_cap = 1")
    # refusals of the C call: no direction, R out of range, bases pending
    args = lambda dps, dxs, r: (h, _lib.MODE_TRAIN, M, pr.data_ptr(), xr.data_ptr(), er.data_ptr(), B, dps, dxs, r, C.byref(opts), None, 0,
                                lp.data_ptr(), rg.data_ptr(), dout.data_ptr(), ls.ctypes.data, status.ctypes.data, None, None)
    assert l.cnf_inference_jvp_many(*args(None, None, R)) == _lib.ERR_BAD_ARG
    assert l.cnf_inference_jvp_many(*args(dp.data_ptr(), None, 0)) == _lib.ERR_BAD_ARG
    assert l.cnf_inference_jvp_many(*args(dp.data_ptr(), None, 65536)) == _lib.ERR_BAD_ARG
    mean, scale = torch.zeros(M, 2, device="cuda"), torch.ones(M, 2, device="cuda")
    _lib.check(l.cnf_ensemble_set_bases(h, M, 1, mean.data_ptr(), scale.data_ptr(), None), h)
    assert l.cnf_inference_jvp_many(*args(dp.data_ptr(), dx.data_ptr(), R)) == _lib.ERR_UNSUPPORTED
    assert l.cnf_inference_jvp_many(*args(dp.data_ptr(), dx.data_ptr(), R)) == _lib.OK         # (they were consumed)
    torch.cuda.synchronize()
    assert torch.equal(dout, want)
    e.ic.close()


# ---- 9. the handle afterwards ----
def test_the_handle_is_left_as_it_was():
    e = Ens("2-6-2", "vjp")
    xs, ps, eps = _dev(e.xs[0]), _dev(e.flat[0]), _dev(e.eps[0])
    _, _, i0 = cnf.inference_jvp(e.ic, e.T, xs, ps, {}, d_ps=_dev(e.dps[0]), eps=eps)
    steps0 = [a.copy() for a in i0["steps"]]
    cot = torch.ones(4, B, device="cuda")
    cnf.inference_record(e.ic, e.T, xs, ps, {}, eps=eps)
    g0 = cnf.inference_pullback(e.ic, cot).clone()
    cnf.inference_record(e.ic, e.T, xs, ps, {}, eps=eps)
    e.inference(e.dps, e.dxs)
    e.generate(e.dps, e.dz0)
    g1 = cnf.inference_pullback(e.ic, cot)                  # a record made before the calls still pulls back
    assert torch.equal(g0, g1)
    steps1 = cnf.jvp_steps(e.ic)
    assert np.array_equal(steps0[0], steps1[0]) and np.array_equal(steps0[1], steps1[1])
    e.ic.close()
