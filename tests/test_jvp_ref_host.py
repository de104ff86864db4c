"""Forward-mode derivatives without a GPU: the reference tests/jvp_ref.py (central differences, the dot identity with the
reverse-mode references, the float32 floor of every device case), the header / binding table of include/cnfhip_jvp.h, and what
``inference_jvp`` / ``generate_jvp`` / ``loss_jvp`` refuse before they touch a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import gen_vjp_ref as GR
from tests import jvp_ref as J
from tests import vjp_ref as V

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cnf_generate_jvp", "cnf_inference_jvp", "cnf_jvp_steps"]
CASES = [(n, m) for n in J.MAIN_NETS for m in J.MODES]
IDS = [f"{n}-{m}" for n, m in CASES]
f64 = lambda a: None if a is None else np.asarray(a, np.float64)


def _setup(net, mode, B=5, sampling=False, **kw):
    cfg = J.case_cfg(net, mode)
    train = mode != "test"
    flat, xs, z0, eps, dps, dxs, dz0 = J.case_inputs(net, mode, B)
    dts = J.host_steps(cfg, flat, z0 if sampling else xs, eps, train, sampling, **kw)
    assert len(dts) >= 2
    return cfg, train, flat, xs, z0, (eps if train else None), dps, dxs, dz0, dts


@pytest.mark.parametrize("net,mode", CASES, ids=IDS)
def test_tangent_matches_central_differences(net, mode):
    """float64: the tangent of ``vjp_ref.outputs`` against central differences along three random directions of ``ps`` and of
    ``xs``, at two step lengths; the two differences agree with each other and with the tangent."""
    cfg, train, flat, xs, _, eps, _, _, _, dts = _setup(net, mode)
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(3):
        dp = rng.standard_normal(flat.size); dp /= np.linalg.norm(dp)
        dx = rng.standard_normal(xs.shape); dx /= np.linalg.norm(dx)
        for d_flat, d_x in ((dp, None), (None, dx)):
            out, an = J.inference_jvp64(cfg, flat, xs, eps, d_flat, d_x, dts, train)
            out0, _, _ = V.outputs(cfg, f64(flat), f64(xs), f64(eps), dts, train=train)
            assert np.allclose(out, out0, rtol=1e-12, atol=1e-13)     # (the exact trace is summed in another order here)
            fds = []
            for h in (1e-4, 1e-5):
                vals = [V.outputs(cfg, f64(flat) + (s * h * d_flat if d_flat is not None else 0.0),
                                  f64(xs) + (s * h * d_x if d_x is not None else 0.0), f64(eps), dts, train=train)[0] for s in (1.0, -1.0)]
                fds.append((vals[0] - vals[1]) / (2 * h))
            s = V.scale(an)
            assert s > 0
            worst = max(worst, np.abs(fds[0] - fds[1]).max() / s, np.abs(fds[1] - an).max() / s)
    print(f"{net} {mode}: central differences off by {worst:.2e} of the tangent's scale")
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("net,mode", CASES, ids=IDS)
def test_sampling_tangent_matches_central_differences(net, mode):
    cfg, train, flat, _, z0, eps, _, _, _, dts = _setup(net, mode, sampling=True)
    rng = np.random.default_rng(4)
    worst = 0.0
    for _ in range(2):
        dp = rng.standard_normal(flat.size); dp /= np.linalg.norm(dp)
        dz = rng.standard_normal(z0.shape); dz /= np.linalg.norm(dz)
        for d_flat, d_z in ((dp, None), (None, dz)):
            (z, lq), (tz, tl) = J.generate_jvp64(cfg, flat, z0, eps, d_flat, d_z, dts, train)
            z1, lq1, _, _ = GR.forward(cfg, f64(flat), f64(z0), f64(eps), dts, train=train)
            assert np.allclose(z, z1, rtol=1e-12, atol=1e-13) and np.allclose(lq, lq1, rtol=1e-12, atol=1e-13)
            h = 1e-5
            vals = [GR.forward(cfg, f64(flat) + (s * h * d_flat if d_flat is not None else 0.0),
                               f64(z0) + (s * h * d_z if d_z is not None else 0.0), f64(eps), dts, train=train)[:2] for s in (1.0, -1.0)]
            worst = max(worst, np.abs((vals[0][0] - vals[1][0]) / (2 * h) - tz).max() / V.scale(tz),
                        np.abs((vals[0][1] - vals[1][1]) / (2 * h) - tl).max() / V.scale(tl))
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("net,mode", CASES, ids=IDS)
def test_dot_identity_with_the_reverse_mode_references(net, mode):
    """float64: sum cot . JVP(v) = <vjp64(cot), v> to 1e-10 of the terms' scale, for inference (``vjp_ref.vjp64``) and for
    sampling (``gen_vjp_ref.vjp64``): the new reference is tied to the one every gradient test rests on."""
    cfg, train, flat, xs, z0, eps, dps, dxs, dz0, dts = _setup(net, mode)
    rng = np.random.default_rng(8)
    B = xs.shape[1]
    cot = rng.standard_normal((4, B))
    _, g, gx = V.vjp64(cfg, flat, xs, eps, cot, dts, train=train)
    _, tan = J.inference_jvp64(cfg, flat, xs, eps, dps[0], dxs[0], dts, train)
    rows = slice(0, 4) if train else slice(0, 1)
    lhs_terms = cot[rows] * tan[rows]
    rhs_terms = np.concatenate([g * f64(dps[0]), (gx * f64(dxs[0])).ravel()])
    tol = 1e-10 * (np.abs(lhs_terms).sum() + np.abs(rhs_terms).sum())
    assert abs(lhs_terms.sum() - rhs_terms.sum()) <= tol, (lhs_terms.sum(), rhs_terms.sum())
    dts_s = J.host_steps(cfg, flat, z0, eps, train, True)
    cz, cl = rng.standard_normal(z0.shape), rng.standard_normal(B)
    _, _, g, gz0, _ = GR.vjp64(cfg, flat, z0, eps, cz, cl, dts_s, train=train)
    _, (tz, tl) = J.generate_jvp64(cfg, flat, z0, eps, dps[1], dz0[1], dts_s, train)
    lhs_terms = np.concatenate([(cz * tz).ravel(), cl * tl])
    rhs_terms = np.concatenate([g * f64(dps[1]), (gz0 * f64(dz0[1])).ravel()])
    tol = 1e-10 * (np.abs(lhs_terms).sum() + np.abs(rhs_terms).sum())
    assert abs(lhs_terms.sum() - rhs_terms.sum()) <= tol, (lhs_terms.sum(), rhs_terms.sum())


def _floors(cfg, train, flat, x, eps, dps, dxs, dts, sampling):
    worst = 0.0
    for dp, dx in ((dps, None), (None, dxs), (dps, dxs)):
        for r in range(len(dp if dp is not None else dx)):
            a, b = (None if dp is None else dp[r]), (None if dx is None else dx[r])
            if sampling:
                _, t64 = J.generate_jvp64(cfg, flat, x, eps, a, b, dts, train)
                _, t32 = J.generate_jvp32(cfg, flat, x, eps, a, b, dts, train)
                pairs = list(zip(t64, t32))
            else:
                _, t64 = J.inference_jvp64(cfg, flat, x, eps, a, b, dts, train)
                _, t32 = J.inference_jvp32(cfg, flat, x, eps, a, b, dts, train)
                pairs = [(t64[i], t32[i]) for i in range(4) if np.abs(t64[i]).max() > 0]
            for r64, r32 in pairs:
                worst = max(worst, J.bar(r64, r32)[1])
    return worst


@pytest.mark.parametrize("sampling", [False, True], ids=["inference", "sampling"])
@pytest.mark.parametrize("net,mode", CASES, ids=IDS)
def test_float32_floor_of_every_gpu_case_is_under_the_cap(net, mode, sampling):
    """The floor of the bar ``rtol = max(1e-4, 8 floor) <= 1e-3``: this reference's float32 run against its float64 run on the
    inputs of the device's parity cases (B = 20, R = 3, the three sets of directions), through the steps the float64 oracle's
    adaptive solve accepts -- never a device number.  At most 1.25e-4 for every tangent array."""
    cfg, train, flat, xs, z0, eps, dps, dxs, dz0, _ = _setup(net, mode, B=20)
    x, dx = (z0, dz0) if sampling else (xs, dxs)
    dts = J.host_steps(cfg, flat, x, eps, train, sampling)
    worst = _floors(cfg, train, flat, x, eps, dps, dx, dts, sampling)
    print(f"{net} {mode} {'sampling' if sampling else 'inference'}: float32 floor {worst:.2e} ({len(dts)} steps)")
    assert worst <= J.FLOOR_CAP, worst


@pytest.mark.parametrize("net,mode", J.EXTRA_CASES, ids=[f"{n}-{m}" for n, m in J.EXTRA_CASES])
def test_the_other_instantiations_reference_and_floor(net, mode):
    """The networks that reach the kernel's other instantiations: the reference against central differences (one direction of each
    kind) and the float32 floor of the device case, inference and sampling."""
    cfg, train, flat, xs, z0, eps, dps, dxs, dz0, dts = _setup(net, mode, B=20)
    h = 1e-5
    for dp, dx in ((dps[0] / np.linalg.norm(dps[0]), None), (None, dxs[0] / np.linalg.norm(dxs[0]))):
        _, an = J.inference_jvp64(cfg, flat, xs, eps, dp, dx, dts, train)
        vals = [V.outputs(cfg, f64(flat) + (s * h * dp if dp is not None else 0.0), f64(xs) + (s * h * dx if dx is not None else 0.0),
                          f64(eps), dts, train=train)[0] for s in (1.0, -1.0)]
        assert np.abs((vals[0] - vals[1]) / (2 * h) - an).max() <= 1e-6 * V.scale(an)
    assert _floors(cfg, train, flat, xs, eps, dps, dxs, dts, False) <= J.FLOOR_CAP
    dts = J.host_steps(cfg, flat, z0, eps, train, True)
    assert _floors(cfg, train, flat, z0, eps, dps, dz0, dts, True) <= J.FLOOR_CAP


def test_float32_floor_of_the_other_gpu_cases():
    """B = 260 (16-48-16, VJP), the stiff inputs of the rejected-attempts case (weights x 2, span (0, 2), first step 1.0, tight
    tolerances) and the forward-mode gradient case (2-6-2, B = 16, the one-hot directions, TrainMode and TestMode)."""
    cfg, train, flat, xs, _, eps, dps, dxs, _, dts = _setup("16-48-16", "vjp", B=260)
    assert _floors(cfg, train, flat, xs, eps, dps[:1], dxs[:1], dts, False) <= J.FLOOR_CAP
    cfg, flat, xs, eps, dps, dxs, kw = stiff_case()
    dts = J.host_steps(cfg, flat, xs, eps, True, False, **kw)
    assert _floors(cfg, True, flat, xs, eps, dps, dxs, dts, False) <= J.FLOOR_CAP
    for mode in ("vjp", "test"):
        cfg, train, flat, xs, _, eps, _, _, _, dts = _setup("2-6-2", mode, B=16)
        n = flat.size
        d64 = np.array([loss_tangent(cfg, J.inference_jvp64(cfg, flat, xs, eps, np.eye(n)[i], None, dts, train)[1], train) for i in range(n)])
        d32 = np.array([loss_tangent(cfg, J.inference_jvp32(cfg, flat, xs, eps, np.eye(n)[i], None, dts, train)[1], train) for i in range(n)])
        assert J.bar(d64, d32)[1] <= J.FLOOR_CAP


def stiff_case():
    """The stiff inputs of tests/ensemble_vjp_ref.py's "rejected attempts" case (its member 0), as one model."""
    from tests import ensemble_vjp_ref as E
    case = next(c for c in E.CASES if c.name == "regr-vjp-B17-rejects")
    ps, xs, eps = E.inputs(case)
    rng = np.random.default_rng(77)
    d = lambda *s: rng.standard_normal((J.R,) + s).astype(np.float32)
    return E.member_cfg(case, 0), ps[0], xs[0], eps[0], d(ps[0].size), d(*xs[0].shape), dict(case.sol_kw)


def loss_tangent(cfg, dout, train):
    dout = np.asarray(dout, np.float64)
    if train:
        return float(np.mean(-dout[0] + cfg.lam1 * dout[1] + cfg.lam2 * dout[2] + cfg.lam3 * dout[3]))
    return float(-np.mean(dout[0]))


def test_header_names_and_bindings():
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_jvp.h"', main, flags=re.M), "cnfhip.h does not include cnfhip_jvp.h"
    raw = open(os.path.join(ROOT, "include", "cnfhip_jvp.h")).read()
    assert "test/call_tests.jl:32-66" in raw and ":239-252" in raw
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", strip(raw))))
    assert declared == NAMES, declared
    assert set(declared) == set(_lib.JVP_EXPORTS)
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("EXPORTS") and n != "JVP_EXPORTS"]
    assert len(others) >= 11
    for table in others:
        assert not set(declared) & set(table)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    assert cnf.inference_jvp is cnf.jvp.inference_jvp and cnf.generate_jvp is cnf.jvp.generate_jvp and cnf.loss_jvp is cnf.jvp.loss_jvp


def _model(**kw):
    nn = cnf.Chain(cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh"))
    return cnf.construct(cnf.RNODE, nn, 1, 1, rng=5, **kw)


def test_argument_checks_raise_value_error_before_a_handle_is_made():
    """Every malformed direction (or eps) is turned away by the check that is about it -- the message says which --, and the same
    call with well-formed directions gets PAST those checks: with host-resident torch tensors it ends at the layout's own
    complaint (they must live on the GPU), whatever machine this runs on."""
    icnf = _model()
    n, B = icnf.nn.n_params_internal, 8
    T = cnf.TrainMode()
    xs, ps, eps = torch.zeros(1, B), torch.zeros(n), torch.zeros(2, B)
    DIRS = r"give a direction|d_ps must be|d_xs must be|d_z0 must be|same number of directions|eps must be"
    bad = [
        (dict(), "give a direction"),                                                              # no direction at all
        (dict(d_ps=torch.zeros(n + 1)), "d_ps must be"),                                           # wrong length
        (dict(d_ps=torch.zeros(2, 3, n)), "d_ps must be"),                                         # too many axes
        (dict(d_xs=torch.zeros(1, B + 1)), "d_xs must be"),                                        # wrong batch
        (dict(d_xs=torch.zeros(2, B)), "d_xs must be"),                                            # wrong rows
        (dict(d_ps=torch.zeros(3, n), d_xs=torch.zeros(2, 1, B)), "same number of directions"),    # different R
        (dict(d_ps=torch.zeros(n), d_xs=torch.zeros(1, 1, B)), "same number of directions"),       # one stacked, one not
        (dict(d_ps=torch.zeros(n), eps=torch.zeros(2, B + 1)), "eps must be"),                     # eps of another batch
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            cnf.inference_jvp(icnf, T, xs, ps, {}, **kw)
        with pytest.raises(ValueError, match=msg):
            cnf.loss_jvp(icnf, T, xs, ps, {}, **kw)
    with pytest.raises(ValueError, match="xs must be"):
        cnf.inference_jvp(icnf, T, torch.zeros(3, B), ps, {}, d_ps=torch.zeros(n))
    good = [dict(d_ps=torch.zeros(n)), dict(d_xs=torch.zeros(1, B)), dict(d_ps=torch.zeros(3, n), d_xs=torch.zeros(3, 1, B)),
            dict(d_ps=torch.zeros(n), d_xs=torch.zeros(1, B), eps=eps)]
    for kw in good:
        for call in (cnf.inference_jvp, cnf.loss_jvp):
            with pytest.raises(ValueError, match="must live on the GPU") as e:
                call(icnf, T, xs, ps, {}, **kw)
            assert not re.search(DIRS, str(e.value))
    z0 = torch.zeros(2, B)
    for kw, msg in ((dict(), "give a direction"), (dict(d_ps=torch.zeros(n - 1)), "d_ps must be"),
                    (dict(d_z0=torch.zeros(2, B + 1)), "d_z0 must be"), (dict(d_z0=torch.zeros(1, B)), "d_z0 must be"),
                    (dict(d_ps=torch.zeros(2, n), d_z0=torch.zeros(3, 2, B)), "same number of directions"),
                    (dict(d_ps=torch.zeros(n), eps=torch.zeros(2, B + 1)), "eps must be")):
        with pytest.raises(ValueError, match=msg):
            cnf.generate_jvp(icnf, T, ps, {}, B, z0=z0, **({"eps": eps} | kw))
    with pytest.raises(ValueError, match="z0 must be"):
        cnf.generate_jvp(icnf, T, ps, {}, B, z0=torch.zeros(2, B + 1), d_ps=torch.zeros(n))
    with pytest.raises(NotImplementedError):                                 # host arrays
        cnf.inference_jvp(icnf, T, xs.numpy(), ps.numpy(), {}, d_ps=np.zeros(n, np.float32))
    with pytest.raises(NotImplementedError):                                 # a host generator and no z0
        cnf.generate_jvp(icnf, T, ps, {}, B, d_ps=torch.zeros(n))
    assert icnf._handle is None


def test_refusals_come_before_anything_is_drawn():
    lay = lambda dims, act="tanh": cnf.Chain(*[cnf.Dense(a, b, act) for a, b in zip(dims[:-1], dims[1:])])
    models = {
        "conditional": cnf.construct(cnf.CondRNODE, lay((4, 6, 2)), 1, 1, rng=5),
        "basedist": cnf.construct(cnf.RNODE, lay((2, 6, 2)), 1, 1, rng=5, basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2)),
        "generic": cnf.construct(cnf.RNODE, lay((2, 6, 2)), 1, 1, rng=5, compute_mode=cnf.HIPVecJacMatrixMode("generic")),
        "headline": cnf.construct(cnf.RNODE, lay((32, 128, 128, 32)), 16, 16, rng=5),
        "wide hidden layer": cnf.construct(cnf.RNODE, lay((2, 80, 2)), 1, 1, rng=5),
        "relu": cnf.construct(cnf.RNODE, lay((2, 6, 2), "relu"), 1, 1, rng=5),
        "planar": cnf.construct(cnf.RNODE, cnf.Chain(cnf.PlanarLayer(2, "tanh")), 2, 0, rng=5),
    }
    for name, ic in models.items():
        before = ic.rng.bit_generator.state
        n_in = ic.nvars + ic.naugmented
        x, p = torch.zeros(ic.nvars, 16), torch.zeros(ic.nn.n_params)
        with pytest.raises(NotImplementedError):
            cnf.inference_jvp(ic, cnf.TrainMode(), x, p, {}, d_ps=torch.zeros_like(p))
        with pytest.raises(NotImplementedError):
            cnf.loss_jvp(ic, cnf.TestMode(), x, p, {}, d_xs=torch.zeros_like(x))
        with pytest.raises(NotImplementedError):
            cnf.generate_jvp(ic, cnf.TrainMode(), p, {}, 16, d_ps=torch.zeros_like(p), z0=torch.zeros(n_in, 16))
        assert ic.rng.bit_generator.state == before and ic._handle is None, name
