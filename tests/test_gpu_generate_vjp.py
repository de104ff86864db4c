"""Differentiable sampling on the device: ``generate_record`` / ``generate_pullback`` / ``differentiable_generate`` against the
float64 reference of tests/gen_vjp_ref.py, on every pullback route -- all of them in reverse time, which is how sampling
integrates.

Cases: ``grad_terms.GPU_CASES`` by name (one or two per route; the ``wave`` shape exercises the hand-over to the recorded
route) with lam = (1, 1, 1) ((1, 1, 0) without augmented rows), so that the E and n rows are integrated and must not leak into
a pullback that gives them no cotangent; ``z0`` is drawn with ``seed + 11`` on all n_in rows.  From ONE record three pullbacks:
a cotangent on the samples alone, on logq alone, on both (N(0, 1)/B entries); with augmented rows one more with a cotangent
on all n_in rows of the final state.  TestMode legs (k_adj_test) and one full-covariance ``basedist``.

Bar (tests/vjp_ref.assert_vjp, unchanged, with grad_z0 in the place of grad_x): per parameter block and for grad_z0
max|got - ref64| <= rtol (max|ref64| + rms ref64), rtol = max(1e-4, 8 floor) <= 1e-3, floor = the error of the float32 run of
the same reference over that scale; grad_ys at cond_grad_ref.assert_ys's.  Forward ``xs`` / ``logq``: helpers.assert_parity
against the float64 reference on the device's own steps.
"""
import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from oracle import cnf_oracle as O
from tests import basedist_ref as BR
from tests import cond_grad_ref as CR
from tests import gen_vjp_ref as R
from tests import grad_terms as GT
from tests import helpers
from tests import vjp_ref as V
from tests.test_gen_vjp_ref_host import TEST_CASES, basedist_inputs, inputs_of_testmode, lam_of
from tests.test_gpu_grad_terms import _forced_split, _model
from tests.test_gpu_inference_vjp import _block_bar
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = O.ACT_TANH
f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
_REF = {}                                   # (case, cotangent, steps) -> (ref64, ref32): one reference for both launch forms


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _record(icnf, mode, flat, z0, eps, ys):
    """(xs, logq, z, steps) of one recorded sampling solve, as numpy."""
    xs, logq = cnf.generate_record(icnf, mode, flat, {}, z0.shape[1], ys=_dev(ys) if ys is not None else None, z0=_dev(z0),
                                   eps=_dev(eps) if eps is not None else None)
    return _np(xs), _np(logq), _np(icnf._record["z"]), [float(d) for d in icnf.last_steps]


def _pull(icnf, cot, with_ys=False):
    cz, cl = cot
    res = cnf.generate_pullback(icnf, (None if cz is None else _dev(cz), None if cl is None else _dev(cl)), with_z0=True,
                                with_ys=with_ys)
    return tuple(_np(r) for r in res)


def _reference(key, cfg, flat, z0, eps, ys, cot, dts, train=True, base=None):
    if key not in _REF:
        _REF[key] = (R.vjp64(cfg, flat, z0, eps, cot[0], cot[1], dts, ys, train, base),
                     R.vjp32(cfg, flat, z0, eps, cot[0], cot[1], dts, ys, train, base))
    return _REF[key]


def _check_forward(what, cfg, xs, logq, z, ref):
    z64, q64 = ref[0], ref[1]
    assert xs.shape == (cfg.nvars, z64.shape[1]) and z.shape == z64.shape and logq.shape == q64.shape, what
    assert np.array_equal(xs, z[:cfg.nvars]), what
    helpers.assert_parity(z, z64, f"{what}: final state against the reference on the device's steps")
    helpers.assert_parity(logq, q64, f"{what}: logq against the reference on the device's steps")


def _check_pullbacks(what, net, got, refs, cond):
    for k, g in got.items():
        r64, r32 = refs[k]
        V.assert_vjp(g[0], g[1], (r64[2], r64[3]), (r32[2], r32[3]), net, f"{what} cot={k}")
        if cond:
            CR.assert_ys(g[2], r64[4], r32[4], f"{what} cot={k}")


ROUTES = [("generic-cfg2", None), ("adj3b-B1-fixed", 0), ("adj3b-B1-fixed", 1), ("adj3b-B33-fixed", 0), ("adj3b-B33-fixed", 1),
          ("adj3b-B77-replay", None), ("adj3-30x120x116-aug", None), ("mfma-cfg5-vjp", None), ("mfma-12x64x48-cond-jvp", None),
          ("wave-16x48-B32-replay", None)]


@pytest.mark.parametrize("name,split", ROUTES, ids=[n if s is None else f"{n}-split{s}" for n, s in ROUTES])
def test_routes_against_the_reference(name, split):
    """Forward outputs and three (four with augmented rows) pullbacks from one record, in reverse time, on every route."""
    case = GT.GPU_CASES[name]
    flat, _, eps, ys = case.inputs()
    z0 = R.case_z0(case)
    cfg = case.cfg(lam_of(case))
    cond = ys is not None
    cots = R.cotangents(np.random.default_rng(case.seed + 7), cfg.n_in, case.nvars, case.B, aug_rows=case.naugs > 0)
    with _forced_split(split):
        icnf = _model(case, lam_of(case))
        try:
            xs, logq, z, steps = _record(icnf, cnf.TrainMode(), flat, z0, eps, ys)
            st = dict(icnf.last_stats)
            got = {k: _pull(icnf, c, with_ys=cond) for k, c in cots.items()}          # all from one record
        finally:
            icnf.close()
    assert all(d < 0 for d in steps), (name, steps)                                   # reverse(tspan) of an increasing span
    print(f"generate | {name} split={split}: {st}")
    if case.route != "wave":                                                          # (the solve kernel family the route belongs to)
        assert st["kernel_used"] == (_lib.KERNEL_GENERIC if case.route == "generic" else _lib.KERNEL_MFMA), (name, st)
    assert st["naccept"] == len(steps), (name, st, steps)
    if case.steps[0] == "fixed":
        assert len(steps) == round(abs(case.tspan[1] - case.tspan[0]) / case.steps[1]), (name, steps)
    dts = [abs(d) for d in steps]
    refs = {k: _reference((name, k, tuple(dts)), cfg, flat, z0, eps, ys, c, dts) for k, c in cots.items()}
    _check_forward(name, cfg, xs, logq, z, refs["both"][0])
    _check_pullbacks(f"{name} split={split}", case.net, got, refs, cond)


@pytest.mark.parametrize("dims,nvars,naugs,B,ncond", TEST_CASES, ids=["32x128x128x32-B16", "12x64x48x12-cond-B24"])
def test_testmode(dims, nvars, naugs, B, ncond):
    """k_adj_test in reverse time with the terminal cotangent of sampling; logq is exact (no probes)."""
    net, cfg, flat, z0, ys = inputs_of_testmode(dims, nvars, naugs, B, ncond)
    layers = [cnf.Dense(a, b, helpers.ACT_NAME[k]) for a, b, k in zip(net.dims[:-1], net.dims[1:], net.acts)]
    icnf = cnf.construct(cnf.CondRNODE if ncond else cnf.RNODE, cnf.Chain(*layers), nvars, naugs, tspan=(0.0, 0.5),
                         sol_kwargs=dict(adaptive=False, dt=0.25), rng=0)
    cots = R.cotangents(np.random.default_rng(7), nvars + naugs, nvars, B)
    try:
        xs, logq, z, steps = _record(icnf, cnf.TestMode(), flat, z0, None, ys)
        got = {k: _pull(icnf, c, with_ys=bool(ncond)) for k, c in cots.items()}
    finally:
        icnf.close()
    assert steps == [-0.25, -0.25], steps
    refs = {k: _reference(("test", dims, k), cfg, flat, z0, None, ys, c, [0.25, 0.25], train=False) for k, c in cots.items()}
    _check_forward(f"TestMode {dims}", cfg, xs, logq, z, refs["both"][0])
    _check_pullbacks(f"TestMode {dims}", net, got, refs, bool(ncond))


def _basedist_model(case, mean, cov):
    layers = [cnf.Dense(a, b, "tanh") for a, b in zip(case.dims[:-1], case.dims[1:])]
    return cnf.construct(cnf.FFJORD, cnf.Chain(*layers), 8, 8, tspan=case.tspan, lambda1=1.0, lambda2=1.0, lambda3=1.0,
                         sol_kwargs=case.sol_kw, rng=0, basedist=cnf.MvNormal(mean, cov))


def test_full_covariance_basedist():
    """A non-default base: logpdf(basedist, z0) in logq and its gradient in grad_z0 go through the precision factor."""
    case, mean, cov = basedist_inputs()
    g = BR.Gauss(mean, cov)
    flat, _, eps, _ = case.inputs()
    z0 = g.sample_from(R.case_z0(case)).astype(np.float32)
    cots = R.cotangents(np.random.default_rng(9), 16, 8, case.B)
    icnf = _basedist_model(case, mean, cov)
    try:
        xs, logq, z, steps = _record(icnf, cnf.TrainMode(), flat, z0, eps, None)
        got = {k: _pull(icnf, c) for k, c in cots.items()}
    finally:
        icnf.close()
    cfg, dts = case.cfg((1.0, 1.0, 1.0)), [abs(d) for d in steps]
    refs = {k: _reference(("basedist", k), cfg, flat, z0, eps, None, c, dts, base=g) for k, c in cots.items()}
    _check_forward("basedist", cfg, xs, logq, z, refs["both"][0])
    _check_pullbacks("basedist", case.net, got, refs, False)


def test_generate_with_logp_and_rand_with_logpdf_are_the_record():
    """``generate(with_logp=True)`` and ``rand(d, n, with_logpdf=True)`` return what the record entry point returns;
    ``generate`` without the flag returns the same samples as it always has, at the parity bar."""
    case = GT.GPU_CASES["adj3-30x120x116-aug"]
    flat, _, eps, _ = case.inputs()
    z0 = R.case_z0(case)
    B = case.B
    icnf = _model(case, lam_of(case))
    try:
        kw = dict(z0=_dev(z0), eps=_dev(eps))
        plain = _np(cnf.generate(icnf, cnf.TrainMode(), flat, {}, B, **kw))
        xs, logq, _, steps = _record(icnf, cnf.TrainMode(), flat, z0, eps, None)
        xs1, logq1 = cnf.generate(icnf, cnf.TrainMode(), flat, {}, B, with_logp=True, **kw)
        xs2, logq2 = cnf.rand(cnf.ICNFDist(icnf, cnf.TrainMode(), flat, {}), B, with_logpdf=True, **kw)
        x1, q1 = cnf.rand(cnf.ICNFDist(icnf, cnf.TrainMode(), flat, {}), z0=_dev(z0[:, :1]), eps=_dev(eps[:, :1]), with_logpdf=True)
        hx, hq = cnf.generate(icnf, cnf.TrainMode(), flat, {}, B, z0=z0, eps=eps, with_logp=True)      # host arrays in, host arrays out
    finally:
        icnf.close()
    assert plain.shape == (case.nvars, B)
    for a, b in ((xs1, logq1), (xs2, logq2)):
        assert np.array_equal(_np(a), xs) and np.array_equal(_np(b), logq)
    assert isinstance(hx, np.ndarray) and np.array_equal(hx, xs) and np.array_equal(hq, logq)
    assert x1.shape == (case.nvars,) and q1.dim() == 0
    helpers.assert_parity(plain, xs, "generate without the flag against the recorded samples")
    dts = [abs(d) for d in steps]
    z64, q64, _, _ = R.forward(case.cfg(lam_of(case)), f64(flat), f64(z0), f64(eps), dts)
    helpers.assert_parity(plain, z64[:case.nvars], "generate without the flag against the reference")
    helpers.assert_parity(_np(x1), z64[:case.nvars, 0], "one draw against the reference")
    helpers.assert_parity(np.array([float(q1)]), q64[:1], "logq of one draw against the reference")


@pytest.mark.parametrize("name", ["adj3b-B33-fixed", "generic-cfg2"])
def test_linearity_from_one_record(name):
    case = GT.GPU_CASES[name]
    flat, _, eps, _ = case.inputs()
    z0 = R.case_z0(case)
    rng = np.random.default_rng(11)
    n_in, B = case.nvars + case.naugs, case.B
    d = lambda *s: (rng.standard_normal(s) / B).astype(np.float32)
    c1, c2 = (d(n_in, B), d(B)), (d(n_in, B), d(B))
    a = np.float32(-1.75)
    icnf = _model(case, lam_of(case))
    try:
        _record(icnf, cnf.TrainMode(), flat, z0, eps, None)
        p1, p2, p12 = _pull(icnf, c1), _pull(icnf, c2), _pull(icnf, (a * c1[0] + c2[0], a * c1[1] + c2[1]))
    finally:
        icnf.close()
    rhs = float(a) * f64(p1[0]) + f64(p2[0])
    rhs_z = float(a) * f64(p1[1]) + f64(p2[1])
    _block_bar(p12[0], rhs, case.net, f"{name} linearity", 1e-4, p12[1], rhs_z)


def test_protocol_errors():
    """Pullback without a record, with another B, with no cotangent at all, on the other kind of record (both ways), and after
    another solve: CNFError(ERR_BAD_ARG)."""
    case = GT.GPU_CASES["generic-cfg2"]
    flat, xs, eps, _ = case.inputs()
    z0 = R.case_z0(case)
    B = case.B
    cl = np.full(B, 1.0 / B, np.float32)
    cot4 = np.zeros((4, B), np.float32)
    cot4[0] = 1.0 / B

    def refused(fn, *a, **kw):
        with pytest.raises(cnf.CNFError) as e:
            fn(*a, **kw)
        assert e.value.status == _lib.ERR_BAD_ARG, e.value

    icnf = _model(case, lam_of(case))
    try:
        refused(cnf.generate_pullback, icnf, (None, _dev(cl)))                    # no record at all
        _record(icnf, cnf.TrainMode(), flat, z0, eps, None)
        g0 = _pull(icnf, (None, cl))
        refused(cnf.generate_pullback, icnf, (None, _dev(cl[:B - 1])))            # another B
        refused(cnf.generate_pullback, icnf, (None, None))                        # no cotangent
        refused(cnf.inference_pullback, icnf, _dev(cot4))                         # a sampling record is not an inference record
        gx = torch.empty(B * case.nvars, dtype=torch.float32, device="cuda")      # ... and has no grad_x
        assert _lib.lib().cnf_grad_x(icnf.handle(), gx.data_ptr(), B, None) == _lib.ERR_BAD_ARG
        g1 = _pull(icnf, (None, cl))                                              # (the record survives refused calls)
        assert np.array_equal(g0[0], g1[0]) and np.array_equal(g0[1], g1[1])
        cnf.inference_record(icnf, cnf.TrainMode(), _dev(xs), flat, {}, eps=_dev(eps))
        refused(cnf.generate_pullback, icnf, (None, _dev(cl)))                    # ... and the reverse
        cnf.inference_pullback(icnf, _dev(cot4))
        _record(icnf, cnf.TrainMode(), flat, z0, eps, None)
        cnf.generate(icnf, cnf.TrainMode(), flat, {}, 7, z0=_dev(z0[:, :7]), eps=_dev(eps[:, :7]))
        refused(cnf.generate_pullback, icnf, (None, _dev(cl)))                    # displaced by another solve
    finally:
        icnf.close()


def _target(nvars, seed=31):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(nvars), rng.uniform(0.5, 2.0, nvars)


def test_reverse_kl_backward_is_the_pullback_of_its_cotangents():
    """``reverse_kl`` to a diagonal Gaussian target: value from the reference's outputs, ``.backward()`` against
    ``generate_pullback`` of the hand-formed cotangents (g_logq = 1/B, g_x = (xs - mu) / sigma^2 / B) and against the reference."""
    case = GT.GPU_CASES["adj3b-B33-fixed"]
    flat, _, eps, _ = case.inputs()
    z0 = R.case_z0(case)
    B = case.B
    mu, sig = _target(case.nvars)
    mu_d, sig_d = _dev(mu)[:, None], _dev(sig)[:, None]
    target = lambda x: -0.5 * (((x - mu_d) / sig_d) ** 2).sum(0)
    icnf = _model(case, lam_of(case))
    try:
        ps = _dev(flat).requires_grad_(True)
        out = cnf.reverse_kl(icnf, cnf.TrainMode(), ps, {}, B, target, z0=_dev(z0), eps=_dev(eps))
        assert out.dim() == 0
        steps = [abs(float(d)) for d in icnf.last_steps]
        xs = icnf._record["z"][:case.nvars].clone()
        out.backward()
        g = _np(ps.grad)
        cot = (_np((xs - mu_d) / sig_d ** 2 / B), np.full(B, 1.0 / B, np.float32))
        gp, _ = _pull(icnf, cot)
    finally:
        icnf.close()
    _block_bar(g, gp, case.net, "reverse_kl backward against generate_pullback", 1e-4)
    cfg = case.cfg(lam_of(case))
    z64, q64, _, _ = R.forward(cfg, f64(flat), f64(z0), f64(eps), steps)
    x64 = z64[:case.nvars]
    rval = float(np.mean(q64 + 0.5 * (((x64 - mu[:, None]) / sig[:, None]) ** 2).sum(0)))
    assert abs(float(out.detach()) - rval) <= 1e-5 * max(1.0, abs(rval)), (float(out.detach()), rval)
    c64 = ((x64 - mu[:, None]) / sig[:, None] ** 2 / B, np.full(B, 1.0 / B))
    r64 = R.vjp64(cfg, flat, z0, eps, c64[0], c64[1], steps)
    r32 = R.vjp32(cfg, flat, z0, eps, c64[0], c64[1], steps)
    V.assert_vjp(g, None, (r64[2], None), (r32[2], None), case.net, "autograd reverse_kl")


def test_gradient_reaches_z0_and_ys():
    """z0 = g(context) and ys = encoder(context): a loss on (xs, logq) back-propagates into both, at the bar."""
    case = GT.GPU_CASES["mfma-12x64x48-cond-jvp"]
    flat, _, eps, ys = case.inputs()
    z0 = R.case_z0(case)
    B, n_in = case.B, case.nvars + case.naugs
    rng = np.random.default_rng(41)
    wx, wq = (rng.standard_normal((case.nvars, B)) / B).astype(np.float32), (rng.standard_normal(B) / B).astype(np.float32)
    icnf = _model(case, lam_of(case))
    try:
        ps = _dev(flat).requires_grad_(True)
        zc = _dev(0.5 * z0).requires_grad_(True)
        yc = _dev(ys).requires_grad_(True)
        xs, logq = cnf.differentiable_generate(icnf, cnf.TrainMode(), ps, {}, B, ys=yc, z0=2.0 * zc, eps=_dev(eps))
        steps = [abs(float(d)) for d in icnf.last_steps]
        out = (_dev(wx) * xs).sum() + (_dev(wq) * logq).sum()
        g, gz, gy = torch.autograd.grad(out, (ps, zc, yc))
        g, gz, gy = _np(g), _np(gz), _np(gy)
    finally:
        icnf.close()
    assert gz.shape == (n_in, B) and gy.shape == ys.shape
    cfg = case.cfg(lam_of(case))
    r64 = R.vjp64(cfg, flat, z0, eps, wx, wq, steps, ys)
    r32 = R.vjp32(cfg, flat, z0, eps, wx, wq, steps, ys)
    V.assert_vjp(g, gz / 2.0, (r64[2], r64[3]), (r32[2], r32[3]), case.net, "autograd into ps and z0")
    CR.assert_ys(gy, r64[4], r32[4], "autograd into ys")


def test_displaced_record_gives_the_same_gradient_bit_for_bit():
    case = GT.GPU_CASES["adj3b-B33-fixed"]
    flat, _, eps, _ = case.inputs()
    z0 = R.case_z0(case)
    w = _dev(np.random.default_rng(4).uniform(0.5, 1.5, case.B))
    res = []
    icnf = _model(case, lam_of(case))
    try:
        for disturb in (False, True):
            ps = _dev(flat).requires_grad_(True)
            z = _dev(z0).requires_grad_(True)
            xs, logq = cnf.differentiable_generate(icnf, cnf.TrainMode(), ps, {}, case.B, z0=z, eps=_dev(eps))
            out = (w * (logq - 0.5 * (xs * xs).sum(0))).sum()
            if disturb:
                cnf.generate(icnf, cnf.TrainMode(), flat, {}, 7, z0=_dev(z0[:, :7]), eps=_dev(eps[:, :7]))
            g, gz = torch.autograd.grad(out, (ps, z))
            res.append((_np(xs), _np(logq), _np(g), _np(gz)))
    finally:
        icnf.close()
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
