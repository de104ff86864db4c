"""Differentiable inference on the device: ``inference_record`` / ``inference_pullback`` / ``differentiable_inference`` against
the float64 reference of tests/vjp_ref.py, on every pullback route.

Cases: ``grad_terms.GPU_CASES`` (one per route; the ``wave`` shapes exercise the hand-over to the recorded route) with
lam = (1, 1, 1) ((1, 1, 0) without augmented rows) so that every row exists, a TestMode leg (k_adj_test) and one full-covariance
``basedist``.  For each case the device's own steps are replayed and five cotangents are pulled back from ONE record: each
output row alone (N(0, 1)/B entries in that row) and all rows together.

Bar (tests/grad_terms.py's, unchanged): per parameter block and for grad_xs  max|got - ref64| <= rtol (max|ref64| + rms ref64),
rtol = max(1e-4, 8 floor) <= 1e-3, floor = the error of the float32 run of the same reference over that scale.
"""
import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from oracle import cnf_oracle as O
from tests import basedist_ref as BR
from tests import grad_terms as GT
from tests import helpers
from tests import vjp_ref as V
from tests.test_gpu_grad_terms import TWO_FORMS, _forced_split, _model
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = O.ACT_TANH
f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
_REF = {}                                   # (case, cotangent) -> (ref64, ref32): one reference for both launch forms


def _lam(case):
    return (1.0, 1.0, 1.0 if case.naugs else 0.0)


def _args(inputs):
    flat, xs, eps, ys = inputs
    return (_dev(ys), flat, {}) if ys is not None else (flat, {})


def _np(t):
    return t.detach().cpu().numpy()


def _record(icnf, inputs, mode=None):
    flat, xs, eps, ys = inputs
    mode = mode or cnf.TrainMode()
    train = isinstance(mode, cnf.TrainMode)
    logpx, regs = cnf.inference_record(icnf, mode, _dev(xs), *_args(inputs), eps=_dev(eps) if train else None)
    return _np(logpx), [_np(r) for r in regs], [float(d) for d in icnf.last_steps]


def _pull(icnf, cot):
    g, gx = cnf.inference_pullback(icnf, _dev(cot), with_x=True)
    return _np(g), _np(gx)


def _rows(case):
    return (0, 1, 2, 3) if case.naugs else (0, 1, 2)


def _reference(key, cfg, inputs, cot, dts, train=True, base=None):
    if key not in _REF:
        flat, xs, eps, ys = inputs
        _, g64, x64 = V.vjp64(cfg, flat, xs, eps, cot, dts, ys, train, base)
        _, g32, x32 = V.vjp32(cfg, flat, xs, eps, cot, dts, ys, train, base)
        _REF[key] = ((g64, x64), (g32, x32))
    return _REF[key]


MATRIX = [(c.name, s) for c in GT.GPU_CASES.values() if c.route != "contraction"
          for s in ((0, 1) if c.route in TWO_FORMS else (None,))]


@pytest.mark.parametrize("name,split", MATRIX, ids=[n if s is None else f"{n}-split{s}" for n, s in MATRIX])
def test_row_cotangents_against_the_reference(name, split):
    """Outputs of the recorded inference against ``inference``; five cotangents from one record against the reference."""
    case = GT.GPU_CASES[name]
    inputs = case.inputs()
    flat, xs, eps, ys = inputs
    cfg = case.cfg(_lam(case))
    with _forced_split(split):
        icnf = _model(case, _lam(case))
        try:
            lp0, regs0 = cnf.inference(icnf, cnf.TrainMode(), _dev(xs), *_args(inputs), eps=_dev(eps))
            lp0, regs0 = _np(lp0), [_np(r) for r in regs0]
            lp, regs, steps = _record(icnf, inputs)
            helpers.assert_parity(lp, lp0, f"{name}: logpx of inference_record against inference")
            for a, b, nm in zip(regs, regs0, "EnA"):
                helpers.assert_parity(a, b, f"{name}: {nm} of inference_record against inference")
            if case.steps[0] == "fixed":
                assert len(steps) == round(abs(case.tspan[1] - case.tspan[0]) / case.steps[1]), (name, steps)
            cots = V.row_cotangents(np.random.default_rng(case.seed + 7), case.B, _rows(case))
            got = {k: _pull(icnf, c) for k, c in cots.items()}            # five pullbacks, one record
        finally:
            icnf.close()
    dts = [abs(d) for d in steps]
    out64, _, _ = V.outputs(cfg, f64(flat), f64(xs), f64(eps), dts, f64(ys))
    helpers.assert_parity(lp, out64[0], f"{name}: logpx against the reference on the device's steps")
    for k, c in cots.items():
        r64, r32 = _reference((name, k, tuple(dts)), cfg, inputs, c, dts)
        V.assert_vjp(got[k][0], got[k][1], r64, r32, case.net, f"{name} split={split} cot={k}")


TEST_CASES = [((32, 128, 128, 32), 32, 0, 16, 0), ((12, 64, 48, 12), 8, 4, 24, 3)]


@pytest.mark.parametrize("dims,nvars,naugs,B,ncond", TEST_CASES, ids=["32x128x128x32-B16", "12x64x48x12-cond-B24"])
def test_testmode_pullback(dims, nvars, naugs, B, ncond):
    """k_adj_test with a per-sample cotangent of logpx; rows 1-3 do not exist in TestMode and their cotangents are ignored."""
    net = O.Net((dims[0] + ncond,) + dims[1:], (T, O.ACT_SOFTPLUS, T))
    cfg = O.Cfg(net, nvars, naugs, tspan=(0.0, 0.5))
    rng = np.random.default_rng(3)
    flat = O.glorot_params(net, rng, np.float32, 0.2)
    xs = rng.standard_normal((nvars, B)).astype(np.float32)
    ys = rng.standard_normal((ncond, B)).astype(np.float32) if ncond else None
    inputs = (flat, xs, None, ys)
    layers = [cnf.Dense(a, b, helpers.ACT_NAME[k]) for a, b, k in zip(net.dims[:-1], net.dims[1:], net.acts)]
    icnf = cnf.construct(cnf.CondRNODE if ncond else cnf.RNODE, cnf.Chain(*layers), nvars, naugs, tspan=(0.0, 0.5),
                         sol_kwargs=dict(adaptive=False, dt=0.25), rng=0)
    try:
        lp0, _ = cnf.inference(icnf, cnf.TestMode(), _dev(xs), *_args(inputs))
        lp, regs, steps = _record(icnf, inputs, cnf.TestMode())
        helpers.assert_parity(lp, _np(lp0), f"TestMode {dims}: logpx of inference_record against inference")
        assert len(steps) == 2
        cot = np.zeros((4, B), np.float32)
        cot[0] = (rng.standard_normal(B) / B).astype(np.float32)
        got = _pull(icnf, cot)
        junk = cot.copy()
        junk[1:] = 1.0                                   # (ignored rows)
        got2 = _pull(icnf, junk)
    finally:
        icnf.close()
    dts = [abs(d) for d in steps]
    r64, r32 = _reference(("test", dims), cfg, inputs, cot, dts, train=False)
    V.assert_vjp(got[0], got[1], r64, r32, net, f"TestMode {dims} cot=logpx")
    assert np.array_equal(got[0], got2[0]) and np.array_equal(got[1], got2[1])


def test_full_covariance_basedist():
    """A non-default base: the terminal cotangent goes through the precision factor; d logpdf / d z from basedist_ref.Gauss."""
    case = GT.Case("basedist-16x48", "adj_mfma", (16, 48, 16), (T,) * 2, 8, 8, 32, 1701, scale=0.3)
    inputs = case.inputs()
    flat, xs, eps, ys = inputs
    rng = np.random.default_rng(5)
    mean, cov = 0.3 * rng.standard_normal(16), BR.random_cov(rng, 16, "full")
    g = BR.Gauss(mean, cov)
    layers = [cnf.Dense(a, b, "tanh") for a, b in zip(case.dims[:-1], case.dims[1:])]
    icnf = cnf.construct(cnf.FFJORD, cnf.Chain(*layers), 8, 8, tspan=case.tspan, lambda1=1.0, lambda2=1.0, lambda3=1.0,
                         sol_kwargs=case.sol_kw, rng=0, basedist=cnf.MvNormal(mean, cov))
    try:
        lp, regs, steps = _record(icnf, inputs)
        cots = V.row_cotangents(np.random.default_rng(9), case.B, (0, 1, 2, 3))
        got = {k: _pull(icnf, c) for k, c in cots.items()}
    finally:
        icnf.close()
    cfg, dts = case.cfg((1.0, 1.0, 1.0)), [abs(d) for d in steps]
    out64, _, _ = V.outputs(cfg, f64(flat), f64(xs), f64(eps), dts, base=g)
    helpers.assert_parity(lp, out64[0], "basedist: logpx against the reference")
    for k, c in cots.items():
        r64, r32 = _reference(("basedist", k), cfg, inputs, c, dts, base=g)
        V.assert_vjp(got[k][0], got[k][1], r64, r32, case.net, f"basedist cot={k}")


def _block_bar(got, ref, net, what, rtol, gx=None, rgx=None):
    pairs = [(n, got[sl], ref[sl]) for n, sl in GT.param_blocks(net).items()]
    if gx is not None:
        pairs.append(("grad_x", gx, rgx))
    for n, a, b in pairs:
        s = V.scale(b)
        err = float(np.abs(f64(a) - f64(b)).max())
        assert np.isfinite(err) and err <= rtol * s, f"{what} {n}: off by {err / max(s, 1e-300):.3g} of its scale (rtol {rtol:g})"


IDENTITY = [(n, s) for n, s in MATRIX if "replay" not in n or "B77" in n or "B32" in n]


@pytest.mark.parametrize("name,split", IDENTITY, ids=[n if s is None else f"{n}-split{s}" for n, s in IDENTITY])
def test_loss_cotangent_is_loss_and_grad(name, split):
    """g = (-1/B, lam/B) against ``loss_and_grad`` of the same model, inputs and eps: rtol 1e-4 where both run the same pullback
    kernel, 2e-4 on the wave cases (loss_and_grad runs inside the launch of the solve there: the two sides' bars, added)."""
    case = GT.GPU_CASES[name]
    inputs = case.inputs()
    flat, xs, eps, ys = inputs
    lam = _lam(case)
    B = case.B
    cot = V.loss_cotangent(case.cfg(lam), B).astype(np.float32)
    with _forced_split(split):
        icnf = _model(case, lam)
        try:
            val, rg, rgx = cnf.loss_and_grad(icnf, cnf.TrainMode(), _dev(xs), *_args(inputs), eps=_dev(eps), with_x=True)
            rg, rgx, rsteps = _np(rg), _np(rgx), [float(d) for d in icnf.last_steps]
            _, _, steps = _record(icnf, inputs)
            g, gx = _pull(icnf, cot)
        finally:
            icnf.close()
    bitwise = np.array_equal(g, rg) and np.array_equal(gx, rgx)
    line = (f"vjp identity | {name} split={split}: same steps {steps == rsteps}, bitwise {bitwise}, "
            f"max |diff| {np.abs(g - rg).max():.3e} of {np.abs(rg).max():.3e}")
    helpers.note(line)
    print(line)
    if steps == rsteps:                     # one discrete map on both sides
        _block_bar(g, rg, case.net, f"{name} identity", 2e-4 if case.route == "wave" else 1e-4, gx, rgx)
        return
    # Adaptive stepping on a wave case: loss_and_grad's solve runs in k_solve_wave, the recorded one in the step kernels, and the two
    # controllers, fed rounding noise by the rows that start at 0, accept different steps -- two discrete maps, whose gradients
    # differ by the solver's tolerance and share no bar.  Then each side is held to the float64 reference on ITS OWN steps, at
    # that side's bar (1e-4 each, which is what the 2e-4 of the direct comparison adds up): no less than the comparison asks.
    assert case.route == "wave" and case.steps[0] == "adaptive", (name, steps, rsteps)
    cfg = case.cfg(lam)
    dts, rdts = [abs(d) for d in steps], [abs(d) for d in rsteps]
    r64, r32 = _reference((name, "loss", tuple(dts)), cfg, inputs, cot, dts)
    V.assert_vjp(g, gx, r64, r32, case.net, f"{name} identity, pullback on its own steps")
    _, og, ogx = GT.oracle_run(cfg, flat, xs, eps, ys, rdts)
    _block_bar(rg, og, case.net, f"{name} identity, loss_and_grad on its own steps", 1e-4, rgx, ogx)


@pytest.mark.parametrize("name", ["adj3b-B300-fixed", "mfma-cfg5-vjp"])
def test_samples_are_independent(name):
    """One-hot column cotangent: grad_xs exactly zero elsewhere; all-zero cotangent: gradient exactly zero.  B = 300 on k_adj3b
    and B = 40 on 128-384-128: the tile edges of both layouts."""
    case = GT.GPU_CASES[name]
    inputs = case.inputs()
    B = case.B
    for split in (0, 1):
        with _forced_split(split):
            icnf = _model(case, _lam(case))
            try:
                _record(icnf, inputs)
                for j in sorted({0, 5, 31, 32, B - 1}):
                    cot = np.zeros((4, B), np.float32)
                    cot[:, j] = [0.3, -0.2, 0.1, 0.05 if case.naugs else 0.0]
                    g, gx = _pull(icnf, cot)
                    assert np.isfinite(g).all() and np.abs(g).max() > 0 and np.abs(gx[:, j]).max() > 0, (name, j)
                    assert not np.delete(gx, j, axis=1).any(), (name, split, j, np.nonzero(np.abs(gx).sum(0))[0])
                g, gx = _pull(icnf, np.zeros((4, B), np.float32))
                assert not g.any() and not gx.any(), (name, split)
            finally:
                icnf.close()


@pytest.mark.parametrize("name", ["adj3b-B33-fixed", "mfma-cfg5-jvp", "generic-cfg2"])
def test_linearity_from_one_record(name):
    case = GT.GPU_CASES[name]
    inputs = case.inputs()
    rng = np.random.default_rng(11)
    g1 = (rng.standard_normal((4, case.B)) / case.B).astype(np.float32)
    g2 = (rng.standard_normal((4, case.B)) / case.B).astype(np.float32)
    a = np.float32(-1.75)
    icnf = _model(case, _lam(case))
    try:
        _record(icnf, inputs)
        p1, p2, p12 = _pull(icnf, g1), _pull(icnf, g2), _pull(icnf, a * g1 + g2)
    finally:
        icnf.close()
    rhs = float(a) * f64(p1[0]) + f64(p2[0])
    rhs_x = float(a) * f64(p1[1]) + f64(p2[1])
    _block_bar(p12[0], rhs, case.net, f"{name} linearity", 1e-4, p12[1], rhs_x)


def test_protocol_errors():
    """Pullback without a record, with another B, and after set_params / another inference: CNFError(ERR_BAD_ARG)."""
    case = GT.GPU_CASES["generic-cfg2"]
    inputs = case.inputs()
    flat, xs, eps, ys = inputs
    B = case.B
    cot = np.zeros((4, B), np.float32)
    cot[0] = 1.0 / B

    def refused(icnf, c):
        with pytest.raises(cnf.CNFError) as e:
            cnf.inference_pullback(icnf, _dev(c))
        assert e.value.status == _lib.ERR_BAD_ARG, e.value

    icnf = _model(case, _lam(case))
    try:
        refused(icnf, cot)                                   # no record at all
        _record(icnf, inputs)
        _pull(icnf, cot)
        refused(icnf, cot[:, :B - 1])                        # another B
        _pull(icnf, cot)                                     # (the record survives a refused call)
        cnf.inference(icnf, cnf.TrainMode(), _dev(xs), flat, {}, eps=_dev(eps))
        refused(icnf, cot)                                   # displaced by another solve
        _record(icnf, inputs)
        icnf.set_params(flat * np.float32(1.01))
        refused(icnf, cot)                                   # parameters uploaded
    finally:
        icnf.close()


def _autograd_case(name="adj3-30x120x116-aug"):
    case = GT.GPU_CASES[name]
    return case, case.inputs(), (0.01, 0.02, 0.03)


@pytest.mark.parametrize("which", ["weighted", "tempered"])
def test_autograd_of_the_ready_made_losses(which):
    """torch.autograd.grad of weighted_loss / tempered_loss w.r.t. ps and xs against the float64 reference, the cotangents
    computed in float64 from the reference's outputs."""
    case, inputs, lam = _autograd_case()
    flat, xs, _, _ = inputs
    B = case.B
    rng = np.random.default_rng(21)
    w = rng.uniform(0.0, 2.0, B)
    w[::2] = 0.0                                             # half of the samples carry no weight
    beta = 0.7
    fn = cnf.weighted_loss(w.astype(np.float32)) if which == "weighted" else cnf.tempered_loss(beta)
    icnf = _model(case, lam)
    try:
        ps = _dev(flat).requires_grad_(True)
        x = _dev(xs).requires_grad_(True)
        out = fn(icnf, cnf.TrainMode(), x, ps, {})
        assert out.dim() == 0
        eps = _np(icnf._record["eb"].view())                 # the probes the loss drew
        steps = [abs(float(d)) for d in icnf.last_steps]
        g, gx = torch.autograd.grad(out, (ps, x))
        g, gx, val = _np(g), _np(gx), float(out.detach())
    finally:
        icnf.close()
    cfg = case.cfg(lam)
    o64, _, _ = V.outputs(cfg, f64(flat), f64(xs), f64(eps), steps)
    l = np.array([lam[0], lam[1], lam[2]])
    if which == "weighted":
        rval = float(np.sum(w * (-o64[0] + l @ o64[1:])) / w.sum())
        cot = np.concatenate([[-w / w.sum()], np.outer(l, w / w.sum())])
    else:
        a = beta * o64[0]
        m = a.max()
        lse = m + np.log(np.exp(a - m).sum())
        rval = float(-(lse - np.log(B)) / beta + np.mean(l @ o64[1:]))
        cot = np.concatenate([[-np.exp(a - lse)], np.outer(l, np.full(B, 1.0 / B))])
    assert abs(val - rval) <= 1e-5 * max(1.0, abs(rval)), (which, val, rval)
    _, g64, x64 = V.vjp64(cfg, flat, xs, eps, cot, steps)
    _, g32, x32 = V.vjp32(cfg, flat, xs, eps, cot, steps)
    V.assert_vjp(g, gx, (g64, x64), (g32, x32), case.net, f"autograd {which}_loss")
    if which == "weighted":
        assert not gx[:, ::2].any(), "samples with weight 0 must have exactly zero grad_xs"


def test_displaced_record_gives_the_same_gradient_bit_for_bit():
    case, inputs, lam = _autograd_case("adj3b-B33-fixed")
    flat, xs, eps, _ = inputs
    w = _dev(np.random.default_rng(4).uniform(0.5, 1.5, case.B))
    res = []
    icnf = _model(case, lam)
    try:
        for disturb in (False, True):
            ps = _dev(flat).requires_grad_(True)
            x = _dev(xs).requires_grad_(True)
            logpx, (E, n, A) = cnf.differentiable_inference(icnf, cnf.TrainMode(), x, ps, {}, eps=_dev(eps))
            out = (w * (-logpx + 0.5 * E - 0.25 * n)).sum()
            if disturb:
                cnf.inference(icnf, cnf.TrainMode(), _dev(xs[:, :7]), flat, {}, eps=_dev(eps[:, :7]))
            g, gx = torch.autograd.grad(out, (ps, x))
            res.append((_np(logpx), _np(g), _np(gx)))
    finally:
        icnf.close()
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


def _front_end_model(seed=1, sol_kwargs=None):
    nn = cnf.Chain(cnf.Dense(1, 3, "tanh"), cnf.Dense(3, 1, "tanh"))
    e32 = float(np.finfo(np.float32).eps)
    return cnf.construct(cnf.RNODE, nn, 1, 0, compute_mode=cnf.HIPVecJacMatrixMode(), tspan=(0.0, 13.0), steer_rate=0.1,
                         lambda1=1e-2, lambda2=1e-2, lambda3=1e-2,
                         sol_kwargs=sol_kwargs or dict(reltol=float(np.sqrt(e32)), abstol=e32), rng=seed)


def _restated_loss(icnf, mode, xs, *args):
    """The built-in TrainMode loss, mean(-logpx + l1 E + l2 n + l3 A), through differentiable_inference."""
    logpx, (E, n, A) = cnf.differentiable_inference(icnf, mode, xs, *args)
    return (-logpx + icnf.lambda1 * E + icnf.lambda2 * n + icnf.lambda3 * A).mean()


def test_fit_one_iteration_of_a_restated_loss_is_loss_and_grad():
    """Two models with one rng seed: the custom path draws eps first and then the steered t1, as loss_and_grad does, so one
    seed gives one problem (equal steps); value within 1e-5 max(1, |value|), gradient at the bar (wave route on the other
    side: 2e-4).  The README network with steering, at a fixed dt: the steered t1 then fixes the step sequence (the last
    step ends at t1), so equal steps say that both sides drew the same t1 -- under adaptive stepping the two sides' forward
    kernels (k_solve_wave here, the recording step kernels there) accept different steps for one and the same problem."""
    r = np.random.default_rng(1).beta(2.0, 4.0, size=(32, 1)).astype(np.float32)
    xs = _dev(np.ascontiguousarray(r.T))
    kw = dict(adaptive=False, dt=0.5)
    a, b = _front_end_model(3, kw), _front_end_model(3, kw)
    try:
        flat = cnf.setup(5, a.nn)[0]
        val, g = cnf.loss_and_grad(a, cnf.TrainMode(), xs, _dev(flat), {})
        sa = [float(d) for d in a.last_steps]
        ps = _dev(flat).requires_grad_(True)
        out = _restated_loss(b, cnf.TrainMode(), xs, ps, {})
        sb = [float(d) for d in b.last_steps]
        gb, = torch.autograd.grad(out, ps)
    finally:
        a.close()
        b.close()
    assert sa == sb and len(sa) >= 24 and abs(sum(sa) - 13.0) > 1e-3, (sa, sb)       # (a steered span, the same on both sides)
    assert abs(float(out.detach()) - val) <= 1e-5 * max(1.0, abs(val)), (float(out.detach()), val)
    _block_bar(_np(gb), _np(g), O.Net((1, 3, 1), (T, T)), "fit iteration", 2e-4)


def test_fit_with_a_custom_loss_passes_the_front_end_assertions():
    icnf = _front_end_model(1)
    r = np.random.default_rng(1).beta(2.0, 4.0, size=(256, 1)).astype(np.float32)
    model = cnf.ICNFModel(icnf, _restated_loss, optimizers=(cnf.Lion(eta=1e-2),), n_epochs=12, batch_size=32)
    try:
        fitresult, cache, report = cnf.fit(model, 0, r)
    finally:
        icnf.close()
    losses = report["losses"]
    assert report["stats"]["iterations"] == 12 * 8 and cache is None and not report["stats"]["pipelined"]
    assert np.mean(losses[-8:]) < np.mean(losses[:8]) - 1.0
    assert np.mean(losses[-8:]) > -0.6


def test_fit_with_the_builtin_loss_is_still_pipelined():
    r = np.random.default_rng(1).beta(2.0, 4.0, size=(64, 1)).astype(np.float32)
    for loss in (None, cnf.loss):
        icnf = _front_end_model(1)
        try:
            _, _, report = cnf.fit(cnf.ICNFModel(icnf, loss, optimizers=(cnf.Lion(eta=1e-2),), n_epochs=1, batch_size=32), 0, r)
        finally:
            icnf.close()
        assert report["stats"]["pipelined"] and report["stats"]["iterations"] == 2, report["stats"]


def test_model_call_backpropagates_for_the_six_model_types():
    """The mirror of test/call_tests.jl:239-252 for a function other than ``loss``: icnf(xs, ps, st) with ps.requires_grad."""
    nvars, ndata = 2, 4
    rng = np.random.default_rng(2024)
    for mt in (cnf.RNODE, cnf.FFJORD, cnf.Planar, cnf.CondRNODE, cnf.CondFFJORD, cnf.CondPlanar):
        cond = mt in (cnf.CondRNODE, cnf.CondFFJORD, cnf.CondPlanar)
        planar = mt in (cnf.Planar, cnf.CondPlanar)
        for aug_steer in (False, True):
            naugs = nvars if aug_steer else 0
            n_in, n_cond = nvars + naugs, (nvars if cond else 0)
            if planar:
                chain = cnf.Chain(cnf.PlanarLayer(n_in, "tanh", n_cond=n_cond))
            else:
                dims = (n_in + n_cond, 3 * n_in, n_in)
                chain = cnf.Chain(*[cnf.Dense(i, o, "tanh") for i, o in zip(dims[:-1], dims[1:])])
            flat = cnf.setup(int(rng.integers(1 << 30)), chain)[0]
            lam = dict(lambda1=1e-2, lambda2=1e-2) if mt in (cnf.RNODE, cnf.CondRNODE) else {}
            icnf = cnf.construct(mt, chain, nvars, naugs, steer_rate=1e-1 if aug_steer else 0.0,
                                 lambda3=1e-2 if aug_steer else 0.0, sol_kwargs=dict(adaptive=False, dt=1 / 8), **lam)
            try:
                ps = _dev(flat).requires_grad_(True)
                x = _dev(rng.standard_normal((nvars, ndata))).requires_grad_(True)
                y = _dev(rng.standard_normal((nvars, ndata))) if cond else None
                out, st = icnf((x, y), ps, {}) if cond else icnf(x, ps, {})
                assert out.shape == (ndata,) and st == {}
                g, gx = torch.autograd.grad((out * out).sum(), (ps, x))
                assert g.shape == ps.shape and gx.shape == x.shape, (mt.__name__, g.shape, gx.shape)
                assert torch.isfinite(g).all() and torch.isfinite(gx).all() and g.abs().max() > 0, mt.__name__
            finally:
                icnf.close()
