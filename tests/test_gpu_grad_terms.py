"""Each regulariser term of the loss gradient, on every pullback route of the device, at the term's own scale.

``loss_and_grad`` with the one-hot lam = e_k against the float64 oracle at lam = e_k, per parameter block and for
d loss / d xs, with the bar of tests/grad_terms.py (rtol = max(1e-4, 8 x the float32 oracle's own error) <= 1e-3 of the
scale of the term's share g(e_k) - g(0)); lam = (1, 1, 1) once per case with the whole-gradient bar of the other gradient
tests; zero norms (eps = 0 in some columns, a zero last layer) on every route; and the routes that environment switches
select, each in a child process.  The cases are ``grad_terms.GPU_CASES`` (their float32 floors: tests/test_grad_terms_host.py).
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import grad_terms as GT
from tests import helpers
from tests.test_gpu_parity import _assert_grad, _dev        # the whole-gradient bar: imported, not restated

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WAVE_GRAD_ON = os.environ.get("CNF_WAVE_GRAD", "")[:1] != "0"        # (the child process of CNF_WAVE_GRAD=0 takes the streamed path)
TWO_FORMS = ("adj3b", "adj_mfma")                                       # routes with a one-launch and a two-launch form


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    for line in GT.summary_notes():
        helpers.note(line)
        print(line)
    helpers.note(f"grad term summary | wall time of tests/test_gpu_grad_terms.py: {time.time() - t0:.0f} s")


def _model(case, lam):
    """The device model of ``case`` with the lambdas ``lam`` (the construction of test_gpu_parity's ``_grad_case``)."""
    net = case.net
    layers = [cnf.Dense(a, b, helpers.ACT_NAME[k]) for a, b, k in zip(net.dims[:-1], net.dims[1:], net.acts)]
    cm = cnf.HIPJacVecMatrixMode(case.kernel) if case.jvp else cnf.HIPVecJacMatrixMode(case.kernel)
    return cnf.construct(cnf.CondRNODE if case.n_cond else cnf.FFJORD, cnf.Chain(*layers), case.nvars, case.naugs, compute_mode=cm,
                         tspan=case.tspan, lambda1=lam[0], lambda2=lam[1], lambda3=lam[2] if case.naugs else 0.0,
                         sol_kwargs=case.sol_kw, rng=0)


def _device(icnf, inputs):
    flat, xs, eps, ys = inputs
    args = (_dev(ys), flat, {}) if ys is not None else (flat, {})
    val, grad, gx = cnf.loss_and_grad(icnf, cnf.TrainMode(), _dev(xs), *args, eps=_dev(eps), with_x=True)
    return val, grad.cpu().numpy(), gx.cpu().numpy(), dict(icnf.last_stats), [float(d) for d in icnf.last_steps]


def _check_route(case, icnf, st, what):
    """The kernel family the case is in the matrix for did take it, as far as the statistics of the call tell."""
    B = case.B
    if case.route == "wave":            # solve, loss and adjoint in one launch (+ the sum of the waves' partials)
        if WAVE_GRAD_ON:
            assert st["launches"] <= 2, (what, st)
    elif case.route == "generic":
        assert st["kernel_used"] == _lib.KERNEL_GENERIC and st["launches"] > 2, (what, st)
    else:
        assert _lib.lib().cnf_kernel_for(icnf.handle(), _lib.MODE_TRAIN, B) == _lib.KERNEL_MFMA, what
        assert st["kernel_used"] == _lib.KERNEL_MFMA, (what, st)


def _ora_kw(case, steps):
    """Fixed dt: the oracle takes its own steps (and the device must have taken as many); adaptive: the device's steps replayed."""
    if case.steps[0] == "fixed":
        n = round(abs(case.tspan[1] - case.tspan[0]) / case.steps[1])
        assert len(steps) == n, (case.name, steps)
        return case.sol_kw
    assert len(steps) >= 2, (case.name, steps)
    return dict(dts=steps)


def _loss_ok(val, rval, what):
    assert abs(val - rval) <= 1e-5 * max(1.0, abs(rval)), (what, val, rval)


def _check_terms(case, what):
    """Every term of ``case`` at lam = e_k with the term's bar, then lam = (1, 1, 1) with the whole-gradient bar."""
    inputs = case.inputs()
    for k in case.terms + (None,):
        lam = (1.0, 1.0, 1.0) if k is None else GT.one_hot(k)
        icnf = _model(case, lam)
        try:
            val, grad, gx, st, steps = _device(icnf, inputs)
            _check_route(case, icnf, st, what)
        finally:
            icnf.close()
        assert np.isfinite(grad).all() and np.isfinite(gx).all(), (what, k)
        if k is None:
            dts = GT.resolve_steps(case.cfg(lam), *inputs, _ora_kw(case, steps))
            rval, rgrad, rgx = GT.oracle_run(case.cfg(lam), *inputs, dts)
            _loss_ok(val, rval, what)
            _assert_grad(grad, rgrad, f"{what} lam = (1, 1, 1)")
            _assert_grad(gx, rgx, f"{what} lam = (1, 1, 1), d loss / d xs", rtol=2e-4)
        else:
            ref = GT.term_reference(case.cfg(lam), *inputs, k, _ora_kw(case, steps))
            _loss_ok(val, ref.ref[0], what)
            GT.assert_grad_term(grad, gx, ref, what, route=case.route + ("-jvp" if case.jvp else ""))


def _forced_split(split):
    """Context: ``cnf_set_grad_split(split)`` for the block, restored afterwards (None: left alone)."""
    import contextlib

    @contextlib.contextmanager
    def cm():
        if split is None:
            yield
            return
        l = _lib.lib()
        was = l.cnf_set_grad_split(-1)
        try:
            l.cnf_set_grad_split(split)
            yield
        finally:
            l.cnf_set_grad_split(was)
    return cm()


MATRIX = [(c.name, s) for c in GT.GPU_CASES.values() if c.route != "contraction"
          for s in ((0, 1) if c.route in TWO_FORMS else (None,))]


@pytest.mark.parametrize("name,split", MATRIX, ids=[n if s is None else f"{n}-split{s}" for n, s in MATRIX])
def test_grad_terms(name, split):
    """One case of the matrix: lam1, lam2 (and lam3 with augmentation) one at a time, then all three."""
    case = GT.GPU_CASES[name]
    what = name if split is None else f"{name} split={split}"
    with _forced_split(split):
        _check_terms(case, what)


def test_contraction_terms_after_a_larger_batch():
    """The weight-gradient contraction reads whole 32-row chunks of the factor rows: after a larger call on the same handle
    (B = 1100, data three times as large) the ragged batches 17, 70, 333 (K = 6 x 5 x B) must not see what it left -- per term."""
    cases = [c for c in GT.GPU_CASES.values() if c.route == "contraction"]
    big = GT.Case("contraction-big", "contraction", cases[0].dims, cases[0].acts, cases[0].nvars, 0, 1100, 1699,
                  steps=cases[0].steps, xs_scale=3.0)
    for k in cases[0].terms:
        icnf = _model(big, GT.one_hot(k))            # (one handle per term: the lambdas belong to the handle)
        try:
            flat_big, xs, eps, _ = big.inputs()
            cnf.loss_and_grad(icnf, cnf.TrainMode(), _dev(xs), flat_big, {}, eps=_dev(eps))
            for case in cases:
                inputs = case.inputs()
                val, grad, gx, st, steps = _device(icnf, inputs)
                _check_route(case, icnf, st, case.name)
                ref = GT.term_reference(case.cfg(GT.one_hot(k)), *inputs, k, _ora_kw(case, steps))
                _loss_ok(val, ref.ref[0], case.name)
                GT.assert_grad_term(grad, gx, ref, case.name, route="contraction")
        finally:
            icnf.close()


DEGENERATE_ON = [("wave-16x48-B32-replay", None), ("wave-16x48-B32-jvp", None), ("wave-6x18-B40-cond", None),
                 ("adj3b-B33-fixed", 0), ("adj3b-B33-fixed", 1), ("adj3b-B77-replay", 1), ("adj3-softplus-sigmoid", None),
                 ("adj3-30x120x116-aug", None), ("mfma-12x64x48-cond-vjp", 0), ("mfma-12x64x48-cond-vjp", 1),
                 ("mfma-12x64x48-cond-jvp", 0), ("mfma-12x64x48-cond-jvp", 1), ("mfma-cfg5-vjp", 1), ("mfma-cfg5-jvp", 1),
                 ("generic-cfg2", None), ("generic-cfg3", None)]


@pytest.mark.parametrize("which", GT.DEGENERATE)
@pytest.mark.parametrize("name,split", DEGENERATE_ON, ids=[n if s is None else f"{n}-split{s}" for n, s in DEGENERATE_ON])
def test_degenerate_inputs(name, split, which):
    """Zero norms at lam = (1, 1, 1): eps = 0 in a few columns of a tile (|eps' J| or |J eps| = 0 there only), and a zero last
    layer (zdot = 0, the augmented rows stay 0: |zdot|, |eps' J| and |z_aug| are 0 at every stage).  The unit vector of a zero
    vector is 0 (the oracle's convention and the kernels'): finite, and the whole-gradient bar against the oracle."""
    case = GT.GPU_CASES[name]
    what = f"{name} {which}" + ("" if split is None else f" split={split}")
    inputs = GT.degenerate_inputs(case, which)
    lam = (1.0, 1.0, 1.0)
    with _forced_split(split):
        icnf = _model(case, lam)
        try:
            val, grad, gx, st, steps = _device(icnf, inputs)
            _check_route(case, icnf, st, what)
        finally:
            icnf.close()
    assert np.isfinite(val) and np.isfinite(grad).all() and np.isfinite(gx).all(), what
    ora_kw = case.sol_kw if case.steps[0] == "fixed" else dict(dts=steps)
    dts = GT.resolve_steps(case.cfg(lam), *inputs, ora_kw)
    assert len(dts) == len(steps), (what, dts, steps)
    rval, rgrad, rgx = GT.oracle_run(case.cfg(lam), *inputs, dts)
    print(f"{what}: max |err| {np.abs(grad - rgrad).max():.3e} of max |ref| {np.abs(rgrad).max():.3e}; "
          f"d loss / d xs {np.abs(gx - rgx).max():.3e} of {np.abs(rgx).max():.3e}")
    _loss_ok(val, rval, what)
    _assert_grad(grad, rgrad, what)
    _assert_grad(gx, rgx, what + ", d loss / d xs", rtol=2e-4)
    if which == "zero-eps-columns":         # the zeroed samples on their own, at the scale of their own columns
        cols = [c for c in (0, 5, case.B - 1) if c < case.B]
        _assert_grad(gx[:, cols], rgx[:, cols], what + ", d loss / d xs of the zero-eps columns", rtol=2e-4)


SWITCHES = (
    ("CNF_WAVE_GRAD=0", "test_grad_terms and wave"),                                  # the streamed gradient path for the small networks
    ("CNF_WAVE_RICH=0", "(test_grad_terms or test_degenerate_inputs) and wave and not jvp"),   # the wave kernel recomputes its forward half
    ("CNF_ADJ3B=0", "(test_grad_terms or test_degenerate_inputs) and adj3b and split0"),       # k_adj3 on the headline shape
    ("CNF_ADJ_GENERIC=1", "(test_grad_terms or test_degenerate_inputs) and adj3-"),          # k_adj_mfma on the shapes k_adj3 takes
    ("CNF_WGRAD_LDS=1", "test_contraction or (test_grad_terms and (adj3b-B300-fixed-split0 or mfma-cfg5-vjp-split0))"),   # k_wgrad_mfma_b
    ("CNF_WGRAD_FP32=1", "test_contraction or (test_grad_terms and (adj3b-B300-fixed-split0 or mfma-cfg5-vjp-split0))"),
    ("CNF_WGRAD_KS=3", "test_contraction or (test_grad_terms and (adj3b-B300-fixed-split0 or mfma-cfg5-vjp-split0))"),   # a forced K-split
    ("CNF_STEP_FP32=1", "test_grad_terms and (adj3b-B77 or mfma-headline-jvp) and split1"),   # the fp32-MFMA step kernels record the forward
)


def test_switched_routes_in_child_processes(tmp_path):
    """The routes that environment switches select (read once per process): a selection of this file in a fresh child
    process per switch, one child at a time; the first failing child ends the test.  The children read the references this
    process has computed (CNF_GRAD_TERMS_CACHE)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cache = str(tmp_path / "refs")
    GT.save_cache(cache)
    for var, sel in SWITCHES:
        name, _, val = var.partition("=")
        env = dict(os.environ, **{name: val, "CNF_NO_PARITY_REPORT": "1", "CNF_GRAD_TERMS_CACHE": cache})
        t0 = time.time()
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                            "-k", sel], env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (var, r.stdout[-3000:], r.stderr[-1000:])
        assert " passed" in r.stdout and "failed" not in r.stdout, (var, r.stdout[-500:])
        lines = r.stdout.strip().splitlines()
        helpers.note(f"grad terms under {var}: {lines[-1].strip()} ({time.time() - t0:.0f} s)")
        for line in lines:                      # the child's own table of measured errors
            if "grad term summary |" in line and "wall time" not in line:      # (-s: the first one follows the progress dots)
                helpers.note(f"{var} | {line[line.index('grad term summary |'):]}")
