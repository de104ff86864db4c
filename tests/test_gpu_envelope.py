"""The accepted network envelope on the device (the table and the tolerance rule: tests/envelope.py; floors: tests/test_envelope_host.py).

Per case: the RHS in TrainMode (the case's compute mode) and TestMode, a fixed-step inference in both modes, and the loss
gradient with the data gradient, with ``kernel = auto`` and ``kernel = generic``, each against the float64 oracle at the
case's own rtol = max(1e-4, 8 x float32 floor) <= 1e-3; what is observable about the route (``cnf_kernel_for``,
``last_stats``); the support contract (``kernel = mfma`` refused loudly where there is no such kernel, no HIP error on
anything ``construct`` accepted); and ``CNF_ERR_NONFINITE`` on every solve driver for a NaN / an Inf in one data column.
"""
import time

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from oracle import cnf_oracle as O
from tests import envelope as E
from tests import helpers
from tests.helpers import assert_parity
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORST = {}          # family -> (err_over_bar, what)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    for fam, (e, what) in sorted(WORST.items()):
        line = f"envelope summary | family ({fam}): worst err_over_bar {e:.3f} ({what})"
        helpers.note(line)
        print(line)
    helpers.note(f"envelope summary | wall time of tests/test_gpu_envelope.py: {time.time() - t0:.0f} s")


def _file(case, e, what):
    if e > WORST.get(case.family, (-1.0, ""))[0]:
        WORST[case.family] = (e, what)


def _parity(case, got, ref, what, rtol, trace_row=None):
    e = assert_parity(got, ref, f"envelope {case.name} {what}", rtol=rtol, trace_row=trace_row)
    _file(case, e, f"{case.name} {what}")
    return e


def _grad_parity(case, got, ref, what, rtol):
    """The whole-gradient bar max|err| <= rtol (max|ref| + rms ref), filed like a parity comparison."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(ref), (what, got.shape, np.shape(ref))
    assert np.isfinite(got).all(), f"{case.name} {what}: non-finite gradient"
    e = E.grad_err(got, ref) / rtol
    helpers.REPORT.append({"what": f"envelope {case.name} {what}", "shape": list(got.shape), "rtol": rtol, "err_over_bar": e,
                           "max_abs_err": float(np.abs(got - ref).max()), "max_rel_err": e * rtol, "mean_rel_err": e * rtol})
    _file(case, e, f"{case.name} {what}")
    assert e <= 1.0, f"{case.name} {what}: gradient error {e:.3f} x the bar (rtol {rtol:g})"


def _nn(icnf, ys):
    return cnf.CondLayer(icnf.nn, _dev(ys)) if ys is not None else icnf.nn


def _args(ys, flat):
    return (_dev(ys), flat, {}) if ys is not None else (flat, {})


KERNEL_ID = {"generic": _lib.KERNEL_GENERIC, "mfma-lds": _lib.KERNEL_MFMA, "mfma-streamed": _lib.KERNEL_MFMA,
             "jvp-mfma": _lib.KERNEL_MFMA, "trace-mfma": _lib.KERNEL_MFMA}


def _forward(case, kernel):
    """RHS (TrainMode, TestMode) and fixed-step inference (both modes) of ``case`` with ``kernel``, each against the oracle."""
    flat, xs, eps, ys, u = case.inputs()
    n_in = case.nvars + case.naugs
    ref, rt = E.references(case.name), E.rtols(case.name)
    icnf = E.model(case, kernel)
    out = {}
    try:
        h, l = icnf.handle(), _lib.lib()
        if kernel == "auto":            # the restated dispatch is the library's
            assert l.cnf_kernel_for(h, _lib.MODE_TRAIN, case.B) == KERNEL_ID[case.route], (case.name, case.route)
            assert l.cnf_kernel_for(h, _lib.MODE_TEST, case.B) == KERNEL_ID[case.route_test], (case.name, case.route_test)
        du = cnf.augmented_f(_dev(u), flat, 0.0, icnf, cnf.TrainMode(), _nn(icnf, ys), {}, _dev(eps)).cpu().numpy()
        _parity(case, du, ref["du_train"], f"rhs train {kernel}", rt["du_train"], trace_row=n_in)
        out["du_train"] = du
        if case.test_solve:
            dt = cnf.augmented_f(_dev(u[:n_in + 1]), flat, 0.0, icnf, cnf.TestMode(), _nn(icnf, ys), {}, None).cpu().numpy()
            _parity(case, dt, ref["du_test"], f"rhs test {kernel}", rt["du_test"], trace_row=n_in)
            out["du_test"] = dt
        logpx, regs = cnf.inference(icnf, cnf.TrainMode(), _dev(xs), *_args(ys, flat), eps=_dev(eps))
        st = dict(icnf.last_stats)
        assert st["naccept"] == case.steps and st["nreject"] == 0 and st["nf"] == 1 + 6 * case.steps, (case.name, kernel, st)
        out["logpx"], out["regs"] = logpx.cpu().numpy(), np.stack([r.cpu().numpy() for r in regs])
        _parity(case, out["logpx"], ref["logpx"], f"logpx {kernel}", rt["logpx"])
        _parity(case, out["regs"], ref["regs"], f"regs {kernel}", rt["regs"])
        if kernel == "auto":
            assert st["kernel_used"] == KERNEL_ID[case.route], (case.name, st)
            if case.one_launch is not None:
                assert (st["launches"] <= 3) == case.one_launch, (case.name, st)
        else:
            assert st["kernel_used"] == _lib.KERNEL_GENERIC and st["launches"] > 3, (case.name, st)
        if case.test_solve:
            lpt, _ = cnf.inference(icnf, cnf.TestMode(), _dev(xs), *_args(ys, flat))
            st = dict(icnf.last_stats)
            assert st["naccept"] == case.steps, (case.name, kernel, st)
            assert st["kernel_used"] == (KERNEL_ID[case.route_test] if kernel == "auto" else _lib.KERNEL_GENERIC), (case.name, kernel, st)
            out["logpx_test"] = lpt.cpu().numpy()
            _parity(case, out["logpx_test"], ref["logpx_test"], f"logpx test {kernel}", rt["logpx_test"])
    finally:
        icnf.close()
    return out


def _gradient(case, kernel):
    flat, xs, eps, ys, u = case.inputs()
    ref, rt = E.references(case.name), E.rtols(case.name)
    icnf = E.model(case, kernel)
    try:
        val, grad, gx = cnf.loss_and_grad(icnf, cnf.TrainMode(), _dev(xs), *_args(ys, flat), eps=_dev(eps), with_x=True)
        steps = [abs(float(d)) for d in icnf.last_steps]
        assert np.allclose(steps, [case.dt] * case.steps, rtol=1e-6, atol=0), (case.name, steps)     # the oracle replays these
        assert abs(val - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"])), (case.name, kernel, val, ref["loss"])
        _grad_parity(case, grad.cpu().numpy(), ref["grad"], f"grad {kernel}", rt["grad"])
        _grad_parity(case, gx.cpu().numpy(), ref["grad_x"], f"grad_x {kernel}", rt["grad_x"])
        if case.test_grad and kernel == "auto":
            val, grad, gx = cnf.loss_and_grad(icnf, cnf.TestMode(), _dev(xs), *_args(ys, flat), with_x=True)
            assert len(icnf.last_steps) == case.steps
            assert abs(val - ref["loss_test"]) <= 1e-5 * max(1.0, abs(ref["loss_test"])), (case.name, val, ref["loss_test"])
            _grad_parity(case, grad.cpu().numpy(), ref["grad_test"], "grad test", rt["grad_test"])
            _grad_parity(case, gx.cpu().numpy(), ref["grad_x_test"], "grad_x test", rt["grad_x_test"])
    finally:
        icnf.close()


def _refused(case, mode, ys, flat, u, eps):
    """``kernel = mfma`` where the dispatch has no such kernel: CNF_ERR_UNSUPPORTED with a message, from the RHS and the solve."""
    n_in = case.nvars + case.naugs
    icnf = E.model(case, "mfma")
    try:
        train = mode.cnf == _lib.MODE_TRAIN
        with pytest.raises(cnf.CNFError) as e:
            cnf.augmented_f(_dev(u if train else u[:n_in + 1]), flat, 0.0, icnf, mode, _nn(icnf, ys), {}, _dev(eps) if train else None)
        assert e.value.status == _lib.ERR_UNSUPPORTED and "no kernel" in str(e.value), (case.name, str(e.value))
        with pytest.raises(cnf.CNFError) as e:
            cnf.inference(icnf, mode, _dev(case.inputs()[1]), *_args(ys, flat), eps=_dev(eps) if train else None)
        assert e.value.status == _lib.ERR_UNSUPPORTED and "no kernel" in str(e.value), (case.name, str(e.value))
    finally:
        icnf.close()


@pytest.mark.parametrize("name", list(E.CASES))
def test_envelope_case(name):
    """One case of the table.  A ``CNFError`` with a HIP status anywhere in here is a bug: ``construct`` accepted the shape."""
    case = E.CASES[name]
    flat, xs, eps, ys, u = case.inputs()
    rt = E.rtols(name)
    auto = _forward(case, "auto")
    gen = _forward(case, "generic")
    # auto and generic against each other where auto is another kernel (both met their bar against the oracle, so this one
    # cannot be tighter than twice that bar: it files the direct difference)
    n_in = case.nvars + case.naugs
    for k, row in (("du_train", n_in), ("du_test", n_in), ("logpx", None), ("regs", None), ("logpx_test", None)):
        routed = case.route_test if "test" in k else case.route
        if k in auto and routed != "generic":
            _parity(case, auto[k], gen[k].astype(np.float64), f"{k} auto vs generic", 2 * rt[k], trace_row=row)
    if case.grad:
        _gradient(case, "auto")
        _gradient(case, "generic")
    else:
        # beyond grad_supported the library refuses the gradient; RHS and inference above are unaffected
        assert not E.grad_supported(case.dims, case.n_cond), name
        icnf = E.model(case, "auto")
        try:
            with pytest.raises(cnf.CNFError) as e:
                cnf.loss_and_grad(icnf, cnf.TrainMode(), _dev(xs), *_args(ys, flat), eps=_dev(eps))
            assert e.value.status == _lib.ERR_UNSUPPORTED and "too wide" in str(e.value), str(e.value)
        finally:
            icnf.close()
    if case.route == "generic":
        _refused(case, cnf.TrainMode(), ys, flat, u, eps)
    if case.route_test == "generic" and case.test_solve:
        _refused(case, cnf.TestMode(), ys, flat, u, eps)


# ---------------------------------------------------------------------------------------
# non-finite data
# ---------------------------------------------------------------------------------------
T = O.ACT_TANH
# driver -> (dims, nvars, naugs, jvp, kernel, call, expectation of a clean solve: launches <= 3).  Every kernel loop these reach
# ends on StepState::nonfinite (ctrl_after_step sets done) and is bounded by maxiters: the host drivers count their launches
# against opts->maxiters (cnf_abi.hip), the one-launch kernels loop `it < sv.maxiters` (cnf_step3.hip, cnf_wave.hip,
# cnf_bcast.hip, cnf_trace.hip).  The record-* drivers other than record-wave are named for the forward solve the shape and
# kernel select in loss_and_grad; last_stats counts that solve's and the pullback's launches together and the suite has no
# threshold on it for them, so only their status and numbers are asserted.
DRIVERS = {
    "generic-steps": ((32, 128, 128, 32), 32, 0, False, "generic", "train", False),
    "mfma-steps-lds": ((32, 128, 112, 32), 32, 0, False, "auto", "train", False),
    "mfma-steps-streamed": ((32, 144, 144, 32), 32, 0, False, "auto", "train", False),
    "jvp-mfma-steps": ((32, 576, 576, 32), 32, 0, True, "auto", "train", False),
    "one-launch-vjp": ((32, 128, 128, 32), 32, 0, False, "auto", "train", True),
    "one-launch-jvp": ((32, 128, 128, 32), 32, 0, True, "auto", "train", True),
    "wave": ((16, 48, 16), 8, 8, False, "auto", "train", True),
    "bcast": ((128, 384, 128), 64, 64, False, "auto", "train", True),
    "trace-solve": ((32, 128, 128, 32), 32, 0, False, "auto", "test", True),
    "trace-steps": ((32, 128, 112, 32), 32, 0, False, "auto", "test", False),
    "generic-test-steps": ((32, 128, 112, 32), 32, 0, False, "generic", "test", False),
    "record-one-launch": ((32, 128, 128, 32), 32, 0, False, "auto", "grad", None),
    "record-one-launch-jvp": ((32, 128, 128, 32), 32, 0, True, "auto", "grad", None),
    "record-wave": ((16, 48, 16), 8, 8, False, "auto", "grad", None),
    "record-mfma-steps": ((32, 128, 112, 32), 32, 0, False, "auto", "grad", None),
    "record-bcast": ((128, 384, 128), 64, 64, False, "auto", "grad", None),
    "record-generic": ((32, 128, 112, 32), 32, 0, False, "generic", "grad", None),
    "record-test": ((32, 128, 112, 32), 32, 0, False, "auto", "grad-test", None),
    "submitted-one-launch": ((32, 128, 128, 32), 32, 0, False, "auto", "submit", None),
    "submitted-wave": ((16, 48, 16), 8, 8, False, "auto", "submit", None),
}
NF_B = 100          # column 70: the third 32-sample tile, the fifth 16-sample tile, the ninth 8-sample tile
NF_COL = 70


def _nf_model(dims, nvars, naugs, jvp, kernel, sol_kw):
    cfg = O.Cfg(O.Net(dims, (T,) * (len(dims) - 1)), nvars, naugs, 1e-2, 1e-2, 1e-2 if naugs else 0.0, use_jvp=jvp, tspan=(0.0, 1.0))
    return cfg, helpers.make_icnf(cnf, cfg, jvp=jvp, kernel=kernel, sol_kwargs=sol_kw, tag=cnf.RNODE)


def _nf_call(icnf, call, xs, flat, eps):
    """Runs ``call`` and returns (logpx or loss value ...); raises CNFError as the library reports it."""
    if call == "train":
        return cnf.inference(icnf, cnf.TrainMode(), _dev(xs), flat, {}, eps=_dev(eps))[0].cpu().numpy()
    if call == "test":
        return cnf.inference(icnf, cnf.TestMode(), _dev(xs), flat, {})[0].cpu().numpy()
    if call == "grad":
        return cnf.loss_and_grad(icnf, cnf.TrainMode(), _dev(xs), flat, {}, eps=_dev(eps))[1].cpu().numpy()
    if call == "grad-test":
        return cnf.loss_and_grad(icnf, cnf.TestMode(), _dev(xs), flat, {})[1].cpu().numpy()
    assert call == "submit"
    try:
        logpx, _ = cnf.inference_submit(icnf, cnf.TrainMode(), _dev(xs), flat, {}, eps=_dev(eps))
    except cnf.CNFError as e:           # a submitted solve reports at its collect: the submission itself must go through
        raise AssertionError(f"inference_submit raised: {e}") from e
    cnf.inference_collect(icnf)
    return logpx.cpu().numpy()


@pytest.mark.parametrize("stepping", ["fixed", "adaptive"])
@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("driver", list(DRIVERS))
def test_nonfinite_data_is_reported_by_every_solve_driver(driver, bad, stepping):
    """A NaN / an Inf in one entry of column 70 of 100 (not in the first tile of any kernel): the call reports
    CNF_ERR_NONFINITE -- not OK, not CNF_ERR_MAXITERS -- and the same handle then solves the clean batch as a fresh one does
    (fixed steps: to the usual parity with the float64 oracle as well).  With fixed steps only the non-finite count of the
    state can see it (an Inf leaves every derivative finite: tanh saturates); with the controller on, a NaN reaches the
    error norm too.  maxiters is small: the status must not depend on running out of it."""
    dims, nvars, naugs, jvp, kernel, call, one = DRIVERS[driver]
    sol_kw = dict(adaptive=False, dt=0.25, maxiters=12) if stepping == "fixed" else dict(maxiters=40)
    cfg, icnf = _nf_model(dims, nvars, naugs, jvp, kernel, sol_kw)
    rng = np.random.default_rng(2900 + len(driver))
    flat = O.glorot_params(cfg.net, rng, np.float32, 0.1)
    xs = rng.standard_normal((nvars, NF_B)).astype(np.float32)
    eps = rng.standard_normal((cfg.n_in, NF_B)).astype(np.float32)
    poisoned = xs.copy()
    poisoned[min(3, nvars - 1), NF_COL] = np.nan if bad == "nan" else np.inf
    what = f"{driver} {bad} {stepping}"
    try:
        clean0 = _nf_call(icnf, call, xs, flat, eps)                      # the driver the case is named for does take it
        st = dict(icnf.last_stats)
        if one is not None:
            assert (st["launches"] <= 3) == one, (what, st)
        if driver == "record-wave":     # solve, loss and adjoint in the wave kernel's launch (+ the sum of the partials), as
            assert st["launches"] <= 2, (what, st)          # tests/test_gpu_grad_terms.py reads it
        if driver.startswith("submitted"):
            assert st["launches"] <= 3, (what, st)          # (the one-launch forms are the ones that can be submitted)
        with pytest.raises(cnf.CNFError) as e:
            _nf_call(icnf, call, poisoned, flat, eps)
        assert e.value.status == _lib.ERR_NONFINITE, (what, str(e.value))
        clean1 = _nf_call(icnf, call, xs, flat, eps)                      # the handle is usable, and nothing of the bad call is left
        assert np.isfinite(clean1).all() and np.array_equal(clean0, clean1), what
        if stepping == "fixed" and call in ("train", "test", "submit"):
            f64 = lambda a: a.astype(np.float64)
            train = call != "test"
            _, ref_lp, _, _ = O.inference(cfg, f64(flat), f64(xs), f64(eps) if train else None, train, dt=0.25, adaptive=False)
            assert_parity(clean1, ref_lp, f"envelope nonfinite {what}: clean batch afterwards")
    finally:
        icnf.close()
