"""tests/cond_grad_ref.py, the reference of the gradient w.r.t. the conditioning inputs ``ys``, pinned without a device, and the
presence of the feature (header, built library, bindings, Python signatures).

On the four conditional cases of tests/grad_terms.py, TrainMode (VJP and JVP compute modes) and TestMode:

1. identity: ``grad`` and ``grad_x`` of ``vjp_ys64`` equal ``vjp_ref.vjp64``'s to 1e-13 of their scale (the restated pullbacks
   do the same arithmetic in the same order: the difference is expected to be exactly 0);
2. central differences in float64, step 1e-6, of sum(cot * outputs) w.r.t. single entries ys[k, b]: within 1e-7 of the scale
   of grad_ys (truncation is O(h^2) ~ 1e-12 relative, rounding of the quotient ~ 1e-16 / 1e-6 = 1e-10 of the outputs' scale;
   a missing stage or a wrong row is of order 1);
3. a cotangent that is non-zero in one sample only leaves every other column of grad_ys EXACTLY zero;
4. the float32 run of the reference stays within the bar's cap on grad_ys (8 x floor <= 1e-3) and the scale is positive.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import cond_grad_ref as R
from tests import vjp_ref as V
from tests.grad_terms import GPU_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = (0.01, 0.02, 0.03)
# (case, train): the JVP compute mode does not exist in TestMode, so its case runs in TrainMode only
COMBOS = [(n, True) for n in R.COND_CASES] + [(n, False) for n in R.COND_CASES if not GPU_CASES[n].jvp]
IDS = [f"{n}-{'train' if t else 'test'}" for n, t in COMBOS]


def _cot(case, train, seed=7):
    rng = np.random.default_rng(seed)
    cot = (rng.standard_normal((4, case.B)) / case.B).astype(np.float32)
    if not case.naugs:
        cot[3] = 0
    if not train:
        cot[1:] = 0
    return cot


@pytest.mark.parametrize("name,train", COMBOS, ids=IDS)
def test_reference_is_vjp_ref_plus_one_result_and_matches_central_differences(name, train):
    case = GPU_CASES[name]
    cot = _cot(case, train)
    cfg, r64, r32 = R.case_reference(case, cot, train, LAM, tag="host-random")
    flat, xs, eps, ys = case.inputs()
    dts = R.case_dts(case)
    e = eps if train else None
    # 1. identity with vjp_ref
    _, g, gx = V.vjp64(cfg, flat, xs, e, cot, dts, ys, train)
    eg, ex = np.abs(r64[1] - g).max() / V.scale(g), np.abs(r64[2] - gx).max() / V.scale(gx)
    print(f"{name} train={train}: identity grad {eg:.2e}, grad_x {ex:.2e}")
    assert eg <= 1e-13 and ex <= 1e-13, (eg, ex)
    # 2. central differences w.r.t. single entries of ys
    gy = r64[3]
    s = V.scale(gy)
    assert gy.shape == ys.shape and s > 0
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    rng = np.random.default_rng(11)
    h, worst = 1e-6, 0.0
    for _ in range(4):
        k, b = int(rng.integers(case.n_cond)), int(rng.integers(case.B))
        yp, ym = f64(ys).copy(), f64(ys).copy()
        yp[k, b] += h
        ym[k, b] -= h
        op, _, _ = V.outputs(cfg, f64(flat), f64(xs), f64(e), dts, yp, train)
        om, _, _ = V.outputs(cfg, f64(flat), f64(xs), f64(e), dts, ym, train)
        num = float(np.sum(f64(cot) * (op - om)) / (2 * h))
        worst = max(worst, abs(num - gy[k, b]) / s)
    print(f"{name} train={train}: central differences, worst error {worst:.2e} of scale(gy) = {s:.2e}")
    assert worst <= 1e-7, (name, train, worst)
    # 4. the float32 floor leaves the device's bar under its cap
    err, floor, rtol, s_, ok = R.report_ys(r32[3], r64[3], r32[3])
    print(f"{name} train={train}: float32 floor {floor:.2e}, rtol {rtol:.1e}")
    assert s_ > 0 and rtol <= V.RTOL_CAP and ok, (floor, rtol)


@pytest.mark.parametrize("name,train", COMBOS, ids=IDS)
def test_one_hot_sample_leaves_other_columns_exactly_zero(name, train):
    case = GPU_CASES[name]
    j = 5
    cot = np.zeros((4, case.B))
    cot[:, j] = [0.3, -0.2, 0.1, 0.05 if case.naugs else 0.0]
    if not train:
        cot[1:] = 0
    _, r64, _ = R.case_reference(case, cot, train, LAM, tag="host-one-hot")
    gy = r64[3]
    assert np.abs(gy[:, j]).max() > 0
    assert not np.delete(gy, j, axis=1).any(), np.nonzero(np.abs(gy).sum(0))[0]


def test_unconditional_model_is_refused_by_the_reference():
    case = GPU_CASES["generic-cfg2"]
    flat, xs, eps, _ = case.inputs()
    with pytest.raises(ValueError):
        R.vjp_ys64(case.cfg(LAM), flat, xs, eps, np.zeros((4, case.B)), [0.25, 0.25], None)


def test_new_entry_points_are_declared_exported_and_bound():
    """Fails without the feature: both C symbols in the header, the built library and ``_lib.EXPORTS``; the new keyword in
    the two Python signatures."""
    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "cnfhip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cnf_set_grad_ys", "cnf_grad_ys"):
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} is not declared in include/cnfhip.h"
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert name in _lib.EXPORTS, f"{name} is not bound in _lib.EXPORTS"
    assert len(_lib.EXPORTS) == 62
    for fn in (cnf.inference_pullback, cnf.loss_and_grad):
        p = inspect.signature(fn).parameters
        assert "with_ys" in p and p["with_ys"].default is False, fn.__name__
    assert "with_ys" not in inspect.signature(cnf.loss_and_grad_submit).parameters
    assert _lib.lib().cnf_abi_version() == 1
