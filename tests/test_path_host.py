"""Flow paths without a device: the digits of Tsit5's interpolant against the tableau and the order conditions, its order on a
nonlinear ODE, the save-time checks (Python and C) before any handle exists, and the two entry points of include/cnfhip_path.h
declared, exported and bound."""
import ctypes
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from continuousnf.jl_amd.path import check_saveat
from oracle import cnf_oracle as O
from tests import path_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cnf_path_steps", "cnf_solve_path"]
THETAS = np.linspace(0.0, 1.0, 41)
# Every r_ij is given to double precision (half an ulp relative) and a Horner evaluation adds at most one rounding per
# coefficient: an identity in the b_i(theta), theta in [0, 1], is met to 4 eps64 sum_ij |r_ij| (4e-13) whatever the digits' last
# place.  (Measured when the table was written: 6e-15 at theta = 1, 5e-15 on the order conditions.)
BOUND = 4 * np.finfo(np.float64).eps * float(np.abs(R.R).sum())


def test_entry_points_are_declared_exported_and_bound():
    """Fails without the feature."""
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_path.h"', main, flags=re.M)
    txt = strip(open(os.path.join(ROOT, "include", "cnfhip_path.h")).read())
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", txt)))
    assert declared == NAMES, declared
    assert set(declared) == set(_lib.PATH_EXPORTS)
    for other in (_lib.EXPORTS, _lib.SAMPLING_EXPORTS, _lib.BASEGRAD_EXPORTS, _lib.ENSEMBLE_EXPORTS, _lib.ENSEMBLE_EVAL_EXPORTS):
        assert not set(declared) & set(other)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    for name in ("solve_path", "inference_path", "generate_path"):
        assert callable(getattr(cnf, name, None)), name


def test_interpolant_ends_on_the_tableau():
    """b_i(1) = a_7i (the step's own weights) and b_7(1) = 0: theta = 1 is the accepted state; b_i(0) = 0."""
    b1 = np.array(R.dense_b(1.0))
    assert np.max(np.abs(b1[:6] - np.array(O.TSIT5_A[6]))) <= BOUND
    assert abs(b1[6]) <= BOUND
    assert np.all(np.array(R.dense_b(0.0)) == 0.0)


def test_interpolant_meets_the_order_conditions():
    """sum_i b_i(theta) c_i^m = theta^(m+1) / (m+1) for m = 0..3: quadrature conditions of a 4th-order continuous extension."""
    c = np.array(O.TSIT5_C)
    worst = 0.0
    for th in THETAS:
        b = np.array(R.dense_b(th))
        for m in range(4):
            worst = max(worst, abs(float(np.sum(b * c ** m)) - th ** (m + 1) / (m + 1)))
    assert worst <= BOUND, worst


def _exact(t):
    """u1' = -u1^2, u2' = u2 (1 - u2) cos t: u1 = 1 / (1 + t), u2 = 1 / (1 + 3 exp(-sin t))."""
    return np.array([1.0 / (1.0 + t), 1.0 / (1.0 + 3.0 * np.exp(-np.sin(t)))])


def test_interpolant_is_fifth_order_locally():
    """One step of size h from the exact solution of a nonlinear ODE: the interpolation error at theta in {0.3, 0.5, 0.7} falls by
    2^5 = 32 per halving of h (a third-order interpolant would give 16); at least 24 on the last two halvings."""
    t0 = 0.3
    err = []
    for h in (0.4, 0.2, 0.1, 0.05):
        worst = 0.0
        for th in (0.3, 0.5, 0.7):
            # (autonomous form: the time is a third component)
            f = lambda u: np.array([-u[0] ** 2, u[1] * (1.0 - u[1]) * np.cos(u[2]), 1.0])
            u = np.append(_exact(t0), t0)
            _, ks = R.tsit5_step_all(f, u, f(u), h)
            got = R.interpolate(u, ks, h, th)[:2]
            worst = max(worst, float(np.max(np.abs(got - _exact(t0 + th * h)))))
        err.append(worst)
    ratios = [err[i] / err[i + 1] for i in range(3)]
    print("interpolation errors", err, "ratios", ratios)
    assert ratios[1] >= 24 and ratios[2] >= 24, (err, ratios)


def test_the_float32_form_is_the_float64_form_rounded():
    """The library evaluates the b_i in fp32: the same polynomial to a few fp32 roundings of its largest terms."""
    for th in THETAS:
        b32, b64 = np.array(R.dense_b(th, np.float32), dtype=np.float64), np.array(R.dense_b(th))
        assert np.max(np.abs(b32 - b64)) <= 4 * np.finfo(np.float32).eps * np.abs(R.R).sum(axis=1).max()


BAD_SAVEAT = [([], "empty"), ([0.5, float("nan")], "finite"), ([0.5, float("inf")], "finite"), ([0.5, 0.25], "monotone"),
              ([-0.1, 0.5], "inside"), ([0.5, 1.5], "inside")]


@pytest.mark.parametrize("saveat,word", BAD_SAVEAT)
def test_check_saveat_refuses(saveat, word):
    with pytest.raises(ValueError, match=word):
        check_saveat(saveat, (0.0, 1.0))


def test_check_saveat_accepts_both_directions_and_repeats():
    assert check_saveat([0.0, 0.5, 0.5, 1.0], (0.0, 1.0)).dtype == np.float32
    assert list(check_saveat([1.0, 0.5, 0.0], (1.0, 0.0))) == [1.0, 0.5, 0.0]
    with pytest.raises(ValueError, match="monotone"):
        check_saveat([0.0, 0.5, 1.0], (1.0, 0.0))


def _model():
    nn = cnf.Chain(cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh"))
    return cnf.construct(cnf.RNODE, nn, 1, 1, rng=5)


@pytest.mark.parametrize("saveat,word", BAD_SAVEAT)
def test_python_entry_points_check_saveat_before_any_handle(saveat, word):
    """ValueError, not the CNFError a handle would raise on a machine without a device -- and no handle afterwards."""
    ic = _model()
    xs = np.zeros((1, 4), dtype=np.float32)
    flat = np.zeros(32, dtype=np.float32)
    with pytest.raises(ValueError, match=word):
        cnf.inference_path(ic, cnf.TestMode(), xs, flat, {}, saveat=saveat)
    rev = [1.0 - s for s in saveat]
    with pytest.raises(ValueError, match=word):
        cnf.generate_path(ic, cnf.TestMode(), flat, {}, 4, saveat=rev)
    assert ic._handle is None


def test_generate_path_wants_the_reversed_direction():
    ic = _model()
    with pytest.raises(ValueError, match="monotone"):
        cnf.generate_path(ic, cnf.TestMode(), np.zeros(32, dtype=np.float32), {}, 4, saveat=[0.0, 0.5, 1.0])


def test_the_c_call_checks_saveat_before_the_handle():
    """With no handle at all every complaint about the save times still comes first: CNF_ERR_BAD_ARG, nothing touched."""
    l = _lib.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    opts = _lib.cnf_solve_opts(0.0, 1.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)
    rev = _lib.cnf_solve_opts(1.0, 0.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)

    def call(saveat, o=opts, K=None, out=p):
        sv = np.asarray(saveat, dtype=np.float32)
        return l.cnf_solve_path(None, _lib.MODE_TEST, p, None, p, 4, ctypes.byref(o), sv.ctypes.data if sv.size else p,
                                sv.size if K is None else K, out, None, None)
    for saveat, _ in BAD_SAVEAT:
        assert call(saveat) == _lib.ERR_BAD_ARG, saveat
    assert call([0.0, 0.5, 1.0], o=rev) == _lib.ERR_BAD_ARG                # wrong direction
    assert call([0.5], K=-1) == _lib.ERR_BAD_ARG
    assert call([0.5], out=None) == _lib.ERR_BAD_ARG
    assert l.cnf_solve_path(None, _lib.MODE_TEST, p, None, p, 4, ctypes.byref(opts), None, 1, p, None, None) == _lib.ERR_BAD_ARG
    assert call([0.0, 0.5, 1.0]) == _lib.ERR_BAD_ARG                       # good save times: the NULL handle is the complaint
    assert l.cnf_path_steps(None, None, None, 0) == -1
