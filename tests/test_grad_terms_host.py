"""A test of the per-term gradient bar of tests/grad_terms.py, and a guard of its reference (no GPU needed).

- the loss gradient is affine in (lam1, lam2, lam3) for a fixed step sequence (what isolating a term rests on);
- mutants built from the oracle -- a term's share scaled by a few percent or by an approximate-rsqrt-sized error, one
  sample's share of a term off by 30 %, the s'' sweep dropped from the lam2 term -- are rejected by the new bar, and the
  first three are accepted by the other gradient tests' bar at lam = 0.01 (the gap the new bar closes);
- the float32-oracle floor of every case of the GPU matrix leaves room under the cap of rtol;
- the oracle handles zero norms (eps = 0 in some columns; a zero last layer) without a warning, in both precisions.
"""
import warnings

import numpy as np
import pytest

from oracle import cnf_oracle as O
from tests import grad_terms as GT
from tests.test_gpu_parity import _assert_grad        # the other gradient tests' bar: imported, not restated

T = O.ACT_TANH
# the cases the gap was measured on: configs 2, 3 (both compute modes) and 5, tspan (0, 0.5), dt = 1/4, bias scale 0.1
MUTANT_CASES = {c.name: c for c in (
    GT.Case("cfg2", "host", (16, 48, 16), (T,) * 2, 8, 8, 77, 302),
    GT.Case("cfg3", "host", (32, 128, 128, 32), (T,) * 3, 32, 0, 77, 303),
    GT.Case("cfg3-jvp", "host", (32, 128, 128, 32), (T,) * 3, 32, 0, 77, 303, jvp=True),
    GT.Case("cfg5", "host", (128, 384, 128), (T,) * 2, 64, 64, 40, 305),
)}
LAM_OLD = 0.01              # where the other gradient tests run


def _refs(case):
    inputs = case.inputs()
    return inputs, {k: GT.term_reference(case.cfg(GT.one_hot(0)), *inputs, k, case.sol_kw) for k in case.terms}


def _old_bar_accepts(grad, gx, ref_grad, ref_gx, what):
    try:
        _assert_grad(grad, ref_grad, what)
        _assert_grad(gx, ref_gx, what + " d loss / d xs", rtol=2e-4)
    except AssertionError:
        return False
    return True


def _new_bar(got, got_x, ref):
    """(rejected?, worst err / rtol over the parameter blocks, the same for grad_x)."""
    recs = GT.grad_term_report(got, got_x, ref)
    p = max(r["err"] / r["rtol"] for r in recs if r["block"] != "grad_x")
    x = max(r["err"] / r["rtol"] for r in recs if r["block"] == "grad_x")
    return any(not r["ok"] for r in recs), p, x


@pytest.mark.parametrize("name", ["cfg2", "cfg2-jvp", "cond"])
def test_gradient_is_affine_in_the_lambdas(name):
    """g(lam) = g(0) + sum_k lam_k (g(e_k) - g(0)) in float64 to 1e-12, gradient and d loss / d xs: fixed dt, both compute
    modes, with augmentation and with a conditional model."""
    case = {"cfg2": GT.Case("cfg2", "host", (16, 48, 16), (T,) * 2, 8, 8, 21, 11),
            "cfg2-jvp": GT.Case("cfg2-jvp", "host", (16, 48, 16), (T,) * 2, 8, 8, 21, 12, jvp=True),
            "cond": GT.Case("cond", "host", (6, 18, 6), (T, O.ACT_SOFTPLUS), 4, 2, 13, 13, n_cond=3, scale=0.3)}[name]
    inputs, refs = _refs(case)
    lam = (0.3, 0.7, 0.2)
    dts = refs[1].dts
    _, g, gx = GT.oracle_run(case.cfg(lam), *inputs, dts)
    g_aff = refs[1].zero[1] + sum(lam[k - 1] * refs[k].part for k in case.terms)
    gx_aff = refs[1].zero[2] + sum(lam[k - 1] * refs[k].part_x for k in case.terms)
    for k in case.terms:            # every term has a share to isolate
        assert np.abs(refs[k].part).max() > 1e-3 * np.abs(g).max(), k
    assert np.abs(g - g_aff).max() <= 1e-12 * np.abs(g).max(), np.abs(g - g_aff).max()
    assert np.abs(gx - gx_aff).max() <= 1e-12 * np.abs(gx).max(), np.abs(gx - gx_aff).max()


@pytest.mark.parametrize("name", list(MUTANT_CASES))
def test_mutants_pass_the_whole_gradient_bar_and_fail_the_term_bar(name):
    case = MUTANT_CASES[name]
    inputs, refs = _refs(case)
    flat, xs, eps, ys = inputs
    B = case.B
    dts = refs[1].dts
    lam_old = tuple(LAM_OLD for _ in range(3))
    _, g_old, gx_old = GT.oracle_run(case.cfg(lam_old), *inputs, dts)
    for k in case.terms:
        ref = refs[k]
        what = f"{name} {GT.TERM_NAMES[k]}"
        clean = GT.grad_term_report(ref.ref[1], ref.ref[2], ref)
        assert all(r["ok"] for r in clean) and max(r["rtol"] for r in clean) <= GT.RTOL_CAP, what
        print(f"{what}: rtol {min(r['rtol'] for r in clean):.2e} .. {max(r['rtol'] for r in clean):.2e}")

        def mutant(dpart, dpart_x, label, old_accepts=True):
            """The term's share off by (dpart, dpart_x): new bar at lam = e_k, old bar at lam = 0.01."""
            rejected, p, x = _new_bar(ref.ref[1] + dpart, ref.ref[2] + dpart_x, ref)
            print(f"{what}, {label}: new bar err/rtol params {p:.1f} grad_x {x:.1f}")
            assert rejected, (what, label, p, x)
            if old_accepts:
                assert _old_bar_accepts(g_old + LAM_OLD * dpart, gx_old + LAM_OLD * dpart_x, g_old, gx_old, f"{what} {label}"), (what, label)
            return p, x

        # the term's share uniformly off by 3 %, and by an approximate-rsqrt-sized 1e-3
        for f in (0.97, 1.0 + 1e-3):
            p, x = mutant((f - 1.0) * ref.part, (f - 1.0) * ref.part_x, f"share x {f:g}")
            assert p > 1.0 and x > 1.0, (what, f, p, x)                    # (each of the two on its own)
        # the last sample's share of the term off by 30 %: its share is the term's share of that sample alone, over B
        col = lambda a: None if a is None else a[:, -1:]
        one = GT.term_reference(case.cfg(GT.one_hot(0)), flat, col(xs), col(eps), col(ys), k, dict(dts=dts))
        dcol = 0.3 * one.part / B
        dcol_x = np.zeros_like(ref.part_x)
        dcol_x[:, -1:] = 0.3 * one.part_x / B
        np.testing.assert_allclose(one.part_x / B, ref.part_x[:, -1:], rtol=1e-9, atol=1e-15)   # (columns do not interact)
        p, x = mutant(dcol, dcol_x, "last sample's share off by 30 %")
        assert p > 1.0 and x > 1.0, (what, p, x)
        # that sample's share dropped: the old bar sees this one
        assert not _old_bar_accepts(g_old - LAM_OLD * one.part / B, gx_old - LAM_OLD * dcol_x / 0.3, g_old, gx_old, what)
    # s'' zeroed in the lam2 term only (the only data-dependent tangent through the s'' sweep)
    ref = refs[2]
    with GT.without_second_derivative():
        _, gk, gxk = GT.oracle_run(case.cfg(GT.one_hot(2)), *inputs, dts, tag="no second derivative")
        _, g0, gx0 = GT.oracle_run(case.cfg(GT.one_hot(0)), *inputs, dts, tag="no second derivative")
    rejected, p, x = _new_bar(ref.zero[1] + (gk - g0), ref.zero[2] + (gxk - gx0), ref)
    print(f"{name} lam2 without s'': new bar err/rtol params {p:.1f} grad_x {x:.1f}")
    assert rejected and p > 1.0, (name, p, x)


@pytest.mark.parametrize("name", list(GT.GPU_CASES))
def test_float32_floor_of_the_gpu_matrix(name, capsys):
    """The float32 run of the oracle against its float64 run, per block at the scale of the term's share: at most 1.25e-4,
    so that rtol = max(1e-4, 8 x floor) stays under its cap of 1e-3 on every case the device is held to."""
    case = GT.GPU_CASES[name]
    inputs = case.inputs()
    for k in case.terms:
        ref = GT.term_reference(case.cfg(GT.one_hot(0)), *inputs, k, case.sol_kw)
        floors = GT.term_floors(ref)
        with capsys.disabled():
            print(f"\nfloor {name} {GT.TERM_NAMES[k]} ({len(ref.dts)} steps): " +
                  " ".join(f"{b} {f:.1e}" for b, (_, f) in floors.items()), end="")
        for b, (scale, floor) in floors.items():
            assert scale > 0 and np.isfinite(floor), (name, k, b)
            assert floor <= GT.FLOOR_MAX, (name, k, b, floor)
            assert GT.rtol_of(floor) <= GT.RTOL_CAP


@pytest.mark.parametrize("which", GT.DEGENERATE)
@pytest.mark.parametrize("name", ["cfg2", "cfg2-jvp", "three-layer-cond"])
def test_oracle_handles_zero_norms(name, which):
    """eps = 0 in a few columns (|eps' J| = 0 there only); W_L = b_L = 0 (zdot = 0, the augmented rows stay 0: all three norms
    are 0 at every stage).  The unit vector of a zero vector is 0: finite gradients without a floating-point warning, in
    float64 and float32, and the two agree."""
    case = {"cfg2": GT.Case("cfg2", "host", (16, 48, 16), (T,) * 2, 8, 8, 19, 21),
            "cfg2-jvp": GT.Case("cfg2-jvp", "host", (16, 48, 16), (T,) * 2, 8, 8, 19, 22, jvp=True),
            "three-layer-cond": GT.Case("three-layer-cond", "host", (12, 64, 48, 12), (T, O.ACT_SOFTPLUS, T), 8, 4, 9, 23, n_cond=3)}[name]
    inputs = GT.degenerate_inputs(case, which)
    cfg = case.cfg((1.0, 1.0, 1.0))
    dts = GT.resolve_steps(cfg, *inputs, case.sol_kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v64, g64, gx64 = GT.oracle_run(cfg, *inputs, dts, np.float64)
        v32, g32, gx32 = GT.oracle_run(cfg, *inputs, dts, np.float32)
    for a in (v64, g64, gx64, v32, g32, gx32):
        assert np.isfinite(a).all()
    assert np.abs(g64).max() > 0
    _assert_grad(g32.astype(np.float64), g64, f"{name} {which}: float32 oracle")
    _assert_grad(gx32.astype(np.float64), gx64, f"{name} {which}: float32 oracle, d loss / d xs", rtol=2e-4)
    if which == "zero-last-layer":
        # the regulariser terms have no share at all here: the gradient is that of lam = 0
        _, g0, gx0 = GT.oracle_run(case.cfg((0.0, 0.0, 0.0)), *inputs, dts, np.float64)
        assert np.array_equal(g0, g64) and np.array_equal(gx0, gx64)
