"""tests/vjp_ref.py, the float64 reference of the weighted pullback of ``inference``, pinned three ways without a device,
and the presence of the new entry points (header, built library, bindings, Python mirror).

1. identity: the cotangent of the built-in loss reproduces ``G.loss_and_grad`` (gradient and grad_x) to 1e-12 of the
   gradient's scale -- float64 reassociation is three orders below that, a missing or mis-signed term (each regulariser's
   share of a block is 1e-4 .. 1e-3 of it at lam = 0.01 .. 0.03) nine orders above;
2. central differences in float64 of sum(cot * outputs) along random parameter directions at fixed steps: relative error
   <= 1e-5 at step 1e-6 (truncation + rounding of the quotient; three orders under a wrong term);
3. a cotangent that is non-zero in one sample only gives a grad_xs that is EXACTLY zero in every other column: what catches
   a mis-indexed per-sample weight, which no uniform-weight test can see.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import cnf_grad_oracle as G
from oracle import cnf_oracle as O
from tests import vjp_ref as V

T = O.ACT_TANH
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#        name                  dims                 nvars naugs B   tspan       dt     jvp    bias scale
CASES = [("16x48x16-B32", (16, 48, 16), 8, 8, 32, (0.0, 1.0), 0.125, False, 0.3),
         ("headline-B33", (32, 128, 128, 32), 32, 0, 33, (0.0, 0.5), 0.25, False, 0.1),
         ("headline-B77-jvp", (32, 128, 128, 32), 32, 0, 77, (0.0, 0.5), 0.25, True, 0.1),
         ("30x120x116-aug10-B33", (30, 120, 116, 30), 20, 10, 33, (0.0, 0.5), 0.25, False, 0.1),
         ("128x384x128-B40", (128, 384, 128), 64, 64, 40, (0.0, 0.5), 0.25, False, 0.1)]
IDS = [c[0] for c in CASES]
f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)


def _case(c, lam):
    name, dims, nvars, naugs, B, tspan, dt, jvp, sc = c
    net = O.Net(dims, (T,) * (len(dims) - 1))
    cfg = O.Cfg(net, nvars, naugs, lam[0], lam[1], lam[2] if naugs else 0.0, use_jvp=jvp, tspan=tspan)
    rng = np.random.default_rng(2024)
    flat = O.glorot_params(net, rng, np.float32, sc)
    xs = rng.standard_normal((nvars, B)).astype(np.float32)
    eps = rng.standard_normal((nvars + naugs, B)).astype(np.float32)
    cot = (rng.standard_normal((4, B)) / B).astype(np.float32)
    if not naugs:
        cot[3] = 0
    dts = [dt] * int(round(abs(tspan[1] - tspan[0]) / dt))
    return cfg, flat, xs, eps, cot, dts, rng


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_loss_cotangent_reproduces_loss_and_grad(c):
    cfg, flat, xs, eps, _, dts, _ = _case(c, (0.01, 0.02, 0.03))
    B = xs.shape[1]
    _, g, gx = V.vjp64(cfg, flat, xs, eps, V.loss_cotangent(cfg, B), dts)
    _, gr, st = G.loss_and_grad(cfg, f64(flat), f64(xs), f64(eps), None, dts=dts)
    e, ex = np.abs(g - gr).max() / V.scale(gr), np.abs(gx - st.grad_x).max() / V.scale(st.grad_x)
    print(f"{c[0]}: identity grad {e:.2e}, grad_x {ex:.2e}")
    assert e <= 1e-12 and ex <= 1e-12, (c[0], e, ex)


def test_testmode_loss_cotangent_reproduces_loss_and_grad_test():
    for dims, nvars, naugs, B, ncond in (((32, 128, 128, 32), 32, 0, 16, 0), ((12, 64, 48, 12), 8, 4, 24, 3)):
        net = O.Net((dims[0] + ncond,) + dims[1:], (T, O.ACT_SOFTPLUS, T))
        cfg = O.Cfg(net, nvars, naugs, tspan=(0.0, 0.5))
        rng = np.random.default_rng(3)
        flat = O.glorot_params(net, rng, np.float32, 0.2)
        xs = rng.standard_normal((nvars, B)).astype(np.float32)
        ys = rng.standard_normal((ncond, B)).astype(np.float32) if ncond else None
        dts = [0.25, 0.25]
        _, g, gx = V.vjp64(cfg, flat, xs, None, V.loss_cotangent(cfg, B, train=False), dts, ys, train=False)
        _, gr, st = G.loss_and_grad_test(cfg, f64(flat), f64(xs), f64(ys), dts=dts)
        e, ex = np.abs(g - gr).max() / V.scale(gr), np.abs(gx - st.grad_x).max() / V.scale(st.grad_x)
        print(f"TestMode {dims}: identity grad {e:.2e}, grad_x {ex:.2e}")
        assert e <= 1e-12 and ex <= 1e-12, (dims, e, ex)
        # central differences of sum(cot * logpx)
        cot = np.zeros((4, B))
        cot[0] = rng.standard_normal(B) / B
        _, g64, _ = V.vjp64(cfg, flat, xs, None, cot, dts, ys, train=False)
        d = rng.standard_normal(flat.size)
        d /= np.linalg.norm(d)
        h = 1e-6
        op, _, _ = V.outputs(cfg, f64(flat) + h * d, f64(xs), None, dts, f64(ys), train=False)
        om, _, _ = V.outputs(cfg, f64(flat) - h * d, f64(xs), None, dts, f64(ys), train=False)
        num = float(np.sum(cot * (op - om)) / (2 * h))
        rel = abs(num - float(g64 @ d)) / abs(num)
        print(f"TestMode {dims}: central differences {rel:.2e}")
        assert rel <= 1e-5, (dims, rel)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_central_differences(c):
    cfg, flat, xs, eps, cot, dts, rng = _case(c, (1.0, 1.0, 1.0))
    _, g64, _ = V.vjp64(cfg, flat, xs, eps, cot, dts)
    worst = 0.0
    for _ in range(3):
        d = rng.standard_normal(flat.size)
        d /= np.linalg.norm(d)
        h = 1e-6
        op, _, _ = V.outputs(cfg, f64(flat) + h * d, f64(xs), f64(eps), dts)
        om, _, _ = V.outputs(cfg, f64(flat) - h * d, f64(xs), f64(eps), dts)
        num = float(np.sum(f64(cot) * (op - om)) / (2 * h))
        worst = max(worst, abs(num - float(g64 @ d)) / abs(num))
    print(f"{c[0]}: central differences, worst relative error {worst:.2e}")
    assert worst <= 1e-5, (c[0], worst)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_one_hot_sample_leaves_other_columns_exactly_zero(c):
    cfg, flat, xs, eps, _, dts, _ = _case(c, (1.0, 1.0, 1.0))
    B, j = xs.shape[1], 5
    cot = np.zeros((4, B))
    cot[:, j] = [0.3, -0.2, 0.1, 0.05 if cfg.naugs else 0.0]
    _, g, gx = V.vjp64(cfg, flat, xs, eps, cot, dts)
    assert np.abs(g).max() > 0 and np.abs(gx[:, j]).max() > 0
    others = np.delete(gx, j, axis=1)
    assert not others.any(), (c[0], np.nonzero(np.abs(gx).sum(0))[0])


def test_float32_floor_of_the_reference_leaves_the_bar_at_1e_minus_4():
    """The float32 run of the same reference is what the device is allowed to cost: on the cheapest case and every row
    cotangent it stays 40 times under the point where it would lift rtol above 1e-4."""
    cfg, flat, xs, eps, _, dts, rng = _case(CASES[0], (1.0, 1.0, 1.0))
    for name, cot in V.row_cotangents(rng, xs.shape[1], (0, 1, 2, 3)).items():
        _, g64, x64 = V.vjp64(cfg, flat, xs, eps, cot, dts)
        _, g32, x32 = V.vjp32(cfg, flat, xs, eps, cot, dts)
        recs = V.report(g64, x64, (g64, x64), (g32, x32), cfg.net)
        floor = max(r[2] for r in recs)
        print(f"{CASES[0][0]} {name}: float32 floor {floor:.2e}")
        assert 8 * floor <= 1e-4 / 5, (name, floor)


def test_new_entry_points_are_declared_exported_and_bound():
    """Fails without the feature: both C symbols in the header, the built library and ``_lib.EXPORTS``; the three Python
    functions and the two ready-made losses in the package."""
    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "cnfhip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cnf_inference_record", "cnf_inference_pullback"):
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} is not declared in include/cnfhip.h"
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert name in _lib.EXPORTS, f"{name} is not bound in _lib.EXPORTS"
    for name in ("inference_record", "inference_pullback", "differentiable_inference", "weighted_loss", "tempered_loss"):
        assert callable(getattr(cnf, name, None)), name
    assert _lib.lib().cnf_abi_version() == 1
