"""tests/gen_vjp_ref.py, the float64 reference of differentiable sampling, pinned without a device, and the presence of the
new entry points (header, built library, bindings, Python mirror).

1. torch float64 autograd through the same Tsit5 steps over the reversed span, on a tiny 3-5-3 network with B = 3: TrainMode
   VJP and JVP, TestMode, one conditional model; gradient, grad_z0 and grad_ys to 1e-10 of their scale (float64
   reassociation is four orders below, a missing or mis-signed term ten orders above);
2. central differences in float64 along random directions in the parameters and in z0: relative error <= 1e-5 at step 1e-6;
3. the identity everything rests on: ``logq`` of the generated sample equals ``logpx`` of ``inference(TestMode)`` of it, up to
   the discretisation error of the two solves, which falls with the step as Tsit5's order says;
4. a cotangent in one sample only gives a grad_z0 that is exactly zero in every other column;
5. for every case of tests/test_gpu_generate_vjp.py the float32 run of the reference keeps each block's
   rtol = max(1e-4, 8 floor) under the cap 1e-3, and no block's scale is zero.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import cnf_oracle as O
from tests import basedist_ref as BR
from tests import cond_grad_ref as CR
from tests import gen_vjp_ref as R
from tests import grad_terms as GT
from tests import vjp_ref as V

torch = pytest.importorskip("torch")

T = O.ACT_TANH
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)

#        name         train  jvp    n_cond
TINY = [("train-vjp", True, False, 0), ("train-jvp", True, True, 0), ("test", False, False, 0), ("train-cond", True, False, 2),
        ("test-cond", False, False, 2)]
DTS = [0.3, 0.45, 0.25]                     # over (1 -> 0)


def _tiny(train, jvp, n_cond, seed=5):
    net = O.Net((3 + n_cond, 5, 3), (T, T))
    cfg = O.Cfg(net, 2, 1, 1.0, 1.0, 1.0, use_jvp=jvp, tspan=(0.0, 1.0))
    rng = np.random.default_rng(seed)
    B = 3
    flat = O.glorot_params(net, rng, np.float64, 0.3)
    z0 = rng.standard_normal((3, B))
    eps = rng.standard_normal((3, B)) if train else None
    ys = rng.standard_normal((n_cond, B)) if n_cond else None
    cz, cl = rng.standard_normal((3, B)), rng.standard_normal(B)
    return cfg, flat, z0, eps, ys, cz, cl, rng


# ---- the same discrete map in torch (two tanh layers, the Jacobian written out per sample) ----
def _torch_rhs(net, flat, eps, ys, train, jvp):
    n_in = net.dims[0] - (0 if ys is None else ys.shape[0])
    Ws, bs, off = [], [], 0
    for i, o in zip(net.dims[:-1], net.dims[1:]):
        Ws.append(flat[off:off + i * o].reshape(i, o).t())
        off += i * o
        bs.append(flat[off:off + o])
        off += o

    def f(u):
        z = u[:n_in]
        h = z if ys is None else torch.cat([z, ys])
        J = None                                             # [B][rows][n_in]
        for W, b in zip(Ws, bs):
            h = torch.tanh(W @ h + b[:, None])
            M = (1 - h * h).t()[:, :, None] * W[None]
            J = M[:, :, :n_in] if J is None else M @ J
        if train:
            v = torch.einsum("bij,jb->ib", J, eps) if jvp else torch.einsum("ib,bij->jb", eps, J)
            ldot = -(v * eps).sum(0, keepdim=True)
            return torch.cat([h, ldot, h.norm(dim=0)[None], v.norm(dim=0)[None]])
        return torch.cat([h, -torch.diagonal(J, dim1=1, dim2=2).sum(1)[None]])
    return f


def _torch_generate(cfg, flat, z0, eps, ys, train, dts, base=None):
    f = _torch_rhs(cfg.net, flat, eps, ys, train, cfg.use_jvp)
    u = torch.cat([z0, torch.zeros(cfg.D(train) - cfg.n_in, z0.shape[1], dtype=z0.dtype)])
    tdir = -1.0                                              # reverse(tspan) of (0, 1)
    for h in dts:
        ks = [f(u)]
        for s in range(1, 7):
            acc = sum(O.TSIT5_A[s][j] * ks[j] for j in range(s))
            us = u + tdir * h * acc
            if s < 6:
                ks.append(f(us))
        u = us
    n = cfg.n_in
    if base is None:
        logpz = -0.5 * (n * np.log(2 * np.pi) + (z0 * z0).sum(0))
    else:
        d = z0 - torch.from_numpy(base.mean)[:, None]
        logpz = -0.5 * (n * np.log(2 * np.pi) + base.logdet + (d * (torch.from_numpy(base.prec) @ d)).sum(0))
    return u[:n], logpz + u[n]


@pytest.mark.parametrize("name,train,jvp,n_cond", TINY, ids=[t[0] for t in TINY])
@pytest.mark.parametrize("dist", ["std", "full"])
def test_torch_autograd_pins_the_reference(name, train, jvp, n_cond, dist):
    cfg, flat, z0, eps, ys, cz, cl, rng = _tiny(train, jvp, n_cond)
    base = BR.Gauss(0.3 * rng.standard_normal(3), BR.random_cov(rng, 3, "full")) if dist == "full" else None
    z, logq, g, gz0, gy = R.vjp64(cfg, flat, z0, eps, cz, cl, DTS, ys, train, base)
    t = lambda a, req=False: None if a is None else torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(req)
    tf, tz0, tys = t(flat, True), t(z0, True), t(ys, ys is not None)
    tz, tlq = _torch_generate(cfg, tf, tz0, t(eps), tys, train, DTS, base)
    S = (t(cz) * tz).sum() + (t(cl) * tlq).sum()
    grads = torch.autograd.grad(S, [tf, tz0] + ([tys] if ys is not None else []))
    assert np.abs(z - tz.detach().numpy()).max() <= 1e-12 and np.abs(logq - tlq.detach().numpy()).max() <= 1e-12
    for what, a, b in (("grad", g, grads[0]), ("grad_z0", gz0, grads[1])) + ((("grad_ys", gy, grads[2]),) if ys is not None else ()):
        e = np.abs(a - b.numpy()).max() / V.scale(b.numpy())
        print(f"{name} {dist} {what}: {e:.2e}")
        assert e <= 1e-10, (name, what, e)


@pytest.mark.parametrize("name,train,jvp,n_cond", TINY, ids=[t[0] for t in TINY])
def test_central_differences(name, train, jvp, n_cond):
    cfg, flat, z0, eps, ys, cz, cl, rng = _tiny(train, jvp, n_cond)
    _, _, g, gz0, gy = R.vjp64(cfg, flat, z0, eps, cz, cl, DTS, ys, train)

    def S(flat_, z0_, ys_):
        z, logq, _, _ = R.forward(cfg, flat_, z0_, eps, DTS, ys_, train)
        return float(np.sum(cz * z) + np.sum(cl * logq))

    h = 1e-6
    for _ in range(3):
        df, dz = rng.standard_normal(flat.size), rng.standard_normal(z0.shape)
        dy = rng.standard_normal(ys.shape) if ys is not None else None
        df, dz = df / np.linalg.norm(df), dz / np.linalg.norm(dz)
        num = (S(flat + h * df, z0, ys) - S(flat - h * df, z0, ys)) / (2 * h)
        assert abs(num - g @ df) <= 1e-5 * abs(num), (name, "params", num, g @ df)
        num = (S(flat, z0 + h * dz, ys) - S(flat, z0 - h * dz, ys)) / (2 * h)
        assert abs(num - np.sum(gz0 * dz)) <= 1e-5 * abs(num), (name, "z0", num, np.sum(gz0 * dz))
        if ys is not None:
            num = (S(flat, z0, ys + h * dy) - S(flat, z0, ys - h * dy)) / (2 * h)
            assert abs(num - np.sum(gy * dy)) <= 1e-5 * abs(num), (name, "ys", num, np.sum(gy * dy))


def test_logq_is_the_testmode_logpx_of_the_generated_sample():
    """TestMode, 6-18-6 tanh: generate over (1 -> 0), then ``inference`` of the sample over (0 -> 1) with four times as many
    steps.  The two numbers differ by the discretisation error of the two solves alone: under 1e-9 at 20 steps of 0.05 (Tsit5's
    fifth order: 0.05^5 = 3e-7 times its error constant), and at least 8 times smaller than at 10 steps of 0.1 (order five
    gives 32; a wrong sign or a dropped term leaves an O(1) difference at every step size)."""
    net = O.Net((6, 18, 6), (T, T))
    cfg = O.Cfg(net, 6, 0, tspan=(0.0, 1.0))
    rng = np.random.default_rng(17)
    flat = O.glorot_params(net, rng, np.float64, 0.3)
    z0 = rng.standard_normal((6, 5))
    errs = []
    for nsteps in (10, 20):
        x, logq, _, _ = R.forward(cfg, flat, z0, None, [1.0 / nsteps] * nsteps, train=False)
        out, _, _ = V.outputs(cfg, flat, x, None, [0.25 / nsteps] * (4 * nsteps), train=False)
        errs.append(float(np.abs(out[0] - logq).max()))
    print(f"identity: |logq - logpx| = {errs[0]:.2e} at h = 0.1, {errs[1]:.2e} at h = 0.05")
    assert errs[1] <= 1e-9 and errs[1] <= errs[0] / 8, errs


@pytest.mark.parametrize("name,train,jvp,n_cond", TINY, ids=[t[0] for t in TINY])
def test_one_hot_sample_leaves_other_columns_exactly_zero(name, train, jvp, n_cond):
    cfg, flat, z0, eps, ys, cz, cl, _ = _tiny(train, jvp, n_cond)
    j = 1
    keep = np.zeros(3)
    keep[j] = 1.0
    _, _, g, gz0, gy = R.vjp64(cfg, flat, z0, eps, cz * keep, cl * keep, DTS, ys, train)
    assert np.abs(g).max() > 0 and np.abs(gz0[:, j]).max() > 0
    assert not np.delete(gz0, j, axis=1).any()
    if gy is not None:
        assert np.abs(gy[:, j]).max() > 0 and not np.delete(gy, j, axis=1).any()
    _, _, g, gz0, _ = R.vjp64(cfg, flat, z0, eps, None, None, DTS, ys, train)
    assert not g.any() and not gz0.any()


# ---- the cases of the device tests: what the float32 run of the same reference costs ----
TRAIN_CASES = ("adj3b-B1-fixed", "adj3b-B33-fixed", "adj3b-B77-replay", "adj3-30x120x116-aug", "mfma-cfg5-vjp",
               "mfma-12x64x48-cond-jvp", "generic-cfg2", "wave-16x48-B32-replay")
TEST_CASES = [((32, 128, 128, 32), 32, 0, 16, 0), ((12, 64, 48, 12), 8, 4, 24, 3)]


def lam_of(case):
    return (1.0, 1.0, 1.0 if case.naugs else 0.0)


def host_dts(case, cfg, flat, z0, eps, ys):
    """Fixed cases: their steps; adaptive ones: those the float64 oracle's controller accepts over the reversed span."""
    if case.steps[0] == "fixed":
        return R.fixed_dts(case)
    u0 = np.vstack([f64(z0), np.zeros((3, case.B))])
    _, st = O.tsit5_solve(cfg.rhs(f64(flat), f64(eps), True, f64(ys)), u0, cfg.tspan[1], cfg.tspan[0], **case.sol_kw)
    return list(st.dts)


def inputs_of_testmode(dims, nvars, naugs, B, ncond):
    """The inputs of tests/test_gpu_inference_vjp.TEST_CASES, and a base draw behind them."""
    net = O.Net((dims[0] + ncond,) + dims[1:], (T, O.ACT_SOFTPLUS, T))
    cfg = O.Cfg(net, nvars, naugs, tspan=(0.0, 0.5))
    rng = np.random.default_rng(3)
    flat = O.glorot_params(net, rng, np.float32, 0.2)
    rng.standard_normal((nvars, B))
    ys = rng.standard_normal((ncond, B)).astype(np.float32) if ncond else None
    z0 = rng.standard_normal((nvars + naugs, B)).astype(np.float32)
    return net, cfg, flat, z0, ys


def basedist_inputs():
    """The full-covariance case, built like test_gpu_inference_vjp.test_full_covariance_basedist."""
    case = GT.Case("basedist-16x48", "adj_mfma", (16, 48, 16), (T,) * 2, 8, 8, 32, 1701, scale=0.3)
    rng = np.random.default_rng(5)
    mean, cov = 0.3 * rng.standard_normal(16), BR.random_cov(rng, 16, "full")
    return case, mean, cov


def check_floors(what, cfg, flat, z0, eps, ys, dts, cots, train=True, base=None, net=None):
    for k, (cz, cl) in cots.items():
        r64 = R.vjp64(cfg, flat, z0, eps, cz, cl, dts, ys, train, base)
        r32 = R.vjp32(cfg, flat, z0, eps, cz, cl, dts, ys, train, base)
        recs = V.report(r64[2], r64[3], (r64[2], r64[3]), (r32[2], r32[3]), net or cfg.net)
        if ys is not None:
            _, floor, rtol, s, _ = CR.report_ys(r64[4], r64[4], r32[4])
            recs.append(("grad_ys", 0.0, floor, rtol, s, True))
        print(f"{what} cot={k}: " + "; ".join(f"{n} floor {f:.1e} rtol {r:.1e}" for n, _, f, r, _, _ in recs))
        for n, _, f, r, s, _ in recs:
            assert s > 0, (what, k, n)
            assert r <= V.RTOL_CAP, (what, k, n, f, r)


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_float32_floor_of_the_device_cases(name):
    case = GT.GPU_CASES[name]
    flat, _, eps, ys = case.inputs()
    z0 = R.case_z0(case)
    cfg = case.cfg(lam_of(case))
    dts = host_dts(case, cfg, flat, z0, eps, ys)
    n_in = case.nvars + case.naugs
    cots = R.cotangents(np.random.default_rng(case.seed + 7), n_in, case.nvars, case.B, aug_rows=case.naugs > 0)
    check_floors(name, cfg, flat, z0, eps, ys, dts, cots)


@pytest.mark.parametrize("dims,nvars,naugs,B,ncond", TEST_CASES, ids=["32x128x128x32-B16", "12x64x48x12-cond-B24"])
def test_float32_floor_of_the_testmode_cases(dims, nvars, naugs, B, ncond):
    net, cfg, flat, z0, ys = inputs_of_testmode(dims, nvars, naugs, B, ncond)
    cots = R.cotangents(np.random.default_rng(7), nvars + naugs, nvars, B)
    check_floors(f"TestMode {dims}", cfg, flat, z0, None, ys, [0.25, 0.25], cots, train=False)


def test_float32_floor_of_the_basedist_case():
    case, mean, cov = basedist_inputs()
    flat, _, eps, _ = case.inputs()
    z0 = BR.Gauss(mean, cov).sample_from(R.case_z0(case)).astype(np.float32)
    cots = R.cotangents(np.random.default_rng(9), 16, 8, case.B)
    check_floors("basedist", case.cfg((1.0, 1.0, 1.0)), flat, z0, eps, None, R.fixed_dts(case), cots, base=BR.Gauss(mean, cov))


def test_new_entry_points_are_declared_exported_and_bound():
    """Fails without the feature.  The two C symbols are declared in include/cnfhip_generate.h, which include/cnfhip.h includes
    (so a C caller gets them from the one header); they are exported by the built library and bound in
    ``_lib.SAMPLING_EXPORTS``; the Python functions are in the package.

    NOT as the issue words it: it asks for the declarations in cnfhip.h itself and the bindings in ``_lib.EXPORTS``.
    tests/test_cond_grad_host.py pins ``len(_lib.EXPORTS) == 62`` and tests/test_abi_symbols.py pins the names cnfhip.h itself
    declares to be exactly ``EXPORTS``; no entry point can be added to either place while both hold, so the sampling direction
    has a header and a table of its own, held here to test_abi_symbols' rule: the declared names are exactly the bound ones."""
    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import _lib
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_generate.h"', main, flags=re.M), "cnfhip.h does not include cnfhip_generate.h"
    txt = strip(open(os.path.join(ROOT, "include", "cnfhip_generate.h")).read())
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", txt)))
    assert declared == ["cnf_generate_pullback", "cnf_generate_record"], declared
    assert set(declared) == set(_lib.SAMPLING_EXPORTS) and not set(declared) & set(_lib.EXPORTS)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    for name in ("generate_record", "generate_pullback", "differentiable_generate", "reverse_kl"):
        assert callable(getattr(cnf, name, None)), name
    assert _lib.lib().cnf_abi_version() == 1
