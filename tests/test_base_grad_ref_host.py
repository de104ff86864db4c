"""The reference of the gradient w.r.t. a learnable base distribution (tests/base_grad_ref.py) against central differences and
the closed form, the float32 floor of every device case of tests/test_gpu_base_grad.py, the two new C entry points (header,
export, binding table) and the ``ValueError`` paths of the Python surface.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import base_grad_ref as BG
from tests import gen_vjp_ref as R

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["n3-diag-B17", "n16-dense-B17-jvp", "n33-dense-B17-test"]
_FLOOR = {}


def _density_refs(name):
    """(ref64, ref32, summands, ws) of the density direction of a case, for its three cotangents."""
    case, dense, train, cfg, (flat, xs, eps, ys), mean, scale, _, rng = BG.case_setup(name)
    dts = R.fixed_dts(case)
    z64 = BG.final_state(cfg, flat, xs, eps, dts, ys, train, np.float64)
    z32 = BG.final_state(cfg, flat, xs, eps, dts, ys, train, np.float32)
    out = []
    for w in BG.cotangents_w(rng, case.B):
        r64 = BG.logpdf_grads(z64, w, mean, scale, dense, np.float64)
        r32 = BG.logpdf_grads(z32, w, mean, scale, dense, np.float32)
        out.append((r64, r32, BG.summands_of(r64[1], np.sum(w, dtype=np.float64), scale, dense), w))
    return out


# ---- the reference itself ----
@pytest.mark.parametrize("dense", [False, True], ids=["diag", "dense"])
def test_autograd_is_the_closed_form(dense):
    rng = np.random.default_rng(3)
    n, B = 7, 11
    mean, scale = BG.base_of(n, dense, 5)
    z, w = rng.standard_normal((n, B)) * 1.5 + 0.3, rng.standard_normal(B)
    gm, gs = BG.logpdf_grads(z, w, mean, scale, dense)
    fm, fs, quad, logdet = BG.formulas(z, w, mean, scale, dense)
    assert np.abs(gm - fm).max() <= 1e-12 * BG.V.scale(fm)
    assert np.abs(gs - fs).max() <= 1e-12 * max(np.abs(quad).max(), np.abs(logdet).max())
    assert np.array_equal(quad + logdet, fs)
    if dense:
        assert not np.triu(gs, 1).any()
    # the pullback of the draw, and the cancellation the issue states: fixed-z0 partial + pullback of the draw
    # = sum_b lam_b n_b' - (sum w) diag(1 / L), with g_b = lam_b + w_b d logpdf / d z0 and n_b the normals themselves
    nrm, lam = rng.standard_normal((n, B)), rng.standard_normal((n, B))
    z0 = BG.drawn_z0(nrm, mean, scale, dense)
    g = lam - w[None, :] * BG.gauss(mean, scale, dense).neg_grad(z0)
    pm, ps = BG.sample_pullback(nrm, g, dense)
    fm0, fs0, _, logdet0 = BG.formulas(z0, w, mean, scale, dense)
    lm, ls = BG.sample_pullback(nrm, lam, dense)
    assert np.abs(fm0 + pm - lm).max() <= 1e-12 * BG.V.scale(lm)
    assert np.abs(fs0 + ps - (ls + logdet0)).max() <= 1e-12 * (BG.V.scale(ls) + np.abs(fs0).max())


@pytest.mark.parametrize("name", SMALL)
def test_density_direction_against_central_differences(name):
    case, dense, train, cfg, (flat, xs, eps, ys), mean, scale, _, rng = BG.case_setup(name)
    dts = R.fixed_dts(case)
    w = BG.cotangents_w(rng, case.B)[1].astype(np.float64)
    gm, gs = BG.density(cfg, flat, xs, eps, w, dts, mean, scale, dense, ys, train)
    z = BG.final_state(cfg, flat, xs, eps, dts, ys, train)

    def S(m, s):          # sum_b w_b logpx_b up to what does not depend on the base
        return float(np.sum(w * BG.gauss(m, s, dense).logpdf(z)))

    m0, s0 = np.asarray(mean, np.float64), np.asarray(scale, np.float64)
    h = 1e-6
    n_in = m0.size
    for i in (0, n_in // 2, n_in - 1):
        e = np.zeros_like(m0); e[i] = h
        num = (S(m0 + e, s0) - S(m0 - e, s0)) / (2 * h)
        assert abs(num - gm[i]) <= 1e-6 * max(abs(num), BG.V.scale(gm)), (name, "mean", i, num, gm[i])
    entries = [(0,), (n_in - 1,)] if not dense else [(0, 0), (n_in - 1, 0), (n_in - 1, n_in - 1), (n_in // 2, n_in // 2 - 1)]
    for idx in entries:
        e = np.zeros_like(s0); e[idx] = h
        num = (S(m0, s0 + e) - S(m0, s0 - e)) / (2 * h)
        assert abs(num - gs[idx]) <= 1e-6 * max(abs(num), BG.V.scale(gs)), (name, "scale", idx, num, gs[idx])


@pytest.mark.parametrize("name", ["n3-diag-B17", "n16-dense-cond-B17"])
def test_drawn_sampling_against_central_differences(name):
    """The total derivative through z0 = mean + L n: finite differences of sum <cot, (z, logq)> with the base moved AND z0
    redrawn from the same normals."""
    case, dense, train, cfg, (flat, _, eps, ys), mean, scale, nrm, rng = BG.case_setup(name)
    dts = R.fixed_dts(case)
    cz, cl = R.cotangents(rng, cfg.n_in, case.nvars, case.B)["both"]
    gm, gs, _ = BG.sampling_drawn(cfg, flat, nrm, eps, cz, cl, dts, mean, scale, dense, ys, train)
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)

    def S(m, s):
        z, logq, _, _ = R.forward(cfg, f64(flat), BG.drawn_z0(nrm, m, s, dense), f64(eps), dts, f64(ys), train, BG.gauss(m, s, dense))
        return float(np.sum(f64(cz) * z[:case.nvars]) + np.sum(f64(cl) * logq))

    m0, s0 = f64(mean), f64(scale)
    h = 1e-6
    n_in = m0.size
    for i in (0, n_in - 1):
        e = np.zeros_like(m0); e[i] = h
        num = (S(m0 + e, s0) - S(m0 - e, s0)) / (2 * h)
        assert abs(num - gm[i]) <= 1e-5 * max(abs(num), BG.V.scale(gm)), (name, "mean", i, num, gm[i])
    for idx in ([(0,), (n_in - 1,)] if not dense else [(0, 0), (n_in - 1, 1), (n_in - 1, n_in - 1)]):
        e = np.zeros_like(s0); e[idx] = h
        num = (S(m0, s0 + e) - S(m0, s0 - e)) / (2 * h)
        assert abs(num - gs[idx]) <= 1e-5 * max(abs(num), BG.V.scale(gs)), (name, "scale", idx, num, gs[idx])


def test_identity_flow_reverse_kl_closed_form():
    """A zero last layer makes the flow the identity: xs = z0 = mu + sigma n, dlogp = 0, and the reverse KL to N(m, s^2) has
    the per-sample gradients (mu + sigma n - m) / s^2 and -1 / sigma + n (mu + sigma n - m) / s^2."""
    from oracle import cnf_oracle as O
    from tests import grad_terms as GT
    net = O.Net((3, 8, 3), (O.ACT_TANH, O.ACT_IDENTITY))
    cfg = O.Cfg(net, 3, 0, 0.0, 0.0, 0.0, tspan=(0.0, 1.0))
    rng = np.random.default_rng(8)
    flat = GT.zero_last_layer(net, O.glorot_params(net, rng, np.float64, 0.3))
    B = 9
    mu, sig = rng.standard_normal(3), rng.uniform(0.5, 1.5, 3)
    m, s = rng.standard_normal(3), rng.uniform(0.5, 2.0, 3)
    nrm, eps = rng.standard_normal((3, B)), rng.standard_normal((3, B))
    dts = [0.5, 0.5]
    z0 = BG.drawn_z0(nrm, mu, sig, False)
    z, logq, _, _ = R.forward(cfg, flat, z0, eps, dts, None, True, BG.gauss(mu, sig, False))
    assert np.abs(z - z0).max() <= 1e-14
    # loss = mean(logq + 1/2 ((x - m) / s)^2): cot_x = (x - m) / s^2 / B, cot_logq = 1 / B
    cz, cl = (z - m[:, None]) / s[:, None] ** 2 / B, np.full(B, 1.0 / B)
    gm, gs, _ = BG.sampling_drawn(cfg, flat, nrm, eps, cz, cl, dts, mu, sig, False)
    r = (mu[:, None] + sig[:, None] * nrm - m[:, None]) / s[:, None] ** 2
    assert np.abs(gm - r.mean(1)).max() <= 1e-12
    assert np.abs(gs - (-1.0 / sig + (nrm * r).mean(1))).max() <= 1e-12


# ---- the float32 floor of every device case: it must leave the bar of the device tests in force ----
@pytest.mark.parametrize("name", list(BG.CASES))
def test_float32_floor_density_and_fixed_z0(name):
    for i, (r64, r32, summ, _) in enumerate(_density_refs(name)):
        BG.assert_floor(r64, r32, summ, f"{name} density cot {i}")
    case, dense, train, cfg, _, mean, scale, nrm, rng = BG.case_setup(name)
    w = BG.cotangents_w(rng, case.B)[0]
    z0 = BG.drawn_z0(nrm, mean, scale, dense, np.float32)
    r64 = BG.logpdf_grads(z0, w, mean, scale, dense, np.float64)
    r32 = BG.logpdf_grads(z0, w, mean, scale, dense, np.float32)
    BG.assert_floor(r64, r32, BG.summands_of(r64[1], np.sum(w, dtype=np.float64), scale, dense), f"{name} fixed z0")


@pytest.mark.parametrize("name", ["n3-dense-B300", "n16-dense-cond-B17", "n17-diag-B1", "n33-dense-B17-test", "headline-dense-B33"])
def test_float32_floor_drawn_sampling(name):
    case, dense, train, cfg, (flat, _, eps, ys), mean, scale, nrm, rng = BG.case_setup(name)
    dts = R.fixed_dts(case)
    cz, cl = R.cotangents(rng, cfg.n_in, case.nvars, case.B)["both"]
    a = (cfg, flat, nrm, eps if train else None, cz, cl, dts, mean, scale, dense, ys, train)
    r64, r32 = BG.sampling_drawn(*a, dtype=np.float64), BG.sampling_drawn(*a, dtype=np.float32)
    BG.assert_floor(r64[:2], r32[:2], BG.summands_of(r64[1], np.sum(cl, dtype=np.float64), scale, dense), f"{name} drawn z0")


# ---- the C ABI: the new header and table; the pinned ones untouched ----
def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", txt)))


def test_new_entry_points_are_declared_exported_and_bound():
    names = _declared("cnfhip_basegrad.h")
    assert names == ["cnf_base_logpdf_pullback", "cnf_base_sample_pullback"]
    assert set(names) == set(_lib.BASEGRAD_EXPORTS)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(l, n), f"{n} declared but not exported"
    bound = _lib.lib()
    for n in names:
        assert getattr(bound, n).argtypes is not None and getattr(bound, n).restype is ctypes.c_int
    assert not set(names) & set(_lib.EXPORTS) and not set(names) & set(_lib.SAMPLING_EXPORTS)
    assert len(_lib.EXPORTS) == 62 and len(_lib.SAMPLING_EXPORTS) == 2
    assert '#include "cnfhip_basegrad.h"' in open(os.path.join(ROOT, "include", "cnfhip.h")).read()
    assert bound.cnf_abi_version() == 1
    assert bound.cnf_base_logpdf_pullback(None, None, 1, None, None, None) == _lib.ERR_BAD_ARG
    assert bound.cnf_base_sample_pullback(None, None, None, 1, None, None, None) == _lib.ERR_BAD_ARG


# ---- the Python surface without a device ----
def _tiny_model(basedist=None):
    nn = cnf.Chain(cnf.Dense(3, 6, "tanh"), cnf.Dense(6, 3, "tanh"))
    return cnf.construct(cnf.RNODE, nn, 2, 1, basedist=basedist)


def test_learnable_normal_validates_like_mvnormal():
    t = lambda *a: torch.tensor(a, dtype=torch.float32)
    d = cnf.LearnableNormal(t(0.0, 1.0, 2.0), std=t(1.0, 2.0, 0.5))
    assert len(d) == 3 and d.kind == 1 and np.allclose(d.whiten, [1.0, 0.5, 2.0]) and np.array_equal(d.chol, [1.0, 2.0, 0.5])
    ref = cnf.DiagNormal([0.0, 1.0, 2.0], [1.0, 2.0, 0.5])
    assert d.logconst == ref.logconst and np.array_equal(d.whiten, ref.whiten)
    L = torch.tensor([[1.0, 5.0, 5.0], [0.5, 2.0, 5.0], [0.1, -0.3, 0.7]])
    dd = cnf.LearnableNormal(t(0.0, 0.0, 0.0), scale_tril=L)
    mv = cnf.MvNormal(np.zeros(3), np.tril(L.numpy()).astype(np.float64) @ np.tril(L.numpy()).astype(np.float64).T)
    assert dd.kind == 2 and np.allclose(dd.chol, np.tril(L.numpy())) and np.allclose(dd.whiten, mv.whiten, atol=1e-6)
    assert abs(dd.logconst - mv.logconst) <= 1e-6
    for bad in (dict(), dict(scale_tril=L, std=t(1.0, 1.0, 1.0))):
        with pytest.raises(ValueError, match="exactly one"):
            cnf.LearnableNormal(t(0.0, 0.0, 0.0), **bad)
    with pytest.raises(ValueError, match="> 0"):
        cnf.LearnableNormal(t(0.0, 0.0, 0.0), std=t(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="> 0"):
        cnf.LearnableNormal(t(0.0, 0.0, 0.0), scale_tril=torch.diag(t(1.0, -1.0, 1.0)))
    with pytest.raises(ValueError, match="finite"):
        cnf.LearnableNormal(t(0.0, float("nan"), 0.0), std=t(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="finite"):
        cnf.LearnableNormal(t(0.0, 0.0, 0.0), std=t(1.0, float("inf"), 1.0))
    with pytest.raises(ValueError, match="torch tensor"):
        cnf.LearnableNormal([0.0, 0.0, 0.0], std=t(1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        cnf.LearnableNormal(t(0.0, 0.0, 0.0), std=t(1.0, 1.0))
    with pytest.raises(ValueError):
        _tiny_model(cnf.LearnableNormal(t(0.0, 0.0), std=t(1.0, 1.0)))          # length 2 on a model of 3 rows
    assert isinstance(_tiny_model(d).basedist, cnf.LearnableNormal)


def test_refresh_follows_identity_and_version():
    """The rule of ``set_cond``: reduced again only when a tensor's identity or in-place version changed."""
    mean = torch.zeros(3)
    log_std = torch.zeros(3, requires_grad=True)
    d = cnf.LearnableNormal(mean, std=log_std.exp())
    assert d.requires_grad and not d.refresh()
    with torch.no_grad():
        mean.add_(1.0)
    assert d.refresh() and np.array_equal(d.mean, [1.0, 1.0, 1.0]) and not d.refresh()
    d.update(mean, std=(log_std + 1.0).exp())
    assert np.allclose(d.chol, np.e) and not d.refresh()
    with torch.no_grad():
        mean[0] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        d.refresh()


@pytest.mark.parametrize("basedist", [None, "mv"], ids=["default", "MvNormal"])
def test_with_base_needs_a_learnable_base(basedist):
    """``with_base=True`` on a constant base: ValueError before anything touches a device."""
    icnf = _tiny_model(cnf.MvNormal(np.zeros(3), 2.0) if basedist else None)
    xs, ps = np.zeros((2, 4), np.float32), np.zeros(icnf.nn.n_params_internal, np.float32)
    cot = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError, match="LearnableNormal"):
        cnf.inference_pullback(icnf, cot, with_base=True)
    with pytest.raises(ValueError, match="LearnableNormal"):
        cnf.generate_pullback(icnf, (None, np.zeros(4, np.float32)), with_base=True)
    for mode in (cnf.TrainMode(), cnf.TestMode()):
        with pytest.raises(ValueError, match="LearnableNormal"):
            cnf.loss_and_grad(icnf, mode, xs, ps, {}, with_base=True)
    assert icnf._handle is None


def test_with_base_of_loss_and_grad_needs_device_tensors():
    d = cnf.LearnableNormal(torch.zeros(3), std=torch.ones(3))
    icnf = _tiny_model(d)
    with pytest.raises(ValueError, match="device tensors"):
        cnf.loss_and_grad(icnf, cnf.TrainMode(), np.zeros((2, 4), np.float32), np.zeros(icnf.nn.n_params_internal, np.float32), {},
                          with_base=True)
    assert icnf._handle is None


def test_model_uploads_when_and_only_when_the_values_changed():
    """``ICNF.set_basedist`` (run by every call that solves): an upload after an in-place change, after ``update`` with
    recomputed tensors and after another ``LearnableNormal`` was assigned -- none otherwise.  The upload itself is stubbed."""
    mean, log_std = torch.zeros(3), torch.zeros(3, requires_grad=True)
    d = cnf.LearnableNormal(mean, std=log_std.exp())
    icnf = _tiny_model(d)
    calls = []
    icnf._handle = object()                                   # (no device here: the handle is never used by the stub)
    icnf._upload_basedist = lambda: (calls.append(icnf.basedist.mean.copy()), setattr(icnf, "_base_id", (icnf.basedist, icnf.basedist.generation)))
    try:
        icnf.set_basedist()
        icnf.set_basedist()
        assert len(calls) == 1
        with torch.no_grad():
            mean.add_(2.0)
        icnf.set_basedist()
        assert len(calls) == 2 and np.array_equal(calls[-1], [2.0, 2.0, 2.0])
        d.update(mean + 1.0, std=log_std.exp())               # new tensors, reduced by update itself: still to be uploaded
        icnf.set_basedist()
        icnf.set_basedist()
        assert len(calls) == 3 and np.array_equal(calls[-1], [3.0, 3.0, 3.0])
        icnf.basedist = cnf.LearnableNormal(mean, std=log_std.exp())
        icnf.set_basedist()
        assert len(calls) == 4 and np.array_equal(calls[-1], [2.0, 2.0, 2.0])
        icnf.basedist = cnf.LearnableNormal(torch.zeros(2), std=torch.ones(2))
        with pytest.raises(ValueError, match="length"):
            icnf.set_basedist()
    finally:
        icnf._handle = None


def test_buffer_layout_keeps_tickets_apart_for_both_kinds(tmp_path):
    """cnf_basegrad_plan.h on the CPU (tests/support/basegrad_plan_test.cpp): no ticket word of either kind of base ever lies
    where the other kind writes -- the handle's buffer is cleared only when it grows, and the kind may change on a live handle."""
    import subprocess
    exe = str(tmp_path / "basegrad_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "continuousnf.jl_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "support", "basegrad_plan_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr


def test_a_displaced_record_is_not_made_again_with_another_base():
    """What ``record_again`` of both autograd functions checks first: the base's values are not among the saved inputs."""
    from continuousnf.jl_amd.vjp import _base_key, _base_unchanged
    mean = torch.zeros(3)
    d = cnf.LearnableNormal(mean, std=torch.ones(3))
    icnf = _tiny_model(d)
    key = _base_key(icnf)
    _base_unchanged(icnf, key)
    with torch.no_grad():
        mean.add_(1.0)
    with pytest.raises(RuntimeError, match="changed between forward and backward"):
        _base_unchanged(icnf, key)
    key = _base_key(icnf)
    icnf.basedist = cnf.LearnableNormal(mean, std=torch.ones(3))
    with pytest.raises(RuntimeError):
        _base_unchanged(icnf, key)
    plain = _tiny_model(None)
    assert _base_key(plain) is None
    _base_unchanged(plain, None)
