"""Ensembles with a base distribution per member without a device: the entry points of include/cnfhip_ensemble_base.h are
declared, exported and bound, and each cites the reference; ``EnsembleBases`` checks and slices; ``bases=`` is checked before any
handle is made; the float32 floor of every case of tests/test_gpu_ensemble_base.py leaves its bars in force (computed from the
float64 and float32 references, never from a device number); and a base of (0, I) turns the reference into the default's."""
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import base_grad_ref as BG
from tests import ensemble_base_ref as EB
from tests import ensemble_vjp_ref as R
from tests import vjp_ref as V
from tests.helpers import make_icnf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cnf_ensemble_base_capacity", "cnf_ensemble_base_logpdf_pullback", "cnf_ensemble_base_sample",
         "cnf_ensemble_base_sample_pullback", "cnf_ensemble_clear_bases", "cnf_ensemble_set_bases"]
M = EB.M


def test_entry_points_are_declared_exported_and_bound():
    """Fails without the feature."""
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_ensemble_base.h"', main, flags=re.M), "cnfhip.h does not include cnfhip_ensemble_base.h"
    raw = open(os.path.join(ROOT, "include", "cnfhip_ensemble_base.h")).read()
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", strip(raw))))
    assert declared == NAMES, declared
    assert set(declared) == set(_lib.ENSEMBLE_BASE_EXPORTS)
    for other in (_lib.EXPORTS, _lib.SAMPLING_EXPORTS, _lib.BASEGRAD_EXPORTS, _lib.ENSEMBLE_EXPORTS, _lib.ENSEMBLE_EVAL_EXPORTS,
                  _lib.ENSEMBLE_VJP_EXPORTS, _lib.ENSEMBLE_GENERATE_VJP_EXPORTS, _lib.PATH_EXPORTS, _lib.PATH_VJP_EXPORTS,
                  _lib.ENSEMBLE_HETERO_EXPORTS, _lib.ENSEMBLE_PATH_EXPORTS, _lib.JVP_EXPORTS):
        assert not set(declared) & set(other)
    l = _lib.lib()
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(l, name).argtypes is not None, f"{name} is not bound"
        comment = re.findall(r"/\*(?:(?!\*/).)*?\*/\s*(?:cnf_status|int)\s+" + name + r"\(", raw, flags=re.S)
        assert comment and "src/base_icnf.jl:" in comment[0], f"{name}: its comment does not cite the reference"
    assert cnf.EnsembleBases is cnf.ensemble_base.EnsembleBases


def test_the_c_calls_check_their_arguments_before_any_device():
    l = _lib.lib()
    assert l.cnf_ensemble_set_bases(None, 3, 1, 8, 8, None) == _lib.ERR_BAD_ARG
    assert l.cnf_ensemble_clear_bases(None) == _lib.ERR_BAD_ARG
    assert l.cnf_ensemble_base_capacity(None, _lib.MODE_TRAIN, 32, 0) == 0
    assert l.cnf_ensemble_base_sample(None, 3, 8, 16, 4, None) == _lib.ERR_BAD_ARG
    assert l.cnf_ensemble_base_logpdf_pullback(None, 3, 8, 4, 8, 8, None) == _lib.ERR_BAD_ARG
    assert l.cnf_ensemble_base_sample_pullback(None, 3, 1, 8, 8, 4, None, 8, 8, None) == _lib.ERR_BAD_ARG


def test_ensemble_bases_validation_and_slicing():
    """Fails without the feature."""
    rng = np.random.default_rng(0)
    mean = rng.standard_normal((M, 4))
    std = rng.uniform(0.5, 2.0, (M, 4))
    L = np.tril(rng.standard_normal((M, 4, 4)) * 0.2) + np.eye(4)
    d, f = cnf.EnsembleBases(mean, std=std), cnf.EnsembleBases(mean, scale_tril=L)
    assert (len(d), d.n_in, d.kind, len(f), f.n_in, f.kind) == (M, 4, 1, M, 4, 2) and not d.requires_grad
    for bad in (dict(), dict(std=std, scale_tril=L), dict(std=std[:2]), dict(std=std[:, :3]), dict(scale_tril=L[:, :3]),
                dict(std=std[0]), dict(std=np.array([["a"] * 4] * M)), dict(std=std.astype(complex))):
        with pytest.raises(ValueError):
            cnf.EnsembleBases(mean, **bad)
    with pytest.raises(ValueError):
        cnf.EnsembleBases(mean[0], std=std[0])
    neg = std.copy()
    neg[2, 1] = -0.5
    with pytest.raises(ValueError, match="member 2"):
        cnf.EnsembleBases(mean, std=neg)                                   # (a non-positive sigma: caught on the host)
    Lz = L.copy()
    Lz[1, 3, 3] = 0.0
    with pytest.raises(ValueError, match="member 1"):
        cnf.EnsembleBases(mean, scale_tril=Lz)
    for nf in (np.nan, np.inf):
        with pytest.raises(ValueError):
            cnf.EnsembleBases(np.where(np.arange(4) == 1, nf, mean), std=std)
    # bases[m]: the single model's distribution of member m
    b1, f2 = d[1], f[2]
    assert isinstance(b1, cnf.DiagNormal) and np.array_equal(b1.mean64, mean[1]) and np.array_equal(b1.chol64, std[1])
    assert isinstance(f2, cnf.MvNormal) and f2.kind == 2 and np.allclose(f2.chol64, L[2], rtol=1e-13, atol=1e-14)
    with pytest.raises(IndexError):
        d[M]
    # slices follow the members
    s = f[1:]
    assert len(s) == M - 1 and np.array_equal(s.mean, mean[1:]) and np.array_equal(s.scale, L[1:])
    t = d.take([2, 0])
    assert np.array_equal(t.mean, mean[[2, 0]]) and np.array_equal(t.scale, std[[2, 0]])
    # torch tensors are held, may require grad, and host values are checked again when they are read
    torch = pytest.importorskip("torch")
    log_std = torch.zeros((M, 4), requires_grad=True)
    tb = cnf.EnsembleBases(torch.zeros((M, 4)), std=log_std.exp())
    assert tb.requires_grad and tb.is_torch and len(tb[1:]) == M - 1
    with pytest.raises(ValueError):
        cnf.EnsembleBases(torch.zeros((M, 4), dtype=torch.int64), std=torch.ones((M, 4)))
    with pytest.raises(ValueError):
        cnf.EnsembleBases(torch.zeros((M, 4)), std=std)                    # (one numpy, one torch)


def test_bases_are_checked_before_any_handle_is_made():
    """Fails without the feature (``bases=`` is a TypeError there)."""
    torch = pytest.importorskip("torch")
    case = EB.BY_NAME["readme-vjp-B33"]
    icnf = make_icnf(cnf, case.cfg, kernel="mfma")
    n_in, B = case.cfg.n_in, 4
    xs, ps = torch.zeros((M, case.cfg.nvars, B)), torch.zeros((M, icnf.nn.n_params_internal))
    ok = cnf.EnsembleBases(np.zeros((M, n_in)), std=np.ones((M, n_in)))
    before = icnf.rng.bit_generator.state
    for bad in (cnf.EnsembleBases(np.zeros((M + 1, n_in)), std=np.ones((M + 1, n_in))),
                cnf.EnsembleBases(np.zeros((M, n_in + 1)), std=np.ones((M, n_in + 1))), "N(0, I)"):
        with pytest.raises(ValueError):
            cnf.inference_many(icnf, cnf.TrainMode(), xs, ps, bases=bad)
        with pytest.raises(ValueError):
            cnf.generate_many(icnf, cnf.TrainMode(), ps, None, B, bases=bad)
    for call in (lambda: cnf.loss_and_grad_many(icnf, cnf.TrainMode(), xs, ps, with_base=True),
                 lambda: cnf.inference_vjp_many(icnf, cnf.TrainMode(), xs, ps, None, (xs[:, 0], None), with_base=True)):
        with pytest.raises(ValueError):
            call()
    # the path calls take no bases: refused before anything is drawn
    for call in (lambda: cnf.inference_path_many(icnf, cnf.TrainMode(), xs, ps, saveat=[0.5], bases=ok),
                 lambda: cnf.generate_path_many(icnf, cnf.TrainMode(), ps, None, B, saveat=[0.5], bases=ok),
                 lambda: cnf.inference_path_vjp_many(icnf, cnf.TrainMode(), xs, ps, saveat=[0.5], bases=ok),
                 lambda: cnf.generate_path_vjp_many(icnf, cnf.TrainMode(), ps, None, B, saveat=[0.5], bases=ok),
                 lambda: cnf.differentiable_inference_path_many(icnf, cnf.TrainMode(), xs, ps, saveat=[0.5], bases=ok),
                 lambda: cnf.differentiable_generate_path_many(icnf, cnf.TrainMode(), ps, None, B, saveat=[0.5], bases=ok)):
        with pytest.raises(NotImplementedError, match="bases"):
            call()
    # a model with a base of its own is refused as before, with or without bases=
    own = make_icnf(cnf, case.cfg, kernel="mfma")
    own.basedist = cnf.DiagNormal(np.zeros(n_in), np.ones(n_in))
    with pytest.raises(NotImplementedError, match="basedist"):
        cnf.inference_many(own, cnf.TrainMode(), xs, ps, bases=ok)
    assert icnf.rng.bit_generator.state == before and icnf._handle is None and own._handle is None


def _loss_cot(case, m):
    return V.loss_cotangent(R.member_cfg(case, m), case.B, case.train).astype(np.float32)


@pytest.mark.parametrize("case,kind", EB.CASE_KINDS, ids=EB.IDS)
def test_float32_floor_of_every_gpu_case_leaves_the_bars_in_force(case, kind):
    """``vjp32`` against ``vjp64`` with the member's base, and ``base_grad_ref.density`` in float32 against float64, through the
    steps the float64 oracle's adaptive solve accepts: ``rtol = max(1e-4, 8 floor)`` stays at or under the cap 1e-3 with a factor
    2 to spare, on every parameter block, on grad_x and on (g_mean, g_scale)."""
    ps, xs, eps = R.inputs(case)
    mean, scale = EB.bases(case, kind)
    worst = worst_b = 0.0
    for m in range(M):
        dts, _ = R.host_steps(case, m, ps, xs, eps)
        g = EB.gauss(mean, scale, kind, m)
        for name, cot in (("all", R.cotangents(case, m)["all"]), ("loss", _loss_cot(case, m))):
            _, r64, r32 = EB.reference(case, m, ps, xs, eps, cot, dts, g)
            for block, _, floor, rtol, s, _ in V.report(r64[0], r64[1], r64, r32, case.cfg.net):
                worst = max(worst, floor)
                assert s > 0 and 2 * V.FLOOR_FACTOR * floor <= V.RTOL_CAP, (case.name, kind, m, name, block, floor, rtol)
            b64, b32, summands = EB.base_reference(case, m, ps, xs, eps, cot[0], dts, mean, scale, kind)
            for block, _, floor, rtol, s, _ in BG.assert_floor(b64, b32, summands, f"{case.name} {kind} member {m} cot {name}"):
                worst_b = max(worst_b, floor)
                assert 2 * BG.FLOOR_FACTOR * floor <= BG.RTOL_CAP, (case.name, kind, m, name, block, floor, rtol)
    print(f"{case.name} {kind}: worst float32 floor {worst:.2e} (parameters, grad_x), {worst_b:.2e} (g_mean, g_scale); cap "
          f"{V.RTOL_CAP / V.FLOOR_FACTOR:.3g}")


@pytest.mark.parametrize("case,kind", EB.CASE_KINDS, ids=EB.IDS)
def test_a_base_of_zero_and_identity_is_the_default(case, kind):
    """Member ``UNIT`` of every case has mean 0 and scale I exactly; the reference with that base is the default's."""
    ps, xs, eps = R.inputs(case)
    mean, scale = EB.bases(case, kind)
    m = EB.UNIT
    assert not mean[m].any() and np.array_equal(scale[m], np.eye(case.cfg.n_in) if kind == "dense" else np.ones(case.cfg.n_in))
    assert all(np.abs(mean[k]).max() > 0.1 for k in range(M) if k != m)
    dts, _ = R.host_steps(case, m, ps, xs, eps)
    cot = R.cotangents(case, m)["all"]
    out, (g, gx), _ = EB.reference(case, m, ps, xs, eps, cot, dts, EB.gauss(mean, scale, kind, m))
    out0, (g0, gx0), _ = EB.reference(case, m, ps, xs, eps, cot, dts, None)
    for a, b in ((out, out0), (g, g0), (gx, gx0)):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
