"""Heterogeneous ensembles without a device: the two entry points of include/cnfhip_ensemble_hetero.h are declared, exported and
bound (the rule of tests/test_gen_vjp_ref_host.py: a header and a binding table of their own, none of the pinned lists grows);
every argument error of the new keywords is raised before anything is drawn -- generator state unchanged, no handle made --;
and the pure helpers (padding, the batches of ``fit_many``, the per-member loss from sums with its own lambdas and count) agree
with numpy."""
import ctypes
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from continuousnf.jl_amd import ensemble as E

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cnf_ensemble_clear_members", "cnf_ensemble_set_members"]
KEYWORDS = ("counts", "reltol", "abstol")


def _model(dims=(2, 6, 2), nvars=1, naugs=1, **kw):
    layers = [cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])]
    return cnf.construct(cnf.RNODE, cnf.Chain(*layers), nvars, naugs, rng=5, **kw)


def test_entry_points_are_declared_exported_and_bound():
    """Fails without the feature."""
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_ensemble_hetero.h"', main, flags=re.M), "cnfhip.h does not include cnfhip_ensemble_hetero.h"
    raw = open(os.path.join(ROOT, "include", "cnfhip_ensemble_hetero.h")).read()
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", strip(raw))))
    assert declared == NAMES, declared
    assert set(declared) == set(_lib.ENSEMBLE_HETERO_EXPORTS)
    for other in (_lib.EXPORTS, _lib.SAMPLING_EXPORTS, _lib.BASEGRAD_EXPORTS, _lib.ENSEMBLE_EXPORTS, _lib.ENSEMBLE_EVAL_EXPORTS,
                  _lib.ENSEMBLE_VJP_EXPORTS, _lib.ENSEMBLE_GENERATE_VJP_EXPORTS, _lib.PATH_EXPORTS, _lib.PATH_VJP_EXPORTS):
        assert not set(declared) & set(other)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    # each entry point cites the reference lines it replaces: construct's lambdas and sol_kwargs
    for name in NAMES:
        comment = re.findall(r"/\*(?:(?!\*/).)*?\*/\s*cnf_status\s+" + name, raw, flags=re.S)
        assert comment and "src/base_icnf.jl:26-38" in comment[-1], name
    # no signature of the other ensemble headers changed: the five calls take what they took
    for name, n_args in (("cnf_loss_grad_many", 14), ("cnf_inference_many", 16), ("cnf_generate_many", 15),
                         ("cnf_inference_vjp_many", 17), ("cnf_generate_vjp_many", 18)):
        assert len(getattr(_lib.lib(), name).argtypes) == n_args, name


def test_the_python_keywords_exist():
    """Fails without the feature."""
    import inspect
    for name in ("inference_many", "loss_many", "generate_many", "inference_vjp_many", "generate_vjp_many",
                 "differentiable_inference_many", "differentiable_generate_many", "reverse_kl_many", "loss_and_grad_many"):
        sig = inspect.signature(getattr(cnf, name)).parameters
        for k in KEYWORDS:
            assert k in sig and sig[k].default is None, (name, k)
    for name in ("loss_and_grad_many", "loss_many", "fit_many"):
        sig = inspect.signature(getattr(cnf, name)).parameters
        assert "lambdas" in sig and sig["lambdas"].default is None, name
    for k in ("reltol", "abstol"):
        assert k in inspect.signature(cnf.fit_many).parameters
    assert inspect.signature(cnf.EnsembleDist.rand).parameters["ragged"].default is False


def test_the_c_calls_check_their_arguments_before_any_device():
    l = _lib.lib()
    c = np.ones(3, dtype=np.int32)
    assert l.cnf_ensemble_set_members(None, 3, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, None) == _lib.ERR_BAD_ARG
    assert l.cnf_ensemble_clear_members(None) == _lib.ERR_BAD_ARG


def _unchanged(icnf, before):
    assert icnf.rng.bit_generator.state == before and icnf._handle is None


def test_argument_errors_come_before_anything_is_drawn():
    """Wrong lengths, a count of 0 or above B, a zero lambda against a non-zero one (and the reverse), a non-positive or
    non-finite tolerance: ``ValueError`` from every call that takes the keyword, with the generator where it was and no handle."""
    icnf = _model(lambda1=1e-2, lambda2=1e-2, lambda3=0.0)
    n, M, B = icnf.nn.n_params_internal, 3, 8
    xs, ps = torch.zeros(M, 1, B), torch.zeros(M, n)
    T = cnf.TrainMode()
    cot = (torch.zeros(M, B), None)
    bad_common = [
        dict(counts=[8, 8]), dict(counts=[8, 8, 8, 8]), dict(counts=[8, 0, 8]), dict(counts=[8, 9, 8]), dict(counts=[8, -1, 8]),
        dict(counts=[8.0, 4.0, 2.0]), dict(counts=[[8, 4, 2]]),
        dict(reltol=[1e-3, 1e-3]), dict(reltol=0.0), dict(reltol=[1e-3, -1e-3, 1e-3]), dict(reltol=float("nan")),
        dict(abstol=[1e-6] * 4), dict(abstol=0.0), dict(abstol=[1e-6, float("inf"), 1e-6]),
    ]
    bad_lams = [
        dict(lambdas=np.ones((2, 3))), dict(lambdas=np.ones((3, 2))), dict(lambdas=np.ones(3)),
        dict(lambdas=[[1, 1, 1]] * 3),                          # a non-zero lambda_3 where the model's is zero
        dict(lambdas=[[1, 1, 0], [0, 1, 0], [1, 1, 0]]),        # a zero lambda_1 where the model's is not
        dict(lambdas=[[1, 1, 0], [1, float("nan"), 0], [1, 1, 0]]),
    ]
    before = icnf.rng.bit_generator.state
    calls = {
        "loss_and_grad_many": lambda kw: cnf.loss_and_grad_many(icnf, T, xs, ps, {}, **kw),
        "inference_many": lambda kw: cnf.inference_many(icnf, T, xs, ps, {}, **kw),
        "loss_many": lambda kw: cnf.loss_many(icnf, T, xs, ps, {}, **kw),
        "generate_many": lambda kw: cnf.generate_many(icnf, T, ps, {}, B, **kw),
        "inference_vjp_many": lambda kw: cnf.inference_vjp_many(icnf, T, xs, ps, {}, cot, **kw),
        "generate_vjp_many": lambda kw: cnf.generate_vjp_many(icnf, T, ps, {}, B, (None, torch.zeros(M, B)), **kw),
        "differentiable_inference_many": lambda kw: cnf.differentiable_inference_many(icnf, T, xs, ps, {}, **kw),
        "differentiable_generate_many": lambda kw: cnf.differentiable_generate_many(icnf, T, ps, {}, B, **kw),
        "reverse_kl_many": lambda kw: cnf.reverse_kl_many(icnf, T, ps, {}, B, lambda x: x[:, 0], **kw),
    }
    for name, call in calls.items():
        for kw in bad_common + (bad_lams if name in ("loss_and_grad_many", "loss_many") else []):
            with pytest.raises(ValueError):
                call(kw)
            _unchanged(icnf, before)
    # the good ones pass the checks (host logic only) ...
    het = E._members(icnf, M, B, counts=[8, 3, 1], lambdas=[[1, 2, 0], [3, 4, 0], [5, 6, 0]], reltol=[1e-2, 1e-3, 1e-4], abstol=1e-7)
    assert het.counts.dtype == np.int32 and het.counts.tolist() == [8, 3, 1]
    assert het.lambdas.dtype == np.float32 and het.lambdas.shape == (3, 3)
    assert np.array_equal(het.tols, np.asarray([[1e-7, 1e-2], [1e-7, 1e-3], [1e-7, 1e-4]], dtype=np.float32))
    # ... one tolerance given: the other is the model's; none given: the call is the old one
    m2 = _model(sol_kwargs=dict(abstol=1e-5, reltol=1e-2))
    assert np.array_equal(E._members(m2, 2, 4, reltol=1e-4).tols, np.asarray([[1e-5, 1e-4]] * 2, dtype=np.float32))
    assert np.array_equal(E._members(m2, 2, 4, abstol=[1e-8, 1e-9]).tols, np.asarray([[1e-8, 1e-2], [1e-9, 1e-2]], dtype=np.float32))
    assert E._members(icnf, M, B) is None
    used = E._members_used(m2, None, 2, 4)
    assert used["counts"].tolist() == [4, 4] and np.array_equal(used["tols"], np.asarray([[1e-5, 1e-2]] * 2, dtype=np.float32))
    assert np.array_equal(used["lambdas"], np.asarray([[m2.lambda1, m2.lambda2, m2.lambda3]] * 2, dtype=np.float32))
    _unchanged(icnf, before)


def test_fit_many_refuses_unequal_batch_counts_before_anything_is_drawn():
    icnf = _model()
    model = cnf.ICNFModel(icnf, optimizers=(cnf.Adam(eta=1e-2),), n_epochs=1, batch_size=32)
    before = icnf.rng.bit_generator.state
    Xs = [np.zeros((n, 1), dtype=np.float32) for n in (64, 65)]              # two batches against three
    with pytest.raises(ValueError, match="same number of batches"):
        cnf.fit_many(model, 0, Xs)
    _unchanged(icnf, before)
    with pytest.raises(ValueError):                                           # a sweep of the wrong length
        cnf.fit_many(model, 0, [np.zeros((64, 1), dtype=np.float32)] * 2, lambdas=np.full((3, 3), 1e-2))
    _unchanged(icnf, before)
    with pytest.raises(ValueError):
        cnf.fit_many(model, 0, [np.zeros((64, 1), dtype=np.float32)] * 2, reltol=-1.0)
    _unchanged(icnf, before)
    # the batches of an epoch
    got = E._fit_batches([64, 63, 62], True, 32)
    assert [lo for lo, _ in got] == [0, 32] and got[0][1].tolist() == [32, 32, 32] and got[1][1].tolist() == [32, 31, 30]
    got = E._fit_batches([64, 33], True, 32)
    assert got[1][1].tolist() == [32, 1]
    got = E._fit_batches([10, 7], False, 32)                                  # no batching: one call, every member's whole set
    assert len(got) == 1 and got[0][0] == 0 and got[0][1].tolist() == [10, 7]
    for ns in ([64, 32], [33, 32], [1, 64]):
        with pytest.raises(ValueError):
            E._fit_batches(ns, True, 32)
    with pytest.raises(ValueError):
        E._fit_batches([4, 0], True, 32)


def test_padding_against_numpy():
    rng = np.random.default_rng(0)
    counts = [5, 1, 3]
    parts = [rng.standard_normal((2, c)).astype(np.float32) for c in counts]
    for fill in (0.0, float("nan")):
        out = cnf.pad_columns(parts, 5, fill)
        tout = cnf.pad_columns([torch.from_numpy(p) for p in parts], 5, fill).numpy()
        assert out.shape == (3, 2, 5) and out.dtype == np.float32
        for m, c in enumerate(counts):
            assert np.array_equal(out[m, :, :c], parts[m]) and np.array_equal(tout[m, :, :c], parts[m])
            pad = out[m, :, c:]
            assert (np.isnan(pad).all() if np.isnan(fill) else (pad == 0).all()) and np.array_equal(pad, tout[m, :, c:], equal_nan=True)
    with pytest.raises(ValueError):
        cnf.pad_columns(parts, 4)


def test_member_loss_from_sums_against_numpy():
    """A member's loss is the mean over ITS count with ITS lambdas: float64 arithmetic on the float32 sums, rounded once."""
    rng = np.random.default_rng(1)
    for _ in range(20):
        cnt = int(rng.integers(1, 41))
        lp, e, n, a = (rng.standard_normal(cnt).astype(np.float32) for _ in range(4))
        lam = rng.uniform(0.01, 1.0, 3).astype(np.float32)
        sums = np.asarray([lp.sum(), e.sum(), n.sum(), a.sum(), cnt], dtype=np.float32)
        s64 = sums.astype(np.float64)
        want = np.float32((-s64[0] + float(lam[0]) * s64[1] + float(lam[1]) * s64[2] + float(lam[2]) * s64[3]) / cnt)
        got = cnf.member_loss_from_sums(cnf.TrainMode(), sums, lam)
        assert got == want and got.dtype == np.float32
        # ... and it is the mean of the per-sample losses within float32 rounding of the sums
        per = -lp.astype(np.float64) + lam[0] * e.astype(np.float64) + lam[1] * n.astype(np.float64) + lam[2] * a.astype(np.float64)
        assert abs(float(got) - per.mean()) <= 1e-5 * max(1.0, np.abs(per).max())
        assert cnf.member_loss_from_sums(cnf.TestMode(), sums, lam) == np.float32(-s64[0] / cnt)
    with pytest.raises(ValueError):
        cnf.member_loss_from_sums(cnf.TrainMode(), np.zeros(5, dtype=np.float32), np.ones(3))


def test_member_twin_carries_the_members_own_options():
    icnf = _model(sol_kwargs=dict(abstol=1e-5, reltol=1e-2, maxiters=500), tspan=(0.0, 2.0))
    twin = cnf.member_twin(icnf, lambdas=(0.3, 0.01, 0.02), tols=(1e-7, 1e-4))
    assert twin is not icnf and twin._handle is None and icnf._handle is None
    assert (twin.lambda1, twin.lambda2, twin.lambda3) == tuple(float(np.float32(v)) for v in (0.3, 0.01, 0.02))
    assert twin.sol_kwargs == dict(abstol=float(np.float32(1e-7)), reltol=float(np.float32(1e-4)), maxiters=500)
    assert icnf.sol_kwargs == dict(abstol=1e-5, reltol=1e-2, maxiters=500)          # (the model's own are left alone)
    assert twin.tspan == icnf.tspan and twin.nn is icnf.nn and twin.rng is icnf.rng
    same = cnf.member_twin(icnf)
    assert (same.lambda1, same.lambda2, same.lambda3) == (icnf.lambda1, icnf.lambda2, icnf.lambda3) and same.sol_kwargs == icnf.sol_kwargs
