"""Ensemble inference and sampling without a device: the four entry points of include/cnfhip_ensemble_eval.h are declared,
exported and bound; the C calls say what is wrong with their arguments before they ask for a device; the Python argument checks
and refusals hold; the two pure functions of ``EnsembleDist`` (mixture log-density, count split) are right; and every case of
tests/test_gpu_ensemble_eval.py clears the float32 floor with 4x to spare."""
import ctypes
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import ensemble_eval_ref as R
from tests.helpers import parity_err

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cnf_ensemble_eval_capacity", "cnf_ensemble_eval_steps", "cnf_generate_many", "cnf_inference_many"]


def _model(dims=(2, 6, 2), nvars=1, naugs=1, **kw):
    layers = [cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])]
    return cnf.construct(cnf.RNODE, cnf.Chain(*layers), nvars, naugs, rng=5, **kw)


def test_entry_points_are_declared_exported_and_bound():
    """Fails without the feature."""
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_ensemble_eval.h"', main, flags=re.M)
    txt = strip(open(os.path.join(ROOT, "include", "cnfhip_ensemble_eval.h")).read())
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", txt)))
    assert declared == NAMES, declared
    assert set(declared) == set(_lib.ENSEMBLE_EVAL_EXPORTS)
    for other in (_lib.EXPORTS, _lib.SAMPLING_EXPORTS, _lib.BASEGRAD_EXPORTS, _lib.ENSEMBLE_EXPORTS):
        assert not set(declared) & set(other)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    for name in ("ensemble_eval_capacity", "inference_many", "loss_many", "generate_many", "EnsembleDist", "ensemble_eval_steps",
                 "logpdf_members"):
        assert callable(getattr(cnf, name, None)), name
    for name in ("mixture_logpdf", "split_counts"):           # the two pure functions: importable without a device
        assert callable(getattr(cnf.ensemble, name, None)), name


def test_the_c_calls_check_their_arguments_before_any_device():
    """With no handle at all (none can exist without a device) every complaint about the arguments still comes first."""
    l = _lib.lib()
    buf = np.zeros(64, dtype=np.float32)
    st = np.zeros(4, dtype=np.int32)
    p = buf.ctypes.data
    opts = _lib.cnf_solve_opts(0.0, 1.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)
    inf = lambda M=2, B=16, params=p, xs=p, eps=p, o=ctypes.byref(opts), logpx=p, regs=p, status=st.ctypes.data, mode=_lib.MODE_TRAIN, \
        tc=0: l.cnf_inference_many(None, mode, M, params, xs, eps, B, o, None, logpx, regs, None, status, None, tc, None)
    gen = lambda M=2, B=16, params=p, z0=p, eps=p, o=ctypes.byref(opts), xs=p, status=st.ctypes.data, mode=_lib.MODE_TRAIN, tc=0: \
        l.cnf_generate_many(None, mode, M, params, z0, eps, B, o, None, xs, None, status, None, tc, None)
    for call, names in ((inf, ("params", "xs", "eps", "o", "logpx", "regs", "status")), (gen, ("params", "z0", "eps", "o", "xs", "status"))):
        assert call(M=0) == _lib.ERR_BAD_SHAPE and call(M=-3) == _lib.ERR_BAD_SHAPE
        assert call(B=0) == _lib.ERR_BAD_SHAPE
        for name in names:
            assert call(**{name: None}) == _lib.ERR_BAD_ARG, name
        assert call(mode=7) == _lib.ERR_BAD_ARG
        assert call(tc=-1) == _lib.ERR_BAD_ARG
        assert call(eps=None, mode=_lib.MODE_TEST) == _lib.ERR_BAD_ARG    # (TestMode takes no probes: only the handle is missing)
        assert call() == _lib.ERR_BAD_ARG
    assert l.cnf_ensemble_eval_capacity(None, _lib.MODE_TRAIN, 32) == 0
    assert l.cnf_ensemble_eval_steps(None, 0, None, 0) == -1


def test_python_argument_checks():
    icnf = _model()
    n = icnf.nn.n_params_internal
    xs, ps, eps = torch.zeros(3, 1, 8), torch.zeros(3, n), torch.zeros(3, 2, 8)
    T = cnf.TrainMode()
    bad = [
        dict(xs=torch.zeros(3, 2, 8)), dict(xs=torch.zeros(2, 8)), dict(xs=torch.zeros(3, 1, 0)), dict(xs=torch.zeros(8)),
        dict(ps=torch.zeros(2, n)), dict(ps=torch.zeros(3, n + 1)), dict(ps=torch.zeros(3 * n)),
        dict(eps=torch.zeros(3, 1, 8)), dict(eps=torch.zeros(3, 2, 7)), dict(eps=np.zeros((3, 2, 8), dtype=np.float32)),
        dict(t1=[1.0, 2.0]), dict(t1=[1.0, float("nan"), 1.0]), dict(t1=[1.0, 0.0, 1.0]),
    ]
    for kw in bad:
        a = dict(xs=xs, ps=ps, eps=eps, t1=None)
        a.update(kw)
        with pytest.raises(ValueError):
            cnf.inference_many(icnf, T, a["xs"], a["ps"], {}, eps=a["eps"], t1=a["t1"])
    with pytest.raises(ValueError):
        cnf.inference_many(icnf, cnf.TestMode(), xs, ps, {}, eps=eps)
    with pytest.raises(TypeError):
        cnf.inference_many(icnf, "train", xs, ps, {})
    with pytest.raises(NotImplementedError):                                # host arrays
        cnf.inference_many(icnf, T, xs.numpy(), ps.numpy(), {})
    z = torch.zeros(3, 2, 8)
    for kw in (dict(ps=torch.zeros(3, n + 1)), dict(ps=torch.zeros(n)), dict(n=0), dict(z0=torch.zeros(3, 1, 8)), dict(eps=torch.zeros(2, 2, 8)),
               dict(z0=np.zeros((3, 2, 8), dtype=np.float32)), dict(t0=[1.0]), dict(t0=[1.0, float("inf"), 1.0]), dict(t0=[1.0, 0.0, 1.0])):
        a = dict(ps=ps, n=8, z0=z, eps=z, t0=None)
        a.update(kw)
        with pytest.raises(ValueError):
            cnf.generate_many(icnf, T, a["ps"], {}, a["n"], z0=a["z0"], eps=a["eps"], t0=a["t0"])
    with pytest.raises(TypeError):
        cnf.generate_many(icnf, "train", ps, {}, 8)
    with pytest.raises(NotImplementedError):
        cnf.generate_many(icnf, T, ps.numpy(), {}, 8)
    for w in ([0.5, 0.5], [0.5, 0.6, 0.1], [1.5, -0.5, 0.0], [float("nan"), 0.5, 0.5]):
        with pytest.raises(ValueError):
            cnf.EnsembleDist(icnf, T, ps, {}, weights=w)
    d = cnf.EnsembleDist(icnf, T, ps, {})
    assert np.allclose(d.weights, 1 / 3) and len(d) == 1
    assert tuple(d.rand(0).shape) == (1, 0)                                 # nothing drawn, nothing launched
    with pytest.raises(ValueError):
        d.rand(-1)


def test_refusals_come_before_anything_is_drawn():
    lay = lambda dims: cnf.Chain(*[cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])])
    models = {
        "conditional": cnf.construct(cnf.CondRNODE, lay((4, 6, 2)), 1, 1, rng=5),
        "basedist": cnf.construct(cnf.RNODE, lay((2, 6, 2)), 1, 1, rng=5, basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2)),
        "generic": cnf.construct(cnf.RNODE, lay((2, 6, 2)), 1, 1, rng=5, compute_mode=cnf.HIPVecJacMatrixMode("generic")),
        "32-96-32": cnf.construct(cnf.RNODE, lay((32, 96, 32)), 32, 0, rng=5),
        "wide hidden layer": cnf.construct(cnf.RNODE, lay((2, 80, 2)), 1, 1, rng=5),
        "softplus": cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 6, "softplus"), cnf.Dense(6, 2, "softplus")), 1, 1, rng=5),
        "one layer": cnf.construct(cnf.RNODE, lay((2, 2)), 1, 1, rng=5),
        "planar": cnf.construct(cnf.Planar, cnf.Chain(cnf.PlanarLayer(2, "tanh")), 2, 0, rng=5),
    }
    for name, ic in models.items():
        before = ic.rng.bit_generator.state
        x, p = torch.zeros(2, ic.nvars, 16), torch.zeros(2, ic.nn.n_params_internal)
        for mode in (cnf.TrainMode(), cnf.TestMode()):
            with pytest.raises(NotImplementedError):
                cnf.inference_many(ic, mode, x, p, {})
            with pytest.raises(NotImplementedError):
                cnf.inference_many(ic, mode, x[0], p, {})
            with pytest.raises(NotImplementedError):
                cnf.loss_many(ic, mode, x, p, {})
            with pytest.raises(NotImplementedError):
                cnf.generate_many(ic, mode, p, {}, 16)
            with pytest.raises(NotImplementedError):
                cnf.EnsembleDist(ic, mode, p, {})
            assert cnf.ensemble_eval_capacity(ic, mode, 16) == 0, name
        assert ic.rng.bit_generator.state == before and ic._handle is None, name


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-device error needs a machine without one")
def test_no_device_is_the_handles_error():
    icnf = _model()
    with pytest.raises(cnf.CNFError) as e:
        icnf.handle()
    n = icnf.nn.n_params_internal
    with pytest.raises(cnf.CNFError) as e2:
        cnf.inference_many(icnf, cnf.TrainMode(), torch.zeros(2, 1, 8), torch.zeros(2, n), {})
    with pytest.raises(cnf.CNFError) as e3:
        cnf.generate_many(icnf, cnf.TrainMode(), torch.zeros(2, n), {}, 8)
    assert e3.value.status == e2.value.status == e.value.status == _lib.ERR_NO_DEVICE
    with pytest.raises(cnf.CNFError):
        cnf.ensemble_eval_capacity(icnf, cnf.TrainMode(), 32)


# ---- the two pure functions of EnsembleDist ----
def _lse64(logp, w):
    """float64 restatement of scipy.special.logsumexp(logp, axis=0, b=w[:, None])."""
    logp, w = np.asarray(logp, dtype=np.float64), np.asarray(w, dtype=np.float64)
    out = np.full(logp.shape[1], -np.inf)
    for j in range(logp.shape[1]):
        terms = [(lp, wi) for lp, wi in zip(logp[:, j], w) if wi > 0 and lp > -np.inf]
        if terms:
            mx = max(lp for lp, _ in terms)
            out[j] = mx + np.log(sum(wi * np.exp(lp - mx) for lp, wi in terms))
    return out


def _reference_lse(logp, w):
    try:
        from scipy.special import logsumexp
    except ImportError:
        return _lse64(logp, w)
    with np.errstate(divide="ignore"):
        ref = logsumexp(np.asarray(logp, dtype=np.float64), axis=0, b=np.asarray(w, dtype=np.float64)[:, None])
    assert np.allclose(ref, _lse64(logp, w), rtol=1e-12, atol=1e-12, equal_nan=True)
    return ref


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_mixture_logpdf(kind):
    rng = np.random.default_rng(4)
    M, n = 5, 40
    logp = (rng.standard_normal((M, n)) * 30 - 50)
    wrap = (lambda a: a) if kind == "numpy" else (lambda a: torch.from_numpy(np.ascontiguousarray(a)))
    back = (lambda a: a) if kind == "numpy" else (lambda a: a.numpy())
    w = rng.random(M)
    w /= w.sum()
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 2e-6)):
        lp = logp.astype(dtype)
        got = back(cnf.ensemble.mixture_logpdf(wrap(lp), w))
        assert got.dtype == dtype and got.shape == (n,)
        ref = _reference_lse(lp, w)
        assert np.all(np.abs(got - ref) <= tol * np.maximum(1.0, np.abs(ref)))
        # one-hot weights: that member's row, exactly
        e = np.zeros(M)
        e[3] = 1.0
        assert np.array_equal(back(cnf.ensemble.mixture_logpdf(wrap(lp), e)), lp[3])
        # a member at -inf contributes nothing; a column where every member is: -inf, not NaN
        hole = lp.copy()
        hole[1] = -np.inf
        hole[:, 7] = -np.inf
        got = back(cnf.ensemble.mixture_logpdf(wrap(hole), w))
        ref = _reference_lse(hole, w)
        assert got[7] == -np.inf and not np.isnan(got).any()
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(got)) and np.all(np.abs(got[fin] - ref[fin]) <= tol * np.maximum(1.0, np.abs(ref[fin])))
    # uniform weights: log mean exp
    u = back(cnf.ensemble.mixture_logpdf(wrap(logp), np.full(M, 1 / M)))
    assert np.allclose(u, _reference_lse(logp, np.full(M, 1 / M)), rtol=1e-12, atol=1e-12)


def test_split_counts():
    w = np.asarray([0.5, 0.0, 0.3, 0.2])
    a = cnf.ensemble.split_counts(np.random.default_rng(9), 1000, w)
    b = cnf.ensemble.split_counts(np.random.default_rng(9), 1000, w)
    assert a.dtype == np.int64 and a.shape == (4,) and a.sum() == 1000 and np.array_equal(a, b)
    assert a[1] == 0 and (a[[0, 2, 3]] > 100).all()
    assert np.array_equal(a, np.random.default_rng(9).multinomial(1000, w))          # ONE multinomial draw
    assert cnf.ensemble.split_counts(np.random.default_rng(1), 3, np.full(8, 1 / 8)).sum() == 3    # more members than draws: zeros
    assert cnf.ensemble.split_counts(np.random.default_rng(1), 7, [0, 1.0, 0]).tolist() == [0, 7, 0]
    with pytest.raises(ValueError):
        cnf.ensemble.split_counts(np.random.default_rng(1), 7, [0.7, 0.7])


# ---- the float32 floor of every GPU case ----
SPARE = 4.0


def _floor_inference(cfg, train, ps, xs, eps, sol_kw, what, t1=None):
    worst = 0.0
    for m in range(ps.shape[0]):
        c = cfg if t1 is None else R.cfg_of(cfg, (cfg.tspan[0], float(np.float32(t1[m]))), cfg.use_jvp)
        hs = R.oracle_steps(c, train, ps[m], xs[m], eps[m], sol_kw)
        assert abs(sum(hs) - (c.tspan[1] - c.tspan[0])) <= 1e-9
        r64, l64 = R.replay_inference(c, train, ps[m], xs[m], eps[m], hs, np.float64)
        r32, l32 = R.replay_inference(c, train, ps[m], xs[m], eps[m], hs, np.float32)
        e = max(parity_err(r32, r64, trace_row=0), parity_err(np.asarray([l32]), np.asarray([l64])))
        assert np.isfinite(r32).all() and e * SPARE <= 1.0, (what, m, e, len(hs))
        worst = max(worst, e)
    return worst


def _floor_sampling(cfg, train, ps, z0, eps, sol_kw, what, t0=None):
    """-> (worst share of the bar, per member (float32 samples, float64 logq))"""
    worst, out = 0.0, []
    for m in range(ps.shape[0]):
        c = cfg if t0 is None else R.cfg_of(cfg, (cfg.tspan[0], float(np.float32(t0[m]))), cfg.use_jvp)
        hs = R.oracle_steps(c, train, ps[m], z0[m], eps[m], sol_kw, generate=True)
        assert abs(sum(hs) - (c.tspan[0] - c.tspan[1])) <= 1e-9
        x64, q64 = R.replay_generate(c, train, ps[m], z0[m], eps[m], hs, np.float64)
        x32, q32 = R.replay_generate(c, train, ps[m], z0[m], eps[m], hs, np.float32)
        e = max(parity_err(x32, x64), parity_err(q32[None], q64[None], trace_row=0))
        assert e * SPARE <= 1.0, (what, m, e, len(hs))
        worst = max(worst, e)
        out.append((x32, q64))
    return worst, out


@pytest.mark.parametrize("ci", range(len(R.INFERENCE_CASES)))
def test_float32_floor_of_the_inference_cases(ci):
    cfg, tspan, M, B, train, jvp, sol_kw = R.INFERENCE_CASES[ci]
    cfg = R.cfg_of(cfg, tspan, jvp)
    ps, xs, eps = R.members(cfg, M, B, 2000 + ci)
    e = _floor_inference(cfg, train, ps, xs, eps, sol_kw, f"inference case {ci}")
    print(f"float32 floor, inference case {ci}: {e:.3f} of the bar")


@pytest.mark.parametrize("ci", range(len(R.GENERATE_CASES)))
def test_float32_floor_of_the_sampling_cases(ci):
    cfg, tspan, M, n, train, jvp, sol_kw = R.GENERATE_CASES[ci]
    cfg = R.cfg_of(cfg, tspan, jvp)
    ps, _, eps = R.members(cfg, M, n, 3000 + ci)
    z0 = R.base_draws(cfg, M, n, 3000 + ci)
    e, _ = _floor_sampling(cfg, train, ps, z0, eps, sol_kw, f"sampling case {ci}")
    print(f"float32 floor, sampling case {ci}: {e:.3f} of the bar")


@pytest.mark.parametrize("name", list(R.END_TIME))
def test_float32_floor_of_the_end_time_cases(name):
    """The members' own end times (and the inference half of the rerun case), on their own spans and step settings."""
    _, cfg, seed, M, B, sol_kw, t1 = R.END_TIME[name]
    cfg = R.cfg_of(cfg)
    ps, xs, eps = R.members(cfg, M, B, seed)
    e = _floor_inference(cfg, True, ps, xs, eps, sol_kw, name, t1=t1)
    print(f"float32 floor, {name}: {e:.3f} of the bar")


@pytest.mark.parametrize("name", list(R.START_TIME))
def test_float32_floor_of_the_start_time_cases(name):
    """Sampling from the members' own start times, the sampling half of the rerun case, and the re-scoring cases: those are
    held on the device to the solver tolerance R.RESCORE_RTOL -- scoring the float32 samples again in float32, on the steps
    the float64 controller takes for them, returns the float64 logq within a quarter of THAT bar."""
    _, cfg, seed, M, n, train, sol_kw, t0 = R.START_TIME[name]
    cfg = R.cfg_of(cfg)
    ps, _, eps = R.members(cfg, M, n, seed)
    z0 = R.base_draws(cfg, M, n, seed)
    e, out = _floor_sampling(cfg, train, ps, z0, eps, sol_kw, name, t0=t0)
    print(f"float32 floor, {name}: {e:.3f} of the bar")
    if name.startswith("re-scoring"):
        for m, (x32, q64) in enumerate(out):
            hs = R.oracle_steps(cfg, False, ps[m], x32, None, sol_kw)
            r32, _ = R.replay_inference(cfg, False, ps[m], x32, None, hs, np.float32)
            e = parity_err(r32[0][None], q64[None], rtol=R.RESCORE_RTOL, trace_row=0)
            assert e * SPARE <= 1.0, (name, m, e)


@pytest.mark.parametrize("oi", range(len(R.OTHER_CASES)))
def test_float32_floor_of_the_other_cases(oi):
    name, cfg, tspan, train, seed, M, B, scales, sol_kw = R.OTHER_CASES[oi]
    cfg = R.cfg_of(cfg, tspan)
    ps, xs, eps = R.members(cfg, M, B, seed, scales=scales)
    e = _floor_inference(cfg, train, ps, xs, eps, sol_kw, name)
    print(f"float32 floor, {name}: {e:.3f} of the bar")
