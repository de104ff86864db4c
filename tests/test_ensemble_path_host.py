"""Ensemble flow paths without a device: the seven entry points of include/cnfhip_ensemble_path.h are declared, exported and
bound; the C calls check every member's save times before they look at the handle; the Python refusals come before anything is
drawn, with ``ensemble._refusal``'s words; both capacities are 0 for what is refused."""
import ctypes
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cnf_ensemble_path_capacity", "cnf_ensemble_path_steps", "cnf_ensemble_path_vjp_capacity", "cnf_generate_path_many",
         "cnf_generate_path_vjp_many", "cnf_inference_path_many", "cnf_inference_path_vjp_many"]
PY_NAMES = ("ensemble_path_capacity", "ensemble_path_vjp_capacity", "ensemble_path_steps", "inference_path_many", "generate_path_many",
            "inference_path_vjp_many", "generate_path_vjp_many", "differentiable_inference_path_many",
            "differentiable_generate_path_many")


def _model(dims=(2, 6, 2), nvars=1, naugs=1, tag=None, **kw):
    layers = [cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])]
    return cnf.construct(tag or cnf.RNODE, cnf.Chain(*layers), nvars, naugs, rng=5, **kw)


def test_entry_points_are_declared_exported_and_bound():
    """Fails without the feature.  A header of its own that cnfhip.h includes, a binding table of its own, disjoint from every
    other table, and the declared names are exactly the bound ones."""
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_ensemble_path.h"', main, flags=re.M)
    raw = open(os.path.join(ROOT, "include", "cnfhip_ensemble_path.h")).read()
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", strip(raw))))
    assert declared == NAMES, declared
    assert set(declared) == set(_lib.ENSEMBLE_PATH_EXPORTS)
    others = [_lib.EXPORTS, _lib.SAMPLING_EXPORTS, _lib.BASEGRAD_EXPORTS, _lib.ENSEMBLE_EXPORTS, _lib.ENSEMBLE_EVAL_EXPORTS,
              _lib.ENSEMBLE_VJP_EXPORTS, _lib.ENSEMBLE_GENERATE_VJP_EXPORTS, _lib.PATH_EXPORTS, _lib.PATH_VJP_EXPORTS,
              _lib.ENSEMBLE_HETERO_EXPORTS]
    for table in others:
        assert not set(declared) & set(table)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    for name in PY_NAMES:
        assert callable(getattr(cnf, name, None)), name
    assert "4096" in raw and "1024" in raw                   # the per-member step caps are stated


def test_the_c_calls_check_every_members_save_times_before_the_handle():
    """With no handle at all: bad save times of ANY member are named first; with good ones the missing handle is."""
    l = _lib.lib()
    buf = np.zeros(256, dtype=np.float32)
    st = np.zeros(8, dtype=np.int32)
    p, sp = buf.ctypes.data, st.ctypes.data
    fwd = _lib.cnf_solve_opts(0.0, 1.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)
    rev = _lib.cnf_solve_opts(1.0, 0.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)
    M, K = 3, 3

    def calls(sv, per, K=K, M=M, times=None):
        s = np.ascontiguousarray(sv, dtype=np.float32)
        sd = s.ctypes.data if s.size else None
        return {
            "inf": lambda o=fwd: l.cnf_inference_path_many(None, _lib.MODE_TRAIN, M, p, p, p, 4, ctypes.byref(o), times, p, p, None, sp, None, 0,
                                                           None, sd, K, per, p),
            "gen": lambda o=rev: l.cnf_generate_path_many(None, _lib.MODE_TRAIN, M, p, p, p, 4, ctypes.byref(o), times, p, p, sp, None, 0, None,
                                                          sd, K, per, p),
            "inf_vjp": lambda o=fwd: l.cnf_inference_path_vjp_many(None, _lib.MODE_TRAIN, M, p, p, p, 4, ctypes.byref(o), sd, K, per, p, p, p, p,
                                                                   p, p, p, sp, None, None),
            "gen_vjp": lambda o=rev: l.cnf_generate_path_vjp_many(None, _lib.MODE_TRAIN, M, p, p, p, 4, ctypes.byref(o), sd, K, per, p, p, p, p, p,
                                                                  p, p, p, sp, None, None),
        }

    good = np.array([[0.0, 0.5, 1.0]] * M, dtype=np.float32)
    cases = {
        "non-monotone for one member": good.copy(),
        "outside the span": good.copy(),
        "not finite": good.copy(),
    }
    cases["non-monotone for one member"][2] = [0.0, 0.7, 0.5]
    cases["outside the span"][1] = [0.0, 0.5, 1.5]
    cases["not finite"][2, 1] = np.nan
    for name, sv in cases.items():
        for who, fn in calls(sv, 1).items():
            # (the sampling calls read the same rows against the reversed span: the good rows are bad there as well)
            assert fn() == _lib.ERR_BAD_ARG, (name, who)
    # shared save times: only the first K are looked at, whatever lies behind them
    shared = np.concatenate([np.array([0.0, 0.5, 1.0], np.float32), np.full(6, np.nan, np.float32)])
    for who, fn in calls(shared, 0).items():
        assert fn() == _lib.ERR_BAD_ARG, who                 # (the NULL handle -- see the reversed span below for the discriminating half)
    # the discriminating half: against the WRONG span the very same good times are refused, which the message tells apart
    # from the handle's complaint only through the order -- so check the order on calls whose other arguments are bad too:
    # M = 0 is CNF_ERR_BAD_SHAPE once the save times pass, CNF_ERR_BAD_ARG while they do not
    ok_fwd, ok_rev = good, good[:, ::-1]
    c = calls(ok_fwd, 1, M=0)
    assert c["inf"]() == _lib.ERR_BAD_SHAPE and c["inf_vjp"]() == _lib.ERR_BAD_SHAPE
    c = calls(ok_rev, 1, M=0)
    assert c["gen"]() == _lib.ERR_BAD_SHAPE and c["gen_vjp"]() == _lib.ERR_BAD_SHAPE
    c = calls(ok_fwd, 1, M=0)                                # the forward times along the reversed span of sampling: the save times speak first
    assert c["gen"]() == _lib.ERR_BAD_ARG and c["gen_vjp"]() == _lib.ERR_BAD_ARG
    c = calls(ok_rev, 1, M=0)
    assert c["inf"]() == _lib.ERR_BAD_ARG and c["inf_vjp"]() == _lib.ERR_BAD_ARG
    bad2 = good.copy()
    bad2[2] = [0.0, 0.7, 0.5]
    c = calls(bad2, 1, M=0)                                  # (M < 1: the first set is still checked, the others do not exist)
    assert c["inf"]() == _lib.ERR_BAD_SHAPE
    for per in (2, -1):                                      # saveat_per_member is 0 or 1
        for who, fn in calls(ok_fwd, per, M=0).items():
            assert fn() == _lib.ERR_BAD_ARG, (per, who)
    for who, fn in calls(ok_fwd, 0, K=0, M=0).items():       # K < 1, NULL save times
        assert fn() == _lib.ERR_BAD_ARG, who
    for who, fn in calls([], 0, M=0).items():
        assert fn() == _lib.ERR_BAD_ARG, who
    # no per-member start / end times on these calls
    c = calls(ok_fwd, 1, M=0, times=p)
    assert c["inf"]() == _lib.ERR_BAD_ARG
    c = calls(ok_rev, 1, M=0, times=p)
    assert c["gen"]() == _lib.ERR_BAD_ARG
    assert l.cnf_ensemble_path_capacity(None, _lib.MODE_TRAIN, 32) == 0
    assert l.cnf_ensemble_path_vjp_capacity(None, _lib.MODE_TRAIN, 32) == 0
    assert l.cnf_ensemble_path_steps(None, 0, None, None, 0) == -1


def _calls(ic, T, x, p, n, sv, svr):
    return {
        "inference_path_many": lambda: cnf.inference_path_many(ic, T, x, p, {}, saveat=sv),
        "generate_path_many": lambda: cnf.generate_path_many(ic, T, p, {}, n, saveat=svr),
        "inference_path_vjp_many": lambda: cnf.inference_path_vjp_many(ic, T, x, p, {}, saveat=sv),
        "generate_path_vjp_many": lambda: cnf.generate_path_vjp_many(ic, T, p, {}, n, saveat=svr),
        "differentiable_inference_path_many": lambda: cnf.differentiable_inference_path_many(ic, T, x, p, {}, saveat=sv),
        "differentiable_generate_path_many": lambda: cnf.differentiable_generate_path_many(ic, T, p, {}, n, saveat=svr),
    }


def test_refusals_come_before_anything_is_drawn_and_without_a_handle():
    models = {
        "conditional": _model((4, 6, 2), tag=cnf.CondRNODE),
        "basedist": _model(basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2)),
        "generic": _model(compute_mode=cnf.HIPVecJacMatrixMode("generic")),
        "32-96-32": _model((32, 96, 32), nvars=32, naugs=0),
        "wide hidden layer": _model((2, 80, 2)),
        "three layers": _model((2, 6, 6, 2)),
        "softplus": cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 6, "softplus"), cnf.Dense(6, 2, "softplus")), 1, 1, rng=5),
        "one layer": _model((2, 2)),
        "planar": cnf.construct(cnf.Planar, cnf.Chain(cnf.PlanarLayer(2, "tanh")), 2, 0, rng=5),
    }
    sv = [0.0, 0.5, 1.0]
    for name, ic in models.items():
        before = ic.rng.bit_generator.state
        p = torch.zeros(3, ic.nn.n_params_internal)
        x = torch.zeros(3, ic.nvars, 16)
        for T in (cnf.TrainMode(), cnf.TestMode()):
            for who, fn in _calls(ic, T, x, p, 16, sv, sv[::-1]).items():
                with pytest.raises(NotImplementedError) as e:
                    fn()
                assert str(e.value) == f"{who}: " + cnf.ensemble._refusal(ic), (name, who)
            assert cnf.ensemble_path_capacity(ic, T, 16) == 0 and cnf.ensemble_path_vjp_capacity(ic, T, 16) == 0, name
        assert ic.rng.bit_generator.state == before and ic._handle is None, name
    # host arrays are refused too, in the words of the ensemble calls
    ic = _model()
    T = cnf.TrainMode()
    n_p = ic.nn.n_params_internal
    xh, ph = np.zeros((3, 1, 8), np.float32), np.zeros((3, n_p), np.float32)
    before = ic.rng.bit_generator.state
    single = {"inference_path_many": "inference_path", "generate_path_many": "generate_path",
              "inference_path_vjp_many": "inference_record and inference_pullback",
              "generate_path_vjp_many": "generate_record and generate_pullback",
              "differentiable_inference_path_many": "differentiable_inference_path",
              "differentiable_generate_path_many": "differentiable_generate_path"}
    for who, fn in _calls(ic, T, xh, ph, 8, sv, sv[::-1]).items():
        with pytest.raises(NotImplementedError) as e:
            fn()
        assert str(e.value) == f"{who} takes device tensors (host arrays: {single[who]}, one member at a time)", who
    for who, fn in _calls(ic, T, xh, torch.zeros(3, n_p), 8, sv, sv[::-1]).items():
        if "inference" in who:                               # (the data on the host, the parameters not)
            with pytest.raises(NotImplementedError):
                fn()
    assert ic._handle is None and ic.rng.bit_generator.state == before


def test_save_times_and_arguments_are_checked_on_the_host():
    ic = _model()
    T = cnf.TrainMode()
    n_p = ic.nn.n_params_internal
    M, B, K = 3, 8, 3
    x, p = torch.zeros(M, 1, B), torch.zeros(M, n_p)
    before = ic.rng.bit_generator.state
    good = np.array([[0.0, 0.5, 1.0]] * M, dtype=np.float32)
    bad_fwd = []
    for row in ([0.0, 0.7, 0.5], [0.0, 0.5, 1.5], [0.0, float("nan"), 1.0]):      # one member of (M, K) is wrong
        b = good.copy()
        b[1] = row
        bad_fwd.append(b)
    bad_fwd += [np.zeros((M + 1, K), np.float32), np.zeros((M, 0), np.float32), np.zeros((1, M, K), np.float32), [], [0.5, 0.2], "abc"]
    for bad in bad_fwd:
        rev = bad if isinstance(bad, str) else np.asarray(bad, dtype=np.float32)[..., ::-1]       # (sampling: along the reversed span)
        for who, fn in _calls(ic, T, x, p, B, bad, rev).items():
            with pytest.raises(ValueError):
                fn()
    b = good.copy()
    b[1] = [0.0, 0.7, 0.5]
    with pytest.raises(ValueError, match="saveat of member 1"):
        cnf.inference_path_many(ic, T, x, p, {}, saveat=b)
    # sampling runs from tspan[1] to tspan[0]: the forward times are refused there, the reversed ones by the density calls
    c = _calls(ic, T, x, p, B, good[:, ::-1], good)
    for who, fn in c.items():
        with pytest.raises(ValueError):
            fn()
    sv, svr = good, np.ascontiguousarray(good[:, ::-1])
    for kw in (dict(xs=torch.zeros(M, 2, B)), dict(ps=torch.zeros(M, n_p + 1)), dict(ps=torch.zeros(M + 1, n_p)), dict(eps=torch.zeros(M, 2, B + 1)),
               dict(path_cot={"z": torch.zeros(M, K, 2, B + 1)}), dict(path_cot={"z": torch.zeros(K, 2, B)}),
               dict(path_cot={"dlogp": torch.zeros(M, B)}), dict(path_cot={"logq": torch.zeros(M, K, B)}),
               dict(path_cot={"z": np.zeros((M, K, 2, B), np.float32)}), dict(path_cot=[torch.zeros(M, K, B)]),
               dict(cot=(torch.zeros(M, B + 1), None)), dict(cot=(torch.zeros(B), None))):
        a = dict(xs=x, ps=p, eps=None, path_cot=None, cot=None)
        a.update(kw)
        with pytest.raises(ValueError):
            cnf.inference_path_vjp_many(ic, T, a["xs"], a["ps"], {}, saveat=sv, cot=a["cot"], path_cot=a["path_cot"], eps=a["eps"])
    with pytest.raises(ValueError):                          # TestMode integrates neither E nor n
        cnf.inference_path_vjp_many(ic, cnf.TestMode(), x, p, {}, saveat=sv, path_cot={"E": torch.zeros(M, K, B)})
    for kw in (dict(n=0), dict(z0=torch.zeros(M, 2, B + 1)), dict(path_cot={"dlogp": torch.zeros(M, K, B)}),
               dict(path_cot={"z": torch.zeros(M, K, 1, B)}), dict(cot=(torch.zeros(M, 1, B + 1), None))):
        a = dict(n=B, z0=None, path_cot=None, cot=None)
        a.update(kw)
        with pytest.raises(ValueError):
            cnf.generate_path_vjp_many(ic, T, p, {}, a["n"], saveat=svr, cot=a["cot"], path_cot=a["path_cot"], z0=a["z0"])
    # the keywords of the other ensemble calls are not keywords here
    for kw in ("counts", "lambdas", "reltol", "abstol", "t1", "t0"):
        with pytest.raises(TypeError):
            cnf.inference_path_many(ic, T, x, p, {}, saveat=sv, **{kw: None})
        with pytest.raises(TypeError):
            cnf.generate_path_vjp_many(ic, T, p, {}, B, saveat=svr, **{kw: None})
    assert ic._handle is None and ic.rng.bit_generator.state == before


def test_check_saveat_many_keeps_the_shape_it_was_given():
    f = cnf.ensemble_path.check_saveat_many
    a = f([0.0, 0.5, 0.5, 1.0], (0.0, 1.0), 3)
    assert a.shape == (4,) and a.dtype == np.float32
    b = f([[0.0, 1.0], [0.5, 0.5], [0.0, 0.0]], (0.0, 1.0), 3)
    assert b.shape == (3, 2) and b.dtype == np.float32 and b.flags.c_contiguous
    c = f([[1.0, 0.0]], (1.0, 0.0), 1)
    assert c.shape == (1, 2)
