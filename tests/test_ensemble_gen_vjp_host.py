"""Differentiable ensemble sampling without a device: the two entry points of include/cnfhip_ensemble_generate_vjp.h are declared,
exported and bound; the C call and ``generate_vjp_many`` say what is wrong with their arguments before they ask for a device;
refusals come before anything is drawn; the float32 floor of every case of tests/test_gpu_ensemble_gen_vjp.py leaves its bar
where that test needs it; and the member that is meant to reject step attempts does so in the oracle too."""
import ctypes
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import ensemble_gen_vjp_ref as R
from tests import vjp_ref as V

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cnf_ensemble_generate_vjp_capacity", "cnf_generate_vjp_many"]


def _model(dims=(2, 6, 2), nvars=1, naugs=1, **kw):
    layers = [cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])]
    return cnf.construct(cnf.RNODE, cnf.Chain(*layers), nvars, naugs, rng=5, **kw)


def test_entry_points_are_declared_exported_and_bound():
    """Fails without the feature.  A header of its own that cnfhip.h includes, a binding table of its own, disjoint from every
    other table, and the declared names are exactly the bound ones."""
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_ensemble_generate_vjp.h"', main, flags=re.M)
    raw = open(os.path.join(ROOT, "include", "cnfhip_ensemble_generate_vjp.h")).read()
    # the header says what the terminal cotangent and grad_z0 are, and where the reference samples
    assert "lam_dlogp = +cot_logq" in raw and "grad_z0 = lam_z(t_start) - cot_logq z0" in raw
    assert "src/base_icnf.jl:358-380" in raw and ":202-211" in raw
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", strip(raw))))
    assert declared == NAMES, declared
    assert set(declared) == set(_lib.ENSEMBLE_GENERATE_VJP_EXPORTS)
    others = [_lib.EXPORTS, _lib.SAMPLING_EXPORTS, _lib.BASEGRAD_EXPORTS, _lib.ENSEMBLE_EXPORTS, _lib.ENSEMBLE_EVAL_EXPORTS,
              _lib.ENSEMBLE_VJP_EXPORTS, _lib.PATH_EXPORTS]
    for table in others:
        assert not set(declared) & set(table)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    for name in ("ensemble_generate_vjp_capacity", "generate_vjp_many", "differentiable_generate_many", "reverse_kl_many"):
        assert callable(getattr(cnf, name, None)), name


def test_the_c_call_checks_its_arguments_before_any_device():
    """With no handle at all (none can exist without a device) every complaint about the arguments still comes first."""
    l = _lib.lib()
    buf = np.zeros(64, dtype=np.float32)
    st = np.zeros(4, dtype=np.int32)
    p = buf.ctypes.data
    opts = _lib.cnf_solve_opts(1.0, 0.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)

    def call(M=2, B=4, params=p, z0=p, eps=p, o=ctypes.byref(opts), cz=p, cl=p, x=p, logq=p, grad=p, gz0=p, status=st.ctypes.data,
             mode=_lib.MODE_TRAIN):
        return l.cnf_generate_vjp_many(None, mode, M, params, z0, eps, B, o, None, cz, cl, x, logq, grad, gz0, status, None, None)

    assert call(M=0) == _lib.ERR_BAD_SHAPE and call(M=-3) == _lib.ERR_BAD_SHAPE
    assert call(B=0) == _lib.ERR_BAD_SHAPE
    for name in ("params", "z0", "eps", "o", "x", "logq", "grad", "status"):
        assert call(**{name: None}) == _lib.ERR_BAD_ARG, name
    assert call(cz=None, cl=None) == _lib.ERR_BAD_ARG                     # not both cotangents
    assert call(cz=None, cl=None, M=0) == _lib.ERR_BAD_ARG                # (the null pointers are named before the shapes)
    assert call(mode=7) == _lib.ERR_BAD_ARG
    # what is allowed to be NULL: only the handle is missing
    assert call(eps=None, mode=_lib.MODE_TEST) == _lib.ERR_BAD_ARG
    assert call(gz0=None) == _lib.ERR_BAD_ARG and call(cz=None) == _lib.ERR_BAD_ARG and call(cl=None) == _lib.ERR_BAD_ARG
    assert call() == _lib.ERR_BAD_ARG
    assert l.cnf_ensemble_generate_vjp_capacity(None, _lib.MODE_TRAIN, 32) == 0


def test_python_argument_checks():
    icnf = _model()
    n_p = icnf.nn.n_params_internal
    M, n = 3, 8
    ps, z0, eps = torch.zeros(M, n_p), torch.zeros(M, 2, n), torch.zeros(M, 2, n)
    gx, gz, gl = torch.zeros(M, 1, n), torch.zeros(M, 2, n), torch.zeros(M, n)
    T = cnf.TrainMode()
    before = icnf.rng.bit_generator.state
    bad_cot = [
        gl, None, (gx,), (gx, gl, gl), (None, None),                                               # not (g_x, g_logq); both None
        (torch.zeros(M, 3, n), gl), (torch.zeros(M, 1, n + 1), None), (torch.zeros(1, n), None),   # rows; columns; no member axis
        (torch.zeros(M - 1, 1, n), gl), (gx, torch.zeros(M, n + 1)), (gx, torch.zeros(n)), (None, torch.zeros(M - 1, n)),
        (gx.numpy(), None), (None, gl.numpy()),                                                    # host arrays
    ]
    for cot in bad_cot:
        with pytest.raises(ValueError):
            cnf.generate_vjp_many(icnf, T, ps, {}, n, cot, z0=z0, eps=eps)
    # the other arguments as generate_many checks them
    for kw in (dict(ps=torch.zeros(M, n_p + 1)), dict(ps=torch.zeros(n_p)), dict(z0=torch.zeros(M, 2, n + 1)), dict(eps=torch.zeros(M, 1, n)),
               dict(z0=torch.zeros(2, n)), dict(n=0), dict(t0=[1.0, 2.0]), dict(t0=[1.0, 0.0, 1.0]), dict(t0=[1.0, np.nan, 1.0])):
        a = dict(ps=ps, n=n, z0=z0, eps=eps, t0=None)
        a.update(kw)
        with pytest.raises(ValueError):
            cnf.generate_vjp_many(icnf, T, a["ps"], {}, a["n"], (gx, gl), z0=a["z0"], eps=a["eps"], t0=a["t0"])
        with pytest.raises(ValueError):
            cnf.differentiable_generate_many(icnf, T, a["ps"], {}, a["n"], z0=a["z0"], eps=a["eps"], t0=a["t0"])
    for fn in (lambda: cnf.generate_vjp_many(icnf, T, ps.numpy(), {}, n, (gx, gl)),                # host arrays
               lambda: cnf.differentiable_generate_many(icnf, T, ps.numpy(), {}, n),
               lambda: cnf.reverse_kl_many(icnf, T, ps.numpy(), {}, n, lambda x: x.sum(1))):
        with pytest.raises(NotImplementedError):
            fn()
    with pytest.raises(ValueError):                                                               # TestMode takes probes too (not used)
        cnf.generate_vjp_many(icnf, cnf.TestMode(), ps, {}, n, (gx, gl), eps=torch.zeros(M, 2, n + 2))
    # all of that before a handle exists or anything is drawn
    assert icnf._handle is None and icnf.rng.bit_generator.state == before
    # what is accepted: either cotangent alone, g_x on nvars or on all n_in rows
    for cot in ((gx, None), (None, gl), (gz, gl), [gx, gl]):
        assert len(cnf.ensemble._cot_pair_many(icnf, cot, M, n)) == 2


def test_refusals_come_before_anything_is_drawn():
    lay = lambda dims: cnf.Chain(*[cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])])
    models = {
        "conditional": cnf.construct(cnf.CondRNODE, lay((4, 6, 2)), 1, 1, rng=5),
        "basedist": cnf.construct(cnf.RNODE, lay((2, 6, 2)), 1, 1, rng=5, basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2)),
        "generic": cnf.construct(cnf.RNODE, lay((2, 6, 2)), 1, 1, rng=5, compute_mode=cnf.HIPVecJacMatrixMode("generic")),
        "wide hidden layer": cnf.construct(cnf.RNODE, lay((2, 80, 2)), 1, 1, rng=5),
    }
    T = cnf.TrainMode()
    for name, ic in models.items():
        before = ic.rng.bit_generator.state
        p = torch.zeros(2, ic.nn.n_params_internal)
        calls = {
            "generate_vjp_many": lambda: cnf.generate_vjp_many(ic, T, p, {}, 16, (None, torch.zeros(2, 16))),
            "differentiable_generate_many": lambda: cnf.differentiable_generate_many(ic, T, p, {}, 16),
            "reverse_kl_many": lambda: cnf.reverse_kl_many(ic, T, p, {}, 16, lambda x: x.sum(1)),
        }
        for who, fn in calls.items():
            with pytest.raises(NotImplementedError) as e:
                fn()
            # ... in the words of the other ensemble calls
            with pytest.raises(NotImplementedError) as e0:
                cnf.generate_many(ic, T, p, {}, 16)
            mine = str(e.value).replace("differentiable_generate_many", "X").replace("generate_vjp_many", "X")
            assert mine == str(e0.value).replace("generate_many", "X"), (name, who)
        assert cnf.ensemble_generate_vjp_capacity(ic, T, 16) == 0, name
        assert ic.rng.bit_generator.state == before and ic._handle is None, name


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_float32_floor_of_every_gpu_case_is_under_a_quarter_of_its_bar(case):
    """The floor: ``vjp32`` against ``vjp64`` of tests/gen_vjp_ref.py on the case's inputs, through the steps the float64
    oracle's adaptive solve of the sampling problem accepts -- never a device number.  Under a quarter of the bar
    ``rtol = max(1e-4, 8 floor)`` AND that bar still at 1e-4: the device has three quarters of 1e-4 to itself on every block
    (and on grad_z0) of every member and cotangent set."""
    ps, z0, eps = R.inputs(case)
    worst = 0.0
    for m in range(R.M):
        dts, st = R.host_steps(case, m, ps, z0, eps)
        assert len(dts) >= 1
        cots = R.cotangents(case, m)
        assert sorted(cots) == ["both", "logq", "x", "z-all-rows"]
        for name, cot in cots.items():
            for block, floor, rtol in R.floors(case, m, ps, z0, eps, cot, dts):
                worst = max(worst, floor)
                assert floor < 0.25 * rtol and rtol == V.RTOL, (case.name, m, name, block, floor, rtol)
    print(f"{case.name}: worst float32 floor {worst:.2e} of the block's scale (bar {V.RTOL:g})")


def test_the_rejecting_member_rejects_in_the_oracle_too():
    case = next(c for c in R.CASES if "rejects" in c.name)
    ps, z0, eps = R.inputs(case)
    _, st = R.host_steps(case, 0, ps, z0, eps)
    assert st.nreject >= 1, st


def test_the_case_list_covers_what_the_kernel_can_get_wrong():
    """Three tiles that must meet with one live column in the last (B = 33) and per-member start times; one tile with one
    column; all three modes; one, three hidden tiles and the identity pair; a network without augmentation."""
    by = {c.name: c for c in R.CASES}
    assert len(R.CASES) == 7 and R.M == 3
    assert by["gen-readme-vjp-B33"].t1 is not None and by["gen-readme-vjp-B33"].B == 33
    assert {c.B for c in R.CASES} == {1, 17, 33}
    assert {(c.train, c.jvp) for c in R.CASES} == {(True, False), (True, True), (False, False)}
    assert {c.cfg.net.dims for c in R.CASES} == {(2, 6, 2), (16, 48, 16), (7, 13, 7), (6, 9, 6)}


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-device error needs a machine without one")
def test_no_device_is_the_handles_error():
    icnf = _model()
    with pytest.raises(cnf.CNFError) as e:
        icnf.handle()
    n = icnf.nn.n_params_internal
    with pytest.raises(cnf.CNFError) as e2:
        cnf.generate_vjp_many(icnf, cnf.TrainMode(), torch.zeros(2, n), {}, 8, (None, torch.zeros(2, 8)))
    assert e2.value.status == e.value.status == _lib.ERR_NO_DEVICE
