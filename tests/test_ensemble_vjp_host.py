"""Differentiable ensembles without a device: the two entry points of include/cnfhip_ensemble_vjp.h are declared, exported and
bound; the C call and ``inference_vjp_many`` say what is wrong with their arguments before they ask for a device; the float32
floor of every case of tests/test_gpu_ensemble_vjp.py leaves its bar where that test needs it; and the cotangent of the
built-in loss ties ``inference_vjp_many``'s convention to ``loss_and_grad_many``'s in the reference."""
import ctypes
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from oracle import cnf_grad_oracle as G
from tests import ensemble_vjp_ref as R
from tests import vjp_ref as V

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cnf_ensemble_vjp_capacity", "cnf_inference_vjp_many"]


def _model(dims=(2, 6, 2), nvars=1, naugs=1, **kw):
    layers = [cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])]
    return cnf.construct(cnf.RNODE, cnf.Chain(*layers), nvars, naugs, rng=5, **kw)


def test_entry_points_are_declared_exported_and_bound():
    """Fails without the feature.  A header of its own that cnfhip.h includes, a binding table of its own, disjoint from every
    other table, and the declared names are exactly the bound ones."""
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_ensemble_vjp.h"', main, flags=re.M)
    txt = strip(open(os.path.join(ROOT, "include", "cnfhip_ensemble_vjp.h")).read())
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", txt)))
    assert declared == NAMES, declared
    assert set(declared) == set(_lib.ENSEMBLE_VJP_EXPORTS)
    others = [_lib.EXPORTS, _lib.SAMPLING_EXPORTS, _lib.BASEGRAD_EXPORTS, _lib.ENSEMBLE_EXPORTS, _lib.ENSEMBLE_EVAL_EXPORTS,
              _lib.PATH_EXPORTS]
    for table in others:
        assert not set(declared) & set(table)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    for name in ("ensemble_vjp_capacity", "inference_vjp_many", "differentiable_inference_many"):
        assert callable(getattr(cnf, name, None)), name
    assert callable(getattr(cnf.EnsembleDist, "log_prob", None))


def test_the_c_call_checks_its_arguments_before_any_device():
    """With no handle at all (none can exist without a device) every complaint about the arguments still comes first."""
    l = _lib.lib()
    buf = np.zeros(64, dtype=np.float32)
    st = np.zeros(4, dtype=np.int32)
    p = buf.ctypes.data
    opts = _lib.cnf_solve_opts(0.0, 1.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)

    def call(M=2, B=4, params=p, xs=p, eps=p, o=ctypes.byref(opts), cot=p, logpx=p, regs=p, grad=p, gx=p, status=st.ctypes.data,
             mode=_lib.MODE_TRAIN):
        return l.cnf_inference_vjp_many(None, mode, M, params, xs, eps, B, o, None, cot, logpx, regs, grad, gx, status, None, None)

    assert call(M=0) == _lib.ERR_BAD_SHAPE and call(M=-3) == _lib.ERR_BAD_SHAPE
    assert call(B=0) == _lib.ERR_BAD_SHAPE
    for name in ("params", "xs", "eps", "o", "cot", "logpx", "regs", "grad", "status"):
        assert call(**{name: None}) == _lib.ERR_BAD_ARG, name
    assert call(mode=7) == _lib.ERR_BAD_ARG
    assert call(eps=None, mode=_lib.MODE_TEST) == _lib.ERR_BAD_ARG        # (TestMode takes no probes: only the handle is missing)
    assert call(gx=None) == _lib.ERR_BAD_ARG                              # (grad_x may be NULL: likewise)
    assert call() == _lib.ERR_BAD_ARG
    assert l.cnf_ensemble_vjp_capacity(None, _lib.MODE_TRAIN, 32) == 0


def test_python_argument_checks():
    icnf = _model()
    n = icnf.nn.n_params_internal
    M, B = 3, 8
    xs, ps, eps = torch.zeros(M, 1, B), torch.zeros(M, n), torch.zeros(M, 2, B)
    g = torch.zeros(M, B)
    T = cnf.TrainMode()
    bad_cot = [
        g, None, (g,), (g, g), (g, (g, g)), (g, (g, g, g, g)),                                     # not (g_logpx, (g_E, g_n, g_A))
        (torch.zeros(M, B + 1), None), (torch.zeros(B), None), (torch.zeros(M - 1, B), None),      # shapes; M mismatch
        (g, (g, torch.zeros(M, 1), g)), (g, (None, None, torch.zeros(B, M))),
        (g.numpy(), None), (g, (g, np.zeros((M, B), np.float32), None)),                            # host arrays
    ]
    for cot in bad_cot:
        with pytest.raises(ValueError):
            cnf.inference_vjp_many(icnf, T, xs, ps, {}, cot, eps=eps)
    # M mismatches between xs, ps and cot; shapes of the other arguments as loss_and_grad_many checks them
    for kw in (dict(xs=torch.zeros(2, 1, B)), dict(ps=torch.zeros(2, n)), dict(ps=torch.zeros(M, n + 1)), dict(eps=torch.zeros(M, 2, 7)),
               dict(xs=torch.zeros(1, B), ps=torch.zeros(2, n)), dict(t1=[1.0, 2.0]), dict(t1=[1.0, 0.0, 1.0])):
        a = dict(xs=xs, ps=ps, eps=eps, t1=None)
        a.update(kw)
        with pytest.raises(ValueError):
            cnf.inference_vjp_many(icnf, T, a["xs"], a["ps"], {}, (g, None), eps=a["eps"], t1=a["t1"])
    with pytest.raises(ValueError):
        cnf.inference_vjp_many(icnf, cnf.TestMode(), xs, ps, {}, (g, None), eps=eps)
    with pytest.raises(NotImplementedError):                                # host arrays
        cnf.inference_vjp_many(icnf, T, xs.numpy(), ps.numpy(), {}, (g, None))
    with pytest.raises(NotImplementedError):
        cnf.differentiable_inference_many(icnf, T, xs.numpy(), ps.numpy(), {})
    # None rows are accepted: these get as far as the device (or the no-device error)
    assert icnf._handle is None
    for cot in ((g, None), (None, (None, g, None)), (None, None), (g, (None, None, None))):
        assert len(cnf.ensemble._cot_many(cot, M, B)) == 4
    # a shared data set (nvars, B) is every member's
    cnf.ensemble._check_inputs(icnf, T, xs[0].unsqueeze(0).expand(M, 1, B), ps, eps, None)


def test_refusals_come_before_anything_is_drawn():
    lay = lambda dims: cnf.Chain(*[cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])])
    models = {
        "conditional": cnf.construct(cnf.CondRNODE, lay((4, 6, 2)), 1, 1, rng=5),
        "basedist": cnf.construct(cnf.RNODE, lay((2, 6, 2)), 1, 1, rng=5, basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2)),
        "generic": cnf.construct(cnf.RNODE, lay((2, 6, 2)), 1, 1, rng=5, compute_mode=cnf.HIPVecJacMatrixMode("generic")),
        "wide hidden layer": cnf.construct(cnf.RNODE, lay((2, 80, 2)), 1, 1, rng=5),
    }
    for name, ic in models.items():
        before = ic.rng.bit_generator.state
        x, p = torch.zeros(2, ic.nvars, 16), torch.zeros(2, ic.nn.n_params_internal)
        with pytest.raises(NotImplementedError):
            cnf.inference_vjp_many(ic, cnf.TrainMode(), x, p, {}, (torch.zeros(2, 16), None))
        with pytest.raises(NotImplementedError):
            cnf.differentiable_inference_many(ic, cnf.TrainMode(), x, p, {})
        assert cnf.ensemble_vjp_capacity(ic, cnf.TrainMode(), 16) == 0, name
        assert ic.rng.bit_generator.state == before and ic._handle is None, name


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_float32_floor_of_every_gpu_case_is_under_a_quarter_of_its_bar(case):
    """The floor: ``vjp32`` against ``vjp64`` on the case's inputs, through the steps the float64 oracle's adaptive solve
    accepts -- never a device number.  Under a quarter of the bar ``rtol = max(1e-4, 8 floor)`` AND that bar still at 1e-4: the
    device has three quarters of 1e-4 to itself on every block of every member and cotangent."""
    ps, xs, eps = R.inputs(case)
    worst = 0.0
    for m in range(R.M):
        dts, st = R.host_steps(case, m, ps, xs, eps)
        assert len(dts) >= 1
        for name, cot in R.cotangents(case, m).items():
            for block, floor, rtol in R.floors(case, m, ps, xs, eps, cot, dts):
                worst = max(worst, floor)
                assert floor < 0.25 * rtol and rtol == V.RTOL, (case.name, m, name, block, floor, rtol)
    print(f"{case.name}: worst float32 floor {worst:.2e} of the block's scale (bar {V.RTOL:g})")


def test_the_rejecting_member_rejects_in_the_oracle_too():
    case = next(c for c in R.CASES if "rejects" in c.name)
    ps, xs, eps = R.inputs(case)
    _, st = R.host_steps(case, 0, ps, xs, eps)
    assert st.nreject >= 1, st


@pytest.mark.parametrize("case", [c for c in R.CASES if c.B > 1], ids=[c.name for c in R.CASES if c.B > 1])
def test_loss_cotangent_reproduces_loss_and_grad(case):
    """The uniform cotangent (-1/B, lam1/B, lam2/B, lam3/B) through ``vjp64`` is ``G.loss_and_grad`` (``loss_and_grad_test`` in
    TestMode) on every member: the convention of ``inference_vjp_many`` -- cotangents themselves, the dlogp row carrying
    -g_logpx -- and the loss's are one."""
    ps, xs, eps = R.inputs(case)
    f64 = lambda a: np.asarray(a, np.float64)
    for m in range(R.M):
        cfg = R.member_cfg(case, m)
        dts, _ = R.host_steps(case, m, ps, xs, eps)
        cot = V.loss_cotangent(cfg, case.B, case.train)
        out, g, gx = V.vjp64(cfg, ps[m], xs[m], eps[m] if case.train else None, cot, dts, train=case.train)
        if case.train:
            val, gr, st = G.loss_and_grad(cfg, f64(ps[m]), f64(xs[m]), f64(eps[m]), None, dts=dts)
        else:
            val, gr, st = G.loss_and_grad_test(cfg, f64(ps[m]), f64(xs[m]), None, dts=dts)
        e, ex = np.abs(g - gr).max() / V.scale(gr), np.abs(gx - st.grad_x).max() / V.scale(st.grad_x)
        assert e <= 1e-12 and ex <= 1e-12, (case.name, m, e, ex)
        # ... and the loss is the cotangent applied to the outputs (it is linear in them)
        assert abs(float(np.sum(cot * out)) - val) <= 1e-12 * max(1.0, abs(val)), (case.name, m)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-device error needs a machine without one")
def test_no_device_is_the_handles_error():
    icnf = _model()
    with pytest.raises(cnf.CNFError) as e:
        icnf.handle()
    n = icnf.nn.n_params_internal
    with pytest.raises(cnf.CNFError) as e2:
        cnf.inference_vjp_many(icnf, cnf.TrainMode(), torch.zeros(2, 1, 8), torch.zeros(2, n), {}, (torch.zeros(2, 8), None))
    assert e2.value.status == e.value.status == _lib.ERR_NO_DEVICE
