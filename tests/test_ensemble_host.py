"""Ensembles without a device: the three entry points of include/cnfhip_ensemble.h are declared, exported and bound; the C call
says what is wrong with its arguments before it asks for a device; the Python argument checks and refusals hold; and
``loss_and_grad_many`` ends in the no-device error where ``icnf.handle()`` does."""
import ctypes
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cnf_ensemble_capacity", "cnf_ensemble_steps", "cnf_loss_grad_many"]


def _model(dims=(2, 6, 2), nvars=1, naugs=1, tag=None, **kw):
    layers = [cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])]
    return cnf.construct(tag or cnf.RNODE, cnf.Chain(*layers), nvars, naugs, rng=5, **kw)


def test_entry_points_are_declared_exported_and_bound():
    """Fails without the feature.  As for the sampling direction (tests/test_gen_vjp_ref_host.py): a header of its own that
    cnfhip.h includes, a binding table of its own, and the declared names are exactly the bound ones."""
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_ensemble.h"', main, flags=re.M)
    txt = strip(open(os.path.join(ROOT, "include", "cnfhip_ensemble.h")).read())
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", txt)))
    assert declared == NAMES, declared
    assert set(declared) == set(_lib.ENSEMBLE_EXPORTS) and not set(declared) & set(_lib.EXPORTS)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    for name in ("ensemble_capacity", "loss_and_grad_many", "fit_many", "ensemble_steps"):
        assert callable(getattr(cnf, name, None)), name


def test_the_c_call_checks_its_arguments_before_any_device():
    """With no handle at all (none can exist without a device) every complaint about the arguments still comes first."""
    l = _lib.lib()
    buf = np.zeros(64, dtype=np.float32)
    st = np.zeros(4, dtype=np.int32)
    p = buf.ctypes.data
    opts = _lib.cnf_solve_opts(0.0, 1.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)
    call = lambda M=2, B=16, params=p, xs=p, eps=p, o=ctypes.byref(opts), loss=p, grad=p, status=st.ctypes.data, mode=_lib.MODE_TRAIN: \
        l.cnf_loss_grad_many(None, mode, M, params, xs, eps, B, o, None, loss, grad, status, None, None)
    assert call(M=0) == _lib.ERR_BAD_SHAPE and call(M=-3) == _lib.ERR_BAD_SHAPE
    assert call(B=0) == _lib.ERR_BAD_SHAPE
    for name in ("params", "xs", "eps", "o", "loss", "grad", "status"):
        assert call(**{name: None}) == _lib.ERR_BAD_ARG, name
    assert call(mode=7) == _lib.ERR_BAD_ARG
    assert call(eps=None, mode=_lib.MODE_TEST) == _lib.ERR_BAD_ARG        # (TestMode takes no probes: only the handle is missing)
    assert call() == _lib.ERR_BAD_ARG
    assert l.cnf_ensemble_capacity(None, _lib.MODE_TRAIN, 32) == 0
    assert l.cnf_ensemble_steps(None, 0, None, 0) == -1


def test_python_argument_checks():
    icnf = _model()
    n = icnf.nn.n_params_internal
    xs, ps, eps = torch.zeros(3, 1, 8), torch.zeros(3, n), torch.zeros(3, 2, 8)
    T = cnf.TrainMode()
    bad = [
        dict(xs=torch.zeros(3, 2, 8)), dict(xs=torch.zeros(1, 8)), dict(xs=torch.zeros(3, 1, 0)),
        dict(ps=torch.zeros(2, n)), dict(ps=torch.zeros(3, n + 1)), dict(ps=torch.zeros(3 * n)),
        dict(eps=torch.zeros(3, 1, 8)), dict(eps=torch.zeros(3, 2, 7)), dict(eps=np.zeros((3, 2, 8), dtype=np.float32)),
        dict(t1=[1.0, 2.0]), dict(t1=[1.0, float("nan"), 1.0]), dict(t1=[1.0, 0.0, 1.0]),
    ]
    for kw in bad:
        a = dict(xs=xs, ps=ps, eps=eps, t1=None)
        a.update(kw)
        with pytest.raises(ValueError):
            cnf.loss_and_grad_many(icnf, T, a["xs"], a["ps"], {}, eps=a["eps"], t1=a["t1"])
    with pytest.raises(ValueError):
        cnf.loss_and_grad_many(icnf, cnf.TestMode(), xs, ps, {}, eps=eps)
    with pytest.raises(TypeError):
        cnf.loss_and_grad_many(icnf, "train", xs, ps, {})
    with pytest.raises(NotImplementedError):                                # host arrays
        cnf.loss_and_grad_many(icnf, T, xs.numpy(), ps.numpy(), {})


def test_refusals_come_before_anything_is_drawn():
    lay = lambda dims: cnf.Chain(*[cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])])
    models = {
        "conditional": cnf.construct(cnf.CondRNODE, lay((4, 6, 2)), 1, 1, rng=5),
        "basedist": cnf.construct(cnf.RNODE, lay((2, 6, 2)), 1, 1, rng=5, basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2)),
        "generic": cnf.construct(cnf.RNODE, lay((2, 6, 2)), 1, 1, rng=5, compute_mode=cnf.HIPVecJacMatrixMode("generic")),
        "headline network": cnf.construct(cnf.RNODE, lay((32, 128, 128, 32)), 32, 0, rng=5),
        "wide hidden layer": cnf.construct(cnf.RNODE, lay((2, 80, 2)), 1, 1, rng=5),
        "relu": cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 6, "relu"), cnf.Dense(6, 2, "tanh")), 1, 1, rng=5),
        "one layer": cnf.construct(cnf.RNODE, lay((2, 2)), 1, 1, rng=5),
        "planar": cnf.construct(cnf.Planar, cnf.Chain(cnf.PlanarLayer(2, "tanh")), 2, 0, rng=5),
    }
    for name, ic in models.items():
        before = ic.rng.bit_generator.state
        x, p = torch.zeros(2, ic.nvars, 16), torch.zeros(2, ic.nn.n_params_internal)
        with pytest.raises(NotImplementedError):
            cnf.loss_and_grad_many(ic, cnf.TrainMode(), x, p, {})
        assert cnf.ensemble_capacity(ic, cnf.TrainMode(), 16) == 0, name
        with pytest.raises(NotImplementedError):
            cnf.fit_many(cnf.ICNFModel(ic, n_epochs=1), 0, [np.zeros((8, ic.nvars), dtype=np.float32)] * 2)
        assert ic.rng.bit_generator.state == before and ic._handle is None, name
    with pytest.raises(NotImplementedError):                                # the built-in loss only
        cnf.fit_many(cnf.ICNFModel(_model(), loss=lambda *a: 0.0, n_epochs=1), 0, [np.zeros((8, 1), dtype=np.float32)] * 2)
    with pytest.raises(ValueError):
        cnf.fit_many(cnf.ICNFModel(_model(), n_epochs=1), 0, [np.zeros((8, 1), dtype=np.float32)] * 2, seeds=[1])


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-device error needs a machine without one")
def test_no_device_is_the_handles_error():
    icnf = _model()
    with pytest.raises(cnf.CNFError) as e:
        icnf.handle()
    with pytest.raises(cnf.CNFError) as e2:
        cnf.loss_and_grad_many(icnf, cnf.TrainMode(), torch.zeros(2, 1, 8), torch.zeros(2, icnf.nn.n_params_internal), {})
    assert e2.value.status == e.value.status == _lib.ERR_NO_DEVICE
    with pytest.raises(cnf.CNFError):
        cnf.ensemble_capacity(icnf, cnf.TrainMode(), 32)
