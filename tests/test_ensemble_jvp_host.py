"""Ensemble forward-mode without a device: the entry points of include/cnfhip_ensemble_jvp.h are declared, exported and bound;
the C calls say what is wrong with their arguments before they ask for a device; the Python shape checks and refusals hold before
anything is drawn or a handle is made; the reduction of ``loss_jvp_many`` is the hand-written mean; and the members the device
tests use (tests/test_gpu_ensemble_jvp.py) keep the float32-against-float64 floor of the reference under ``J.FLOOR_CAP``."""
import ctypes
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import jvp_ref as J

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cnf_ensemble_jvp_steps", "cnf_generate_jvp_many", "cnf_inference_jvp_many"]

# ---- the members of the device tests: M = 3, R = 3, B = 33 (three tiles: full, full, one live column) ----
M, B, SEEDS = 3, 33, (0, 1, 2)
# (16-16 of J.NETS is a one-layer network, which no ensemble call takes: TestMode runs on 2-6-2 and on the identity second layer)
PARITY = [("2-6-2", "vjp"), ("16-48-16", "jvp"), ("2-6-2", "test"), ("6-9-6-id", "test")]
FLOOR_CASES = PARITY + [("2-64-2", "vjp")]


def member_inputs(net, mode, B=B, seeds=SEEDS):
    """``J.case_inputs(net, mode, B, seed=m)`` of every member, stacked along a leading member axis."""
    return tuple(np.stack(a) for a in zip(*[J.case_inputs(net, mode, B, seed=s) for s in seeds]))


def test_entry_points_are_declared_exported_and_bound():
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_ensemble_jvp.h"', main, flags=re.M)
    txt = strip(open(os.path.join(ROOT, "include", "cnfhip_ensemble_jvp.h")).read())
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", txt)))
    assert declared == NAMES, declared
    assert set(declared) == set(_lib.ENSEMBLE_JVP_EXPORTS)
    for other in ("EXPORTS", "JVP_EXPORTS", "ENSEMBLE_EVAL_EXPORTS", "ENSEMBLE_HETERO_EXPORTS"):
        assert not set(declared) & set(getattr(_lib, other)), other
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    for name in ("inference_jvp_many", "generate_jvp_many", "loss_jvp_many", "ensemble_jvp_steps"):
        assert callable(getattr(cnf, name, None)), name


def test_the_c_calls_check_their_arguments_before_any_device():
    """With no handle at all (none can exist without a device) every complaint about the arguments still comes first."""
    l = _lib.lib()
    buf = np.zeros(64, dtype=np.float32)
    st = np.zeros(4, dtype=np.int32)
    p = buf.ctypes.data
    opts = _lib.cnf_solve_opts(0.0, 1.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)

    def inf(M=2, B=16, params=p, xs=p, eps=p, dps=p, dxs=p, R=1, o=ctypes.byref(opts), tc=0, lp=p, rg=p, dout=p, status=st.ctypes.data,
            mode=_lib.MODE_TRAIN):
        return l.cnf_inference_jvp_many(None, mode, M, params, xs, eps, B, dps, dxs, R, o, None, tc, lp, rg, dout, None, status, None, None)

    def gen(M=2, B=16, params=p, z0=p, eps=p, dps=p, dz0=p, R=1, o=ctypes.byref(opts), tc=0, z=p, lq=p, dz=p, dlq=p, status=st.ctypes.data,
            mode=_lib.MODE_TRAIN):
        return l.cnf_generate_jvp_many(None, mode, M, params, z0, eps, B, dps, dz0, R, o, None, tc, z, lq, dz, dlq, status, None, None)

    for call, ptrs in ((inf, ("params", "xs", "eps", "o", "lp", "rg", "dout", "status")),
                       (gen, ("params", "z0", "eps", "o", "z", "lq", "dz", "dlq", "status"))):
        assert call(M=0) == _lib.ERR_BAD_SHAPE and call(B=0) == _lib.ERR_BAD_SHAPE
        for name in ptrs:
            assert call(**{name: None}) == _lib.ERR_BAD_ARG, name
        assert call(mode=7) == _lib.ERR_BAD_ARG
        assert call(R=0) == _lib.ERR_BAD_ARG and call(R=65536) == _lib.ERR_BAD_ARG
        assert call(tc=-1) == _lib.ERR_BAD_ARG and call(tc=65537) == _lib.ERR_BAD_ARG
        assert call() == _lib.ERR_BAD_ARG                               # (only the handle is missing)
    assert inf(dps=None, dxs=None) == _lib.ERR_BAD_ARG and gen(dps=None, dz0=None) == _lib.ERR_BAD_ARG
    assert l.cnf_ensemble_jvp_steps(None, 0, None, None, 0) == -1


def _model(dims=(2, 6, 2), nvars=1, naugs=1):
    layers = [cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])]
    return cnf.construct(cnf.RNODE, cnf.Chain(*layers), nvars, naugs, rng=5)


def test_malformed_shapes_are_value_errors():
    icnf = _model()
    n = icnf.nn.n_params_internal
    T = cnf.TrainMode()
    xs, ps, eps = torch.zeros(3, 1, 8), torch.zeros(3, n), torch.zeros(3, 2, 8)
    ok = dict(d_ps=torch.zeros(3, 2, n), d_xs=torch.zeros(3, 2, 1, 8))
    bad = [
        dict(d_ps=None, d_xs=None),                                        # no direction
        dict(d_ps=torch.zeros(n), d_xs=None), dict(d_ps=torch.zeros(2, n), d_xs=None),      # a missing member axis
        dict(d_ps=None, d_xs=torch.zeros(1, 8)), dict(d_xs=torch.zeros(2, 1, 8)),
        dict(d_ps=torch.zeros(3, 4, n)),                                   # R differs between d_ps and d_xs
        dict(d_ps=torch.zeros(3, n)),                                      # ... or one is stacked and the other is not
        dict(d_ps=torch.zeros(3, 2, n + 1)), dict(d_xs=torch.zeros(3, 2, 1, 7)), dict(d_ps=torch.zeros(3, 0, n), d_xs=None),
    ]
    before = icnf.rng.bit_generator.state
    for kw in bad:
        a = dict(ok)
        a.update(kw)
        with pytest.raises(ValueError):
            cnf.inference_jvp_many(icnf, T, xs, ps, {}, eps=eps, **a)
        with pytest.raises(ValueError):
            cnf.loss_jvp_many(icnf, T, xs, ps, {}, eps=eps, **a)
    with pytest.raises(ValueError):                                        # ps without a member axis
        cnf.inference_jvp_many(icnf, T, xs, torch.zeros(n), {}, eps=eps, **ok)
    z0 = torch.zeros(3, 2, 8)
    okg = dict(d_ps=torch.zeros(3, 2, n), d_z0=torch.zeros(3, 2, 2, 8))
    for kw in (dict(d_ps=None, d_z0=None), dict(d_ps=torch.zeros(n), d_z0=None), dict(d_z0=torch.zeros(2, 2, 8)), dict(d_ps=torch.zeros(3, 4, n)),
               dict(d_z0=torch.zeros(3, 2, 1, 8))):
        a = dict(okg)
        a.update(kw)
        with pytest.raises(ValueError):
            cnf.generate_jvp_many(icnf, T, ps, {}, 8, z0=z0, eps=eps, **a)
    with pytest.raises(ValueError):                                        # counts out of range, checked with the shapes
        cnf.inference_jvp_many(icnf, T, xs, ps, {}, eps=eps, counts=[8, 9, 1], **ok)
    with pytest.raises(ValueError):                                        # a lambda that is zero where the model's is not
        cnf.loss_jvp_many(icnf, T, xs, ps, {}, eps=eps, lambdas=np.zeros((3, 3)), **ok)
    assert icnf.rng.bit_generator.state == before and icnf._handle is None


def test_refusals_come_before_anything_is_drawn():
    """The ``models`` of tests/test_ensemble_host.py, plus ``bases=`` and host arrays."""
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

    def calls(ic, **more):
        n = ic.nn.n_params_internal
        x, p, dp = torch.zeros(2, ic.nvars, 16), torch.zeros(2, n), torch.zeros(2, n)
        yield lambda: cnf.inference_jvp_many(ic, cnf.TrainMode(), x, p, {}, d_ps=dp, **more)
        yield lambda: cnf.loss_jvp_many(ic, cnf.TrainMode(), x, p, {}, d_ps=dp, **more)
        yield lambda: cnf.generate_jvp_many(ic, cnf.TrainMode(), p, {}, 16, d_ps=dp, **more)

    for name, ic in models.items():
        before = ic.rng.bit_generator.state
        for call in calls(ic):
            with pytest.raises(NotImplementedError):
                call()
        assert ic.rng.bit_generator.state == before and ic._handle is None, name
    ic = _model()
    before = ic.rng.bit_generator.state
    bases = cnf.EnsembleBases(np.zeros((2, 2), np.float32), std=np.ones((2, 2), np.float32))
    for call in calls(ic, bases=bases):
        with pytest.raises(NotImplementedError, match="bases"):
            call()
    n = ic.nn.n_params_internal
    x, p, dp = torch.zeros(2, 1, 16), torch.zeros(2, n), torch.zeros(2, n)
    for call in (lambda: cnf.inference_jvp_many(ic, cnf.TrainMode(), x.numpy(), p.numpy(), {}, d_ps=dp.numpy()),
                 lambda: cnf.inference_jvp_many(ic, cnf.TrainMode(), x, p, {}, d_ps=dp.numpy()),
                 lambda: cnf.inference_jvp_many(ic, cnf.TrainMode(), x, p, {}, d_xs=x.numpy()),
                 lambda: cnf.generate_jvp_many(ic, cnf.TrainMode(), p.numpy(), {}, 16, d_ps=dp),
                 lambda: cnf.generate_jvp_many(ic, cnf.TrainMode(), p, {}, 16, d_z0=np.zeros((2, 2, 16), np.float32))):
        with pytest.raises(NotImplementedError, match="device tensors"):
            call()
    assert ic.rng.bit_generator.state == before and ic._handle is None


@pytest.mark.parametrize("stacked", [False, True])
@pytest.mark.parametrize("train", [True, False])
def test_the_reduction_is_the_hand_written_mean(train, stacked):
    rng = np.random.default_rng(3)
    Mh, Bh, Rh = 3, 9, 4
    counts = np.asarray([9, 4, 1])
    lam = np.asarray([[1e-2, 1e-2, 1e-2], [0.5, 0.25, 2.0], [1e-3, 3.0, 0.125]], np.float32)
    rows = rng.standard_normal((Mh, 4, Bh)).astype(np.float32)
    tans = rng.standard_normal((Mh, Rh, 4, Bh) if stacked else (Mh, 4, Bh)).astype(np.float32)
    for m in range(Mh):                                                    # what the device leaves behind a member's count
        rows[m, :, counts[m]:] = np.nan
        tans[m, ..., counts[m]:] = np.nan
    t = lambda a: torch.from_numpy(a)
    prim = (t(rows[:, 0]), (t(rows[:, 1]), t(rows[:, 2]), t(rows[:, 3])))
    tan = (t(tans[..., 0, :]), (t(tans[..., 1, :]), t(tans[..., 2, :]), t(tans[..., 3, :])))
    mode = cnf.TrainMode() if train else cnf.TestMode()
    for cnt in (counts, np.full(Mh, Bh)):
        if cnt[1] == Bh:
            prim = tuple(torch.nan_to_num(a) if torch.is_tensor(a) else tuple(torch.nan_to_num(b) for b in a) for a in prim)
            tan = tuple(torch.nan_to_num(a) if torch.is_tensor(a) else tuple(torch.nan_to_num(b) for b in a) for a in tan)
        losses, d = cnf.loss_jvp_reduce(mode, prim, tan, cnt, lam)
        assert losses.shape == (Mh,) and losses.dtype == np.float32 and tuple(d.shape) == ((Mh, Rh) if stacked else (Mh,))
        pr = np.nan_to_num(rows).astype(np.float64)
        tn = np.nan_to_num(tans).astype(np.float64)
        for m in range(Mh):
            k = int(cnt[m])
            w = np.asarray([-1.0, *lam[m].astype(np.float64)]) if train else np.asarray([-1.0, 0.0, 0.0, 0.0])
            want = np.mean(np.einsum("r,rb->b", w, pr[m, :, :k]))
            wd = np.mean(np.einsum("r,...rb->...b", w, tn[m][..., :k]), axis=-1)
            assert abs(losses[m] - want) <= 1e-5 * max(1.0, abs(want)), (m, losses[m], want)
            assert np.abs(d[m].numpy() - wd).max() <= 1e-5 * max(1.0, np.abs(wd).max()), m


@pytest.mark.parametrize("net,mode", FLOOR_CASES, ids=[f"{n}-{m}" for n, m in FLOOR_CASES])
def test_the_members_of_the_device_tests_keep_the_floor_under_the_cap(net, mode):
    """The float32 run of the reference against its float64 run, on the steps the float64 oracle's own adaptive solve accepts,
    for every member (seed), direction and tangent array the device tests check: under ``J.FLOOR_CAP``, so that the cap of the
    bar never hides a failure there."""
    cfg, train = J.case_cfg(net, mode), mode != "test"
    flat, xs, z0, eps, dps, dxs, dz0 = member_inputs(net, mode)
    worst = 0.0
    for m in range(M):
        e = eps[m] if train else None
        dts = J.host_steps(cfg, flat[m], xs[m], e, train)
        dtg = J.host_steps(cfg, flat[m], z0[m], e, train, sampling=True)
        for r in range(J.R):
            for a, b, c in ((dps[m, r], None, None), (None, dxs[m, r], dz0[m, r]), (dps[m, r], dxs[m, r], dz0[m, r])):
                _, t64 = J.inference_jvp64(cfg, flat[m], xs[m], e, a, b, dts, train)
                _, t32 = J.inference_jvp32(cfg, flat[m], xs[m], e, a, b, dts, train)
                floors = [J.bar(t64[i], t32[i])[1] for i in range(4)]
                _, (z64, l64) = J.generate_jvp64(cfg, flat[m], z0[m], e, a, c, dtg, train)
                _, (z32, l32) = J.generate_jvp32(cfg, flat[m], z0[m], e, a, c, dtg, train)
                floors += [J.bar(z64, z32)[1], J.bar(l64, l32)[1]]
                worst = max(worst, *floors)
                assert max(floors) < J.FLOOR_CAP, (net, mode, m, r, floors)
    print(f"{net} {mode}: worst floor {worst:.2e} (cap {J.FLOOR_CAP:.2e})")
