"""Differentiable flow paths without a device: the reference of tests/path_vjp_ref.py against central differences in float64 and
against the references it extends; the float32 floor of every case of tests/test_gpu_path_vjp.py; the entry points of
include/cnfhip_path_vjp.h declared, exported and bound; refusals and argument errors on the host, before a handle exists.

Measured here (central differences, float64, every case, both directions): at most 6.3e-10 of the gradient's scale (bar 1e-6);
float32 floors through the float64 oracle's own steps at most 9.0e-6 of a block's scale (the bar starts to widen at 1.25e-5)."""
import ctypes
import os
import re

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import gen_vjp_ref as GR
from tests import path_ref as P
from tests import path_vjp_ref as R
from tests import vjp_ref as V

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cnf_generate_path_vjp", "cnf_inference_path_vjp", "cnf_path_vjp_max_batch", "cnf_path_vjp_steps"]
BY = {c.name: c for c in R.CASES}


def _setup(case, sampling, which="mixed"):
    flat, xs, z0, eps = R.inputs(case)
    ts, hs, st = R.host_steps(case, flat, xs, z0, eps, sampling)
    span = (case.cfg.tspan[1], case.cfg.tspan[0]) if sampling else case.cfg.tspan
    sv = R.save_times(case, ts, hs, span, which)
    return flat, xs, z0, eps, ts, hs, sv, span


def _run(case, sampling, flat, xs, z0, eps, cot, pc, ts, hs, sv, dtype=np.float64):
    """-> (value of <cot, outputs> + <path_cot, path>, grad, grad of the input)."""
    e = eps if case.train else None
    if sampling:
        cz, cl = cot if cot is not None else (None, None)
        z, lq, path, lqp, g, gz0 = R.generate(case.cfg, flat, z0, e, cz, cl, pc, ts, hs, sv, case.train, dtype)
        J = 0.0
        if cz is not None:
            J += float(np.sum(np.asarray(cz, np.float64) * z[:np.asarray(cz).shape[0]]))
        if cl is not None:
            J += float(np.sum(np.asarray(cl, np.float64) * lq))
        for k, v in (pc or {}).items():
            J += float(np.sum(np.asarray(v, np.float64) * (path[:, :case.cfg.n_in] if k == "z" else lqp)))
        return J, g, gz0
    out, path, g, gx = R.inference(case.cfg, flat, xs, e, cot, pc, ts, hs, sv, case.train, dtype)
    n_in = case.cfg.n_in
    J = float(np.sum(np.asarray(cot, np.float64) * out)) if cot is not None else 0.0
    rows = {"z": slice(0, n_in), "dlogp": n_in, "E": n_in + 1, "n": n_in + 2}
    for k, v in (pc or {}).items():
        J += float(np.sum(np.asarray(v, np.float64) * path[:, rows[k]]))
    return J, g, gx


@pytest.mark.parametrize("sampling", [False, True], ids=["inference", "sampling"])
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_reference_matches_central_differences(case, sampling):
    """Directional central differences in float64 along three random unit directions of the parameters and of the input, with
    every cotangent set at once; at most 1e-6 of the gradient's scale.  The path's share of the gradient is printed: a missing
    injection cannot hide behind the terminal term."""
    flat, xs, z0, eps, ts, hs, sv, span = _setup(case, sampling)
    kinds = {k for k, _, _ in R.brackets(span, ts, hs, sv)}
    assert kinds == {R.START, R.END, R.INTERIOR}, kinds
    cot, pc = R.path_cotangents(case, len(sv), sampling, "all")
    f64 = lambda a: np.asarray(a, np.float64)
    J, g, gin = _run(case, sampling, flat, xs, z0, eps, cot, pc, ts, hs, sv)
    _, g_term, _ = _run(case, sampling, flat, xs, z0, eps, cot, None, ts, hs, sv)
    share = V.scale(g - g_term) / V.scale(g)
    rng = np.random.default_rng(5)
    worst = 0.0
    x_in = z0 if sampling else xs
    for _ in range(3):
        dp = rng.standard_normal(flat.size); dp /= np.linalg.norm(dp)
        dx = rng.standard_normal(x_in.shape); dx /= np.linalg.norm(dx)
        h = 1e-5
        for d_flat, d_x, grad in ((dp, None, g), (None, dx, gin)):
            vals = []
            for s in (+1.0, -1.0):
                fl = f64(flat) + (s * h * d_flat if d_flat is not None else 0.0)
                xx = f64(x_in) + (s * h * d_x if d_x is not None else 0.0)
                vals.append(_run(case, sampling, fl, xx if not sampling else xs, xx if sampling else z0, eps, cot, pc, ts, hs, sv)[0])
            fd = (vals[0] - vals[1]) / (2 * h)
            an = float(np.sum(grad * (d_flat if d_flat is not None else d_x)))
            worst = max(worst, abs(fd - an) / V.scale(grad))
    print(f"{case.name} {'sampling' if sampling else 'inference'}: central differences off by {worst:.2e} of the gradient's scale; "
          f"the path carries {100 * share:.0f} % of the parameter gradient")
    assert worst <= 1e-6, worst
    assert share > 0.01


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_without_a_path_cotangent_it_is_vjp_ref(case):
    """Bit for bit: ``vjp_ref.vjp`` (inference) and ``gen_vjp_ref.vjp`` (sampling) through the same steps, in float64 and float32."""
    for dtype in (np.float64, np.float32):
        c = lambda a: None if a is None else np.asarray(a).astype(dtype)
        flat, xs, z0, eps, ts, hs, sv, _ = _setup(case, False)
        cot, _ = R.path_cotangents(case, len(sv), False, "terminal")
        e = eps if case.train else None
        out, _, g, gx = R.inference(case.cfg, flat, xs, e, cot, None, ts, hs, sv, case.train, dtype)
        out0, g0, gx0 = V.vjp(case.cfg, c(flat), c(xs), c(e), c(cot), [abs(float(h)) for h in hs], train=case.train)
        assert np.array_equal(out, out0) and np.array_equal(g, g0) and np.array_equal(gx, gx0), (case.name, dtype)
        flat, xs, z0, eps, ts, hs, sv, _ = _setup(case, True)
        (cz, cl), _ = R.path_cotangents(case, len(sv), True, "terminal")
        z, lq, _, _, g, gz0 = R.generate(case.cfg, flat, z0, e, cz, cl, None, ts, hs, sv, case.train, dtype)
        z1, lq1, g1, gz1, _ = GR.vjp(case.cfg, c(flat), c(z0), c(e), c(cz), c(cl), [abs(float(h)) for h in hs], train=case.train)
        assert np.array_equal(z, z1) and np.array_equal(g, g1) and np.array_equal(gz0, gz1), (case.name, dtype)
        assert np.allclose(lq, lq1, rtol=1e-6 if dtype == np.float32 else 1e-14)


def test_a_cotangent_at_t_start_changes_grad_x_only():
    case = BY["path-readme-vjp-B33"]
    flat, xs, z0, eps, ts, hs, sv, _ = _setup(case, False)
    assert sv[0] == np.float32(case.cfg.tspan[0])
    cot, full = R.path_cotangents(case, len(sv), False, "all")
    pc = {"z": np.zeros_like(full["z"])}
    pc["z"][0] = full["z"][0]
    _, path, g, gx = R.inference(case.cfg, flat, xs, eps, cot, pc, ts, hs, sv)
    _, _, g0, gx0 = R.inference(case.cfg, flat, xs, eps, cot, None, ts, hs, sv)
    assert np.array_equal(g, g0)
    assert np.array_equal(gx, gx0 + pc["z"][0][:case.cfg.nvars].astype(np.float64)) and not np.array_equal(gx, gx0)
    assert np.array_equal(path[0][:case.cfg.nvars], xs.astype(np.float64))


def test_a_z_cotangent_at_t_end_is_the_terminal_cotangent_of_sampling():
    case = BY["path-regr-vjp-B17-rejects"]
    flat, xs, z0, eps, ts, hs, sv, _ = _setup(case, True, "end")
    assert len(sv) == 1
    (cz, _), _ = R.path_cotangents(case, 1, True, "terminal")
    a = R.generate(case.cfg, flat, z0, eps, cz, None, None, ts, hs, sv)
    b = R.generate(case.cfg, flat, z0, eps, None, None, {"z": cz[None]}, ts, hs, sv)
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and np.abs(a[4]).max() > 0
    assert np.array_equal(b[2][0][:case.cfg.n_in], b[0])                  # the slice at t_end is the final state


@pytest.mark.parametrize("sampling", [False, True], ids=["inference", "sampling"])
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_float32_floor_keeps_the_bar_under_its_cap(case, sampling):
    """The float32 run of the reference against its float64 run, through the float64 oracle's own steps -- never a device number
    --, for every cotangent set together and for the path rows alone: ``rtol = max(1e-4, 8 floor)`` stays at most
    ``vjp_ref.RTOL_CAP`` on every block."""
    flat, xs, z0, eps, ts, hs, sv, _ = _setup(case, sampling)
    worst = 0.0
    for which in ("all", "path-only"):
        cot, pc = R.path_cotangents(case, len(sv), sampling, which)
        _, g64, x64 = _run(case, sampling, flat, xs, z0, eps, cot, pc, ts, hs, sv)
        _, g32, x32 = _run(case, sampling, flat, xs, z0, eps, cot, pc, ts, hs, sv, np.float32)
        for name, _, floor, rtol, _, _ in V.report(g64, x64, (g64, x64), (g32, x32), case.cfg.net):
            worst = max(worst, floor)
            assert rtol <= V.RTOL_CAP, (case.name, which, name, floor, rtol)
    print(f"{case.name} {'sampling' if sampling else 'inference'}: worst float32 floor {worst:.2e} of the block's scale")


def test_the_rejecting_case_rejects_in_float32_too():
    case = BY["path-regr-vjp-B17-rejects"]
    flat, xs, z0, eps = R.inputs(case)
    for sampling in (False, True):
        _, _, st = R.host_steps(case, flat, xs, z0, eps, sampling, np.float32)
        assert st.nreject >= 1, (sampling, st)


def test_the_case_list_and_the_save_times_cover_what_the_kernel_can_get_wrong():
    assert {c.B for c in R.CASES} == {1, 17, 33}
    assert {(c.train, c.jvp) for c in R.CASES} == {(True, False), (True, True), (False, False)}
    assert {c.cfg.net.dims for c in R.CASES} == {(2, 6, 2), (16, 48, 16), (7, 13, 7), (6, 9, 6)}
    assert any(c.cfg.tspan[1] < c.cfg.tspan[0] for c in R.CASES)
    # the fixed-step case: 0.5 is exactly the end of the second step, and is served as that step's accepted state
    case = BY["path-fixed-B17"]
    flat, xs, z0, eps, ts, hs, sv, span = _setup(case, False)
    assert list(ts) == [0.0, 0.25, 0.5, 0.75] and list(hs) == [0.25] * 4
    br = R.brackets(span, ts, hs, sv)
    assert [b[:2] for b, t in zip(br, sv) if t == np.float32(0.5)] == [(R.END, 1), (R.END, 1)]
    # the mixed set: a duplicate, two interior saves in one step, more saves than steps in the K = 40 set
    for c in R.CASES:
        for sampling in (False, True):
            flat, xs, z0, eps, ts, hs, sv, span = _setup(c, sampling)
            br = R.brackets(span, ts, hs, sv)
            assert {k for k, _, _ in br} == {R.START, R.END, R.INTERIOR}
            assert any(sv[i] == sv[i + 1] for i in range(len(sv) - 1))
            inner = [n for k, n, _ in br if k == R.INTERIOR]
            assert any(inner.count(n) >= 2 for n in inner)
            k40 = R.save_times(c, ts, hs, span, "k40")
            assert len(k40) == 40 > len(ts) or c.name == "path-regr-vjp-B17-rejects" or len(ts) < 40
            # the bracketing is path_ref.replay's: the slices of the reference are the replay's
            f = c.cfg.rhs(np.asarray(flat, np.float64), np.asarray(eps, np.float64) if c.train else None, c.train)
            D = c.cfg.D(c.train)
            u0 = np.vstack([z0, np.zeros((D - c.cfg.n_in, c.B))]) if sampling else np.vstack([xs, np.zeros((D - c.cfg.nvars, c.B))])
            ref, _ = P.replay(f, u0.astype(np.float64), span, ts, hs, sv)
            path = R.adjoint(c.cfg, flat, u0.astype(np.float64), eps, span, ts, hs, sv, lambda u: np.zeros_like(u), None, c.train)[0]
            assert np.array_equal(path, ref), (c.name, sampling)


def test_entry_points_are_declared_exported_and_bound():
    """Fails without the feature.  A header of its own that cnfhip.h includes, a binding table of its own, disjoint from every
    other table, and the declared names are exactly the bound ones."""
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    main = strip(open(os.path.join(ROOT, "include", "cnfhip.h")).read())
    assert re.search(r'^#include "cnfhip_path_vjp.h"', main, flags=re.M)
    raw = open(os.path.join(ROOT, "include", "cnfhip_path_vjp.h")).read()
    assert "NO STREAMED ROUTE" in raw and "cnf_path_vjp_max_batch" in raw
    declared = sorted(set(re.findall(r"\b(cnf_[a-z0-9_]+)\s*\(", strip(raw))))
    assert declared == NAMES, declared
    assert set(declared) == set(_lib.PATH_VJP_EXPORTS)
    others = [_lib.EXPORTS, _lib.SAMPLING_EXPORTS, _lib.BASEGRAD_EXPORTS, _lib.ENSEMBLE_EXPORTS, _lib.ENSEMBLE_EVAL_EXPORTS,
              _lib.ENSEMBLE_VJP_EXPORTS, _lib.ENSEMBLE_GENERATE_VJP_EXPORTS, _lib.PATH_EXPORTS]
    for table in others:
        assert not set(declared) & set(table)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} is not exported by the built library"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    for name in ("inference_path_vjp", "generate_path_vjp", "differentiable_inference_path", "differentiable_generate_path",
                 "path_vjp_max_batch", "path_vjp_steps"):
        assert callable(getattr(cnf, name, None)), name


def test_the_c_calls_check_the_save_times_before_the_handle():
    """cnf_solve_path's check, shared: with no handle at all, bad save times are named first; with good ones the missing handle is."""
    l = _lib.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    opts = _lib.cnf_solve_opts(0.0, 1.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)
    rev = _lib.cnf_solve_opts(1.0, 0.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)

    def inf(sv, o=opts, K=None):
        s = np.asarray(sv, np.float32)
        return l.cnf_inference_path_vjp(None, _lib.MODE_TRAIN, p, p, p, 4, ctypes.byref(o), s.ctypes.data if s.size else None,
                                        len(s) if K is None else K, p, p, p, p, p, p, p, None, None)

    def gen(sv, o=rev):
        s = np.asarray(sv, np.float32)
        return l.cnf_generate_path_vjp(None, _lib.MODE_TRAIN, p, p, p, 4, ctypes.byref(o), s.ctypes.data, len(s), p, p, p, p, p, p, p, p,
                                       None, None)

    for bad in ([0.5, 0.2], [-0.1], [1.5], [np.nan], [np.inf]):
        assert inf(bad) == _lib.ERR_BAD_ARG, bad
    assert inf([]) == _lib.ERR_BAD_ARG and inf([0.5], K=0) == _lib.ERR_BAD_ARG
    assert gen([0.2, 0.5]) == _lib.ERR_BAD_ARG and gen([1.5]) == _lib.ERR_BAD_ARG
    assert inf([0.0, 0.5, 0.5, 1.0]) == _lib.ERR_BAD_ARG and gen([1.0, 0.5, 0.0]) == _lib.ERR_BAD_ARG      # (the NULL handle)
    assert l.cnf_path_vjp_max_batch(None, _lib.MODE_TRAIN) == 0
    assert l.cnf_path_vjp_steps(None, None, None, 0) == -1


def _model(dims=(2, 6, 2), nvars=1, naugs=1, tag=None, **kw):
    layers = [cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])]
    return cnf.construct(tag or cnf.RNODE, cnf.Chain(*layers), nvars, naugs, rng=5, **kw)


def test_refusals_come_before_anything_is_drawn_and_without_a_handle():
    models = {
        "conditional": _model((4, 6, 2), tag=cnf.CondRNODE),
        "basedist": _model(basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2)),
        "generic": _model(compute_mode=cnf.HIPVecJacMatrixMode("generic")),
        "wide hidden layer": _model((2, 80, 2)),
        "three layers": _model((2, 6, 6, 2)),
        "planar": cnf.construct(cnf.Planar, cnf.Chain(cnf.PlanarLayer(2, "tanh")), 2, 0, rng=5),
    }
    T = cnf.TrainMode()
    sv = [0.0, 0.5, 1.0]
    for name, ic in models.items():
        before = ic.rng.bit_generator.state
        p = torch.zeros(ic.nn.n_params_internal)
        x = torch.zeros(ic.nvars, 16)
        calls = {
            "inference_path_vjp": lambda: cnf.inference_path_vjp(ic, T, x, p, {}, saveat=sv),
            "generate_path_vjp": lambda: cnf.generate_path_vjp(ic, T, p, {}, 16, saveat=sv[::-1]),
            "differentiable_inference_path": lambda: cnf.differentiable_inference_path(ic, T, x, p, {}, saveat=sv),
            "differentiable_generate_path": lambda: cnf.differentiable_generate_path(ic, T, p, {}, 16, saveat=sv[::-1]),
        }
        for who, fn in calls.items():
            with pytest.raises(NotImplementedError) as e:
                fn()
            assert str(e.value) == f"{who}: " + cnf.ensemble._refusal(ic), (name, who)
        assert cnf.path_vjp_max_batch(ic, T) == 0, name
        assert ic.rng.bit_generator.state == before and ic._handle is None, name
    # host arrays are refused too
    ic = _model()
    n_p = ic.nn.n_params_internal
    for fn in (lambda: cnf.inference_path_vjp(ic, T, np.zeros((1, 8), np.float32), torch.zeros(n_p), {}, saveat=sv),
               lambda: cnf.inference_path_vjp(ic, T, torch.zeros(1, 8), np.zeros(n_p, np.float32), {}, saveat=sv),
               lambda: cnf.generate_path_vjp(ic, T, np.zeros(n_p, np.float32), {}, 8, saveat=sv[::-1]),
               lambda: cnf.differentiable_inference_path(ic, T, np.zeros((1, 8), np.float32), torch.zeros(n_p), {}, saveat=sv),
               lambda: cnf.differentiable_generate_path(ic, T, np.zeros(n_p, np.float32), {}, 8, saveat=sv[::-1])):
        with pytest.raises(NotImplementedError):
            fn()
    assert ic._handle is None


def test_check_saveat_errors_pass_through_and_arguments_are_checked_on_the_host():
    ic = _model()
    T = cnf.TrainMode()
    n_p = ic.nn.n_params_internal
    x, p = torch.zeros(1, 8), torch.zeros(n_p)
    before = ic.rng.bit_generator.state
    for bad in ([], [0.5, 0.2], [-0.1], [1.5], [float("nan")], "abc"):
        with pytest.raises(ValueError) as e:
            cnf.inference_path_vjp(ic, T, x, p, {}, saveat=bad)
        with pytest.raises(ValueError) as e0:
            cnf.path.check_saveat(bad, ic.tspan)
        assert str(e.value) == str(e0.value)
        with pytest.raises(ValueError):
            cnf.differentiable_inference_path(ic, T, x, p, {}, saveat=bad)
    for bad in ([0.2, 0.5], [1.5]):                        # sampling runs from tspan[1] to tspan[0]
        with pytest.raises(ValueError):
            cnf.generate_path_vjp(ic, T, p, {}, 8, saveat=bad)
        with pytest.raises(ValueError):
            cnf.differentiable_generate_path(ic, T, p, {}, 8, saveat=bad)
    sv = [0.0, 0.5, 1.0]
    for kw in (dict(xs=torch.zeros(2, 8)), dict(ps=torch.zeros(n_p + 1)), dict(eps=torch.zeros(2, 9)),
               dict(path_cot={"z": torch.zeros(3, 2, 9)}), dict(path_cot={"dlogp": torch.zeros(2, 8)}), dict(path_cot={"logq": torch.zeros(3, 8)}),
               dict(path_cot={"z": np.zeros((3, 2, 8), np.float32)}), dict(path_cot=[torch.zeros(3, 8)]), dict(cot=(torch.zeros(9), None))):
        a = dict(xs=x, ps=p, eps=None, path_cot=None, cot=None)
        a.update(kw)
        with pytest.raises(ValueError):
            cnf.inference_path_vjp(ic, T, a["xs"], a["ps"], {}, saveat=sv, cot=a["cot"], path_cot=a["path_cot"], eps=a["eps"])
    with pytest.raises(ValueError):                        # TestMode integrates neither E nor n
        cnf.inference_path_vjp(ic, cnf.TestMode(), x, p, {}, saveat=sv, path_cot={"E": torch.zeros(3, 8)})
    for kw in (dict(n=0), dict(z0=torch.zeros(2, 9)), dict(path_cot={"dlogp": torch.zeros(3, 8)}), dict(path_cot={"z": torch.zeros(3, 1, 8)}),
               dict(cot=(torch.zeros(1, 9), None))):
        a = dict(n=8, z0=None, path_cot=None, cot=None)
        a.update(kw)
        with pytest.raises(ValueError):
            cnf.generate_path_vjp(ic, T, p, {}, a["n"], saveat=sv[::-1], cot=a["cot"], path_cot=a["path_cot"], z0=a["z0"])
    assert ic._handle is None and ic.rng.bit_generator.state == before


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-device error needs a machine without one")
def test_no_device_is_the_handles_error():
    ic = _model()
    with pytest.raises(cnf.CNFError) as e:
        ic.handle()
    with pytest.raises((cnf.CNFError, ValueError)) as e2:
        cnf.inference_path_vjp(ic, cnf.TrainMode(), torch.zeros(1, 8), torch.zeros(ic.nn.n_params_internal), {}, saveat=[0.0, 1.0])
    assert isinstance(e2.value, ValueError) or e2.value.status == e.value.status == _lib.ERR_NO_DEVICE
