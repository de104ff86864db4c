"""Ensemble flow paths on the device: ``inference_path_many`` / ``generate_path_many`` (the plain ensemble form of k_solve_wave with
the path) and ``inference_path_vjp_many`` / ``generate_path_vjp_many`` (the PATH forms of the per-sample-cotangent gradient with a
member dimension), and the two autograd functions over them.

The contracts:
  1. member m of a call with M = 3 members equals the call with M = 1 on that member's slices, bit for bit, in every output;
  2. without the path nothing differs: ``logpx`` / regs / ``xs`` / ``logq`` are ``inference_many``'s / ``generate_many``'s bit for bit,
     tau = t0 is u0 and tau = t1 the final state;
  3. ``inference_path_vjp_many`` with M = 1 IS ``inference_path_vjp`` (bit for bit); the plain form's slices agree with
     ``inference_path`` / ``generate_path`` of the member alone at the parity bar (bit equality is reported);
  4. against float64: tests/path_vjp_ref.py replaying the steps the call itself reports, per member; slices at the bar of
     tests/test_gpu_path.py, gradients with ``vjp_ref.assert_vjp`` unchanged.

Shapes: M = 3 (two members cannot tell a stride from an offset), B in {1, 17, 33}, the 2-6-2 and 16-48-16 networks, all three
modes.  Save times are built from a first call's reported steps, different per member in the (M, K) case: t0, two times inside
one step, steps with none, a time at a step's end and its duplicate, an interior time in the last step, t1 (K = 7; K = 1 is the
first call)."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import ensemble_vjp_ref as E
from tests import envelope as Env
from tests import helpers
from tests import path_vjp_ref as R
from tests import vjp_ref as V
from tests.helpers import assert_parity, make_icnf, parity_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
M = E.M
NAMES = ["path-readme-vjp-B33", "path-regr-vjp-B17-rejects", "path-regr-jvp-B33", "path-regr-test-B17", "path-noaug-vjp-B1",
         "path-fixed-B17"]
BY = {c.name: c for c in R.CASES}
EBY = {"path-" + c.name: c for c in E.CASES}


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _mode(train):
    return cnf.TrainMode() if train else cnf.TestMode()


def _icnf(case, **kw):
    sol = dict(case.sol_kw)
    sol.update(kw)
    return make_icnf(cnf, case.cfg, jvp=case.jvp, kernel="mfma", sol_kwargs=sol)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """``(ps (M, n_params), xs (M, nvars, B), z0 (M, n_in, B), eps (M, n_in, B))``: the members' own, from ensemble_vjp_ref."""
    case = BY[name]
    if name in EBY:
        ps, xs, eps = E.inputs(EBY[name])
    else:
        parts = [R.inputs(dataclasses.replace(case, seed=case.seed + 100 * m)) for m in range(M)]
        ps, xs, eps = (np.stack([p[i] for p in parts]) for i in (0, 1, 3))
    z0 = np.random.default_rng(9800 + case.seed).standard_normal((M, case.cfg.n_in, case.B)).astype(np.float32)
    return ps, xs, z0, eps


def _span(case, sampling):
    return (case.cfg.tspan[1], case.cfg.tspan[0]) if sampling else case.cfg.tspan


def _times(case, steps, span, m):
    """Member m's K = 7 (the fixed-step case: 8) save times from its own steps: t0, two times inside one step, a time at a step's
    end and its duplicate, an interior time in the last step, t1; the steps between carry none.  Different per member."""
    t_start, t_end = np.float32(span[0]), np.float32(span[1])
    if case.fixed_saveat is not None:
        sv = np.asarray(case.fixed_saveat, np.float64).copy()
        sv[1] += 0.02 * m
        sv[6] -= 0.02 * m
        sv = sv.astype(np.float32)
        return sv if t_end >= t_start else (t_start + t_end - sv).astype(np.float32)
    ts, hs = np.asarray(steps[0], np.float64), np.asarray(steps[1], np.float64)
    N = len(ts)
    assert N >= 4, f"{case.name}: {N} steps are too few to place the save times"
    a = m % 2                                              # the step with two interior times
    at = lambda n, fr: np.float32(ts[n] + fr * hs[n])
    end = np.float32(steps[0][N - 1])                      # the end of step N - 2 (= the start of the last step), as the device filed it
    sv = np.asarray([t_start, at(a, 0.3 + 0.05 * m), at(a, 0.7 + 0.05 * m), end, end, at(N - 1, 0.4 + 0.1 * m), t_end], np.float32)
    d = 1.0 if t_end >= t_start else -1.0
    assert np.all(d * np.diff(sv) >= 0)
    return sv


def _covers(case, span, steps, sv):
    """The save times hold what the kernel can get wrong: all three kinds, a step with two, a step with none, the last step."""
    br = R.brackets(span, steps[0], steps[1], sv)
    kinds = {k for k, _, _ in br}
    assert kinds == {R.START, R.END, R.INTERIOR}, kinds
    served = [n for _, n, _ in br if n >= 0]
    N = len(steps[0])
    assert any(k == R.INTERIOR and n == N - 1 for k, n, _ in br), "no interior time in the last step (the virt stage)"
    assert max(served.count(n) for n in set(served)) >= 2 and len(set(range(N)) - set(served)) >= 1


def _state_path(path, train):
    """The dict of rows the calls return -> M x K x D x B numpy."""
    rows = [_np(path["z"]), _np(path["dlogp"])[:, :, None, :]]
    if train:
        rows += [_np(path["E"])[:, :, None, :], _np(path["n"])[:, :, None, :]]
    return np.concatenate(rows, axis=2)


def _sel_sv(sv, sel):
    return sv[sel] if sv.ndim == 2 else sv


def _plain(icnf, case, sampling, sv, sel=slice(None)):
    ps, xs, z0, eps = _inputs(case.name)
    mode = _mode(case.train)
    if sampling:
        x, lq, path, info = cnf.generate_path_many(icnf, mode, _dev(ps[sel]), {}, case.B, saveat=_sel_sv(sv, sel), z0=_dev(z0[sel]),
                                                   eps=_dev(eps[sel]))
        out = {"x": _np(x), "logq": _np(lq), "logq_path": _np(path["logq"])}
        assert info["launches"] == 2, info["launches"]
    else:
        lp, rg, path, info = cnf.inference_path_many(icnf, mode, _dev(xs[sel]), _dev(ps[sel]), {}, saveat=_sel_sv(sv, sel),
                                                     eps=_dev(eps[sel]) if case.train else None)
        out = {"logpx": _np(lp), "regs": np.stack([_np(r) for r in rg], axis=1)}
        assert info["launches"] == 1, info["launches"]
    assert info["calls"] == 1 and not info["rerun"]
    out.update(path=_state_path(path, case.train), info=info, steps=info["steps"])
    return out


def _member_cots(case, K, sampling, which):
    """Per member ``(cot, path_cot)`` of tests/path_vjp_ref.py, each member its own draws."""
    return [R.path_cotangents(dataclasses.replace(case, seed=case.seed + 1000 * (m + 1)), K, sampling, which) for m in range(M)]


def _vjp(icnf, case, sampling, sv, cots, sel=slice(None), single=False):
    """One ``*_path_vjp_many`` call over the members ``sel`` (``single``: the single-model call on the one member of ``sel``)."""
    ps, xs, z0, eps = _inputs(case.name)
    mode = _mode(case.train)
    mem = list(range(M))[sel]
    cot = [cots[m][0] for m in mem]
    pcs = [cots[m][1] for m in mem]
    pc = None if pcs[0] is None else {k: _dev(np.stack([p[k] for p in pcs])) for k in pcs[0]}
    svs = _sel_sv(sv, sel)
    if single:
        m = mem[0]
        pc1 = None if pc is None else {k: v[0] for k, v in pc.items()}
        sv1 = svs[0] if svs.ndim == 2 else svs
        if sampling:
            c = None if cot[0] is None else (_dev(cot[0][0]), _dev(cot[0][1]))
            x, lq, path, g, gin, info = cnf.generate_path_vjp(icnf, mode, _dev(ps[m]), {}, case.B, saveat=sv1, cot=c, path_cot=pc1,
                                                               z0=_dev(z0[m]), eps=_dev(eps[m]), with_z0=True)
            out = {"x": _np(x)[None], "logq": _np(lq)[None], "logq_path": _np(path["logq"])[None]}
        else:
            c = None if cot[0] is None else (_dev(cot[0][0]), tuple(_dev(r) for r in cot[0][1:]))
            lp, rg, path, g, gin, info = cnf.inference_path_vjp(icnf, mode, _dev(xs[m]), _dev(ps[m]), {}, saveat=sv1, cot=c, path_cot=pc1,
                                                                 eps=_dev(eps[m]) if case.train else None, with_x=True)
            out = {"logpx": _np(lp)[None], "regs": np.stack([_np(r) for r in rg])[None]}
        path = {k: (v[None] if k not in ("t", "steps") else v) for k, v in path.items()}
        out.update(path=_state_path(path, case.train), grad=_np(g)[None], gin=_np(gin)[None], steps=[info["steps"]])
        return out
    if sampling:
        c = None if cot[0] is None else (_dev(np.stack([a[0] for a in cot])), _dev(np.stack([a[1] for a in cot])))
        x, lq, path, g, gin, info = cnf.generate_path_vjp_many(icnf, mode, _dev(ps[sel]), {}, case.B, saveat=svs, cot=c, path_cot=pc,
                                                                z0=_dev(z0[sel]), eps=_dev(eps[sel]), with_z0=True)
        out = {"x": _np(x), "logq": _np(lq), "logq_path": _np(path["logq"])}
    else:
        c = None
        if cot[0] is not None:
            st = np.stack(cot)                             # (m, 4, B)
            c = (_dev(st[:, 0]), tuple(_dev(st[:, r]) for r in (1, 2, 3)))
        lp, rg, path, g, gin, info = cnf.inference_path_vjp_many(icnf, mode, _dev(xs[sel]), _dev(ps[sel]), {}, saveat=svs, cot=c, path_cot=pc,
                                                                  eps=_dev(eps[sel]) if case.train else None, with_x=True)
        out = {"logpx": _np(lp), "regs": np.stack([_np(r) for r in rg], axis=1)}
    assert info["launches"] == (4 if sampling else 2) and info["calls"] == 1 and not info["rerun"], info
    out.update(path=_state_path(path, case.train), grad=_np(g), gin=_np(gin), info=info, steps=info["steps"])
    return out


VALUE_KEYS = ("logpx", "regs", "x", "logq", "logq_path", "path", "grad", "gin")


def _same_bits(whole, part, m, what, host_formed=()):
    """Member m of ``whole`` equals member 0 of ``part`` in every output, the steps included.  ``host_formed``: outputs the two
    calls form on the host by different sums of the same device numbers (held at the parity bar)."""
    for k in VALUE_KEYS:
        if k in whole and k in host_formed:
            assert_parity(whole[k][m], part[k][0], f"{what}: {k}")
        elif k in whole:
            assert k in part and np.array_equal(whole[k][m], part[k][0]), f"{what}: {k} of member {m} differs from the member alone"
    for a, b in zip(whole["steps"][m], part["steps"][0]):
        assert np.array_equal(a, b), f"{what}: the steps of member {m} differ"


def _reference(case, sampling, m, sv, cot, pc, steps, dtype):
    ps, xs, z0, eps = _inputs(case.name)
    e = eps[m] if case.train else None
    ts, hs = steps
    if sampling:
        cz, cl = cot if cot is not None else (None, None)
        z, lq, path, lqp, g, gin = R.generate(case.cfg, ps[m], z0[m], e, cz, cl, pc, ts, hs, sv, case.train, dtype)
        return {"x": z[:case.cfg.nvars], "logq": lq, "logq_path": lqp, "path": path, "grad": g, "gin": gin}
    out, path, g, gin = R.inference(case.cfg, ps[m], xs[m], e, cot, pc, ts, hs, sv, case.train, dtype)
    return {"logpx": out[0], "regs": out[1:], "path": path, "grad": g, "gin": gin}


def _check_path(got, ref, r32, n_in, what):
    """Every slice at the bar of tests/test_gpu_path.py (the rule of tests/test_gpu_path_vjp.py)."""
    K = len(ref)
    worst = max(parity_err(got[k], ref[k], trace_row=n_in) for k in range(K))
    rtol = helpers.RTOL
    if worst > 1.0:
        floor = helpers.RTOL * max(parity_err(r32[k], ref[k], trace_row=n_in) for k in range(K))
        rtol = Env.rtol_of(floor)
        print(f"{what}: {worst:.2f} x the default bar; float32 floor {floor:.3g} -> rtol {rtol:.3g}")
        assert rtol <= Env.RTOL_CAP, (what, floor)
    for k in range(K):
        assert_parity(got[k], ref[k], f"{what} slice {k}", rtol=rtol, trace_row=n_in)


def _check_member(case, sampling, got, m, sv, cot, pc, what, grads):
    """Member m of ``got`` against the float64 replay of the steps it reports."""
    r64 = _reference(case, sampling, m, sv, cot, pc, got["steps"][m], np.float64)
    r32 = _reference(case, sampling, m, sv, cot, pc, got["steps"][m], np.float32)
    n_in = case.cfg.n_in
    _check_path(got["path"][m], r64["path"], r32["path"], n_in, what)
    if sampling:
        assert_parity(got["x"][m], r64["x"], f"{what} xs")
        assert_parity(got["logq"][m], r64["logq"], f"{what} logq")
        assert_parity(got["logq_path"][m], r64["logq_path"], f"{what} logq along the path")
    else:
        assert_parity(got["logpx"][m], r64["logpx"], f"{what} logpx")
        if case.train:
            assert_parity(got["regs"][m], r64["regs"], f"{what} regs")
    if grads:
        V.assert_vjp(got["grad"][m], got["gin"][m], (r64["grad"], r64["gin"]), (r32["grad"], r32["gin"]), case.cfg.net, what)


def _save_time_sets(icnf, case, sampling, vjp=False):
    """The K = 1 first call (t1 alone: its reported steps place the other save times), then ``(first, shared (K,), own (M, K))``.
    ``vjp``: the first call is the gradient form's (its evaluations use another tanh, so its steps are its own)."""
    span = _span(case, sampling)
    end = np.asarray([span[1]], np.float32)
    first = _vjp(icnf, case, sampling, end, [(None, None)] * M) if vjp else _plain(icnf, case, sampling, end)
    own = np.stack([_times(case, first["steps"][m], span, m) for m in range(M)])
    for m in range(M):
        if case.fixed_saveat is None:
            _covers(case, span, first["steps"][m], own[m])
    return first, own[0].copy(), own


@pytest.mark.parametrize("sampling", [False, True], ids=["inference", "sampling"])
@pytest.mark.parametrize("name", NAMES)
def test_the_plain_calls_keep_their_four_contracts(name, sampling):
    case = BY[name]
    icnf = _icnf(case)
    mode, n_in, nv = _mode(case.train), case.cfg.n_in, case.cfg.nvars
    ps, xs, z0, eps = _inputs(name)
    span = _span(case, sampling)
    assert cnf.ensemble_path_capacity(icnf, mode, case.B) >= M
    first, shared, own = _save_time_sets(icnf, case, sampling)
    if "rejects" in name:
        assert first["info"]["stats"][0]["nreject"] >= 1, first["info"]["stats"][0]
    # contract 2: without the path nothing differs
    if sampling:
        bx, bq = cnf.generate_many(icnf, mode, _dev(ps), {}, case.B, z0=_dev(z0), eps=_dev(eps), with_logp=True)
        base = {"x": _np(bx), "logq": _np(bq)}
    else:
        lp, rg, binfo = cnf.inference_many(icnf, mode, _dev(xs), _dev(ps), {}, eps=_dev(eps) if case.train else None)
        base = {"logpx": _np(lp), "regs": np.stack([_np(r) for r in rg], axis=1)}
        assert [s["naccept"] for s in binfo["stats"]] == [s["naccept"] for s in first["info"]["stats"]]
    bits = []
    for label, sv in (("shared", shared), ("own", own)):
        got = _plain(icnf, case, sampling, sv)
        what = f"ensemble path {name} {'sampling' if sampling else 'inference'} {label} save times"
        for k, v in base.items():
            assert np.array_equal(got[k], v), f"{what}: {k} differs from the call without a path"
        for m in range(M):
            assert all(np.array_equal(a, b) for a, b in zip(got["steps"][m], first["steps"][m])), "the save times moved a step"
            svm = _sel_sv(sv, m)
            assert svm[0] == np.float32(span[0]) and svm[-1] == np.float32(span[1])
            u0 = z0[m] if sampling else np.vstack([xs[m], np.zeros((n_in - nv, case.B), np.float32)])
            assert np.array_equal(got["path"][m, 0, :n_in], u0) and not got["path"][m, 0, n_in:].any()      # tau = t0 is u0
            if sampling:                                   # tau = t1 is the final state
                assert np.array_equal(got["path"][m, -1, :nv], got["x"][m])
                # (logq is formed by the column kernel, logq along the path on the host: the same sum to an ulp)
                assert_parity(got["logq_path"][m, -1], got["logq"][m], f"{what} member {m}: logq at t1")
            elif case.train:
                assert np.array_equal(got["path"][m, -1, n_in + 1], got["regs"][m, 0]) and np.array_equal(got["path"][m, -1, n_in + 2], got["regs"][m, 1])
            # contract 1: the member alone, bit for bit
            alone = _plain(icnf, case, sampling, sv, slice(m, m + 1))
            _same_bits(got, alone, m, what)
            # contract 4: float64 on the steps the call reports
            _check_member(case, sampling, got, m, svm, None, None, f"{what} member {m}", grads=False)
            # contract 3: the single-model plain call (the PATH form without ENS) at the parity bar
            if label == "own":
                twin = _icnf(case)
                if sampling:
                    x1, q1, p1 = cnf.generate_path(twin, mode, _dev(ps[m]), {}, case.B, saveat=svm, z0=_dev(z0[m]), eps=_dev(eps[m]))
                else:
                    l1, r1, p1 = cnf.inference_path(twin, mode, _dev(xs[m]), _dev(ps[m]), {}, saveat=svm, eps=_dev(eps[m]) if case.train else None)
                one = np.concatenate([_np(p1["z"]), _np(p1["dlogp"])[:, None, :]] + ([_np(p1["E"])[:, None, :], _np(p1["n"])[:, None, :]] if case.train else []), axis=1)
                for k in range(len(svm)):
                    assert_parity(got["path"][m, k], one[k], f"{what} member {m} vs the single-model path, slice {k}", trace_row=n_in)
                bits.append(bool(np.array_equal(got["path"][m], one)))
                twin.close()
    helpers.note(f"ensemble path {name} {'sampling' if sampling else 'inference'}: members bit-equal to the single-model path call: {bits}")
    icnf.close()


@pytest.mark.parametrize("sampling", [False, True], ids=["inference", "sampling"])
@pytest.mark.parametrize("name", NAMES)
def test_the_vjp_calls_keep_their_contracts_for_every_cotangent_set(name, sampling):
    case = BY[name]
    icnf = _icnf(case)
    mode = _mode(case.train)
    assert cnf.ensemble_path_vjp_capacity(icnf, mode, case.B) >= M
    first, shared, own = _save_time_sets(icnf, case, sampling, vjp=True)
    assert not first["grad"].any() and not first["gin"].any()                                    # (no cotangent at all: zeros)
    names = R.cot_sets(case, sampling)
    assert names[0] == "terminal" and names[-1] == "all" and len(names) >= 4
    K = own.shape[1]
    for which in names:
        for label, sv in (("own", own),) + ((("shared", shared),) if which == "all" else ()):
            cots = _member_cots(case, K, sampling, which)
            got = _vjp(icnf, case, sampling, sv, cots)
            what = f"ensemble path vjp {name} {'sampling' if sampling else 'inference'} cot {which} {label} save times"
            for m in range(M):
                assert all(np.array_equal(a, b) for a, b in zip(got["steps"][m], first["steps"][m])), "the cotangents moved a step"
                # contract 1: M = 1 of the same call, bit for bit; contract 3: the single-model call IS that case
                alone = _vjp(icnf, case, sampling, sv, cots, slice(m, m + 1))
                _same_bits(got, alone, m, what)
                if which in ("terminal", "all") and label == "own":
                    single = _vjp(icnf, case, sampling, sv, cots, slice(m, m + 1), single=True)
                    # (sampling: logpdf(z0) of logq along the path, and the sum over k of the -(sum_k g_k) z0 tail of grad_z0, are
                    # summed by torch there and in index order here -- so that a member's bits do not depend on M)
                    hf = ("logq_path", "gin") if sampling else ()
                    _same_bits(alone, single, 0, what + " (M = 1 against the single-model call)", hf)
                    _same_bits(single, alone, 0, what + " (the single-model call against M = 1)", hf)
                # contract 4
                _check_member(case, sampling, got, m, _sel_sv(sv, m), cots[m][0], cots[m][1], f"{what} member {m}", grads=True)
    icnf.close()


def _block_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) / V.scale(b)


@pytest.mark.parametrize("name", ["path-readme-vjp-B33", "path-regr-test-B17", "path-regr-jvp-B33"])
def test_without_a_path_cotangent_it_is_the_ensemble_vjp(name):
    """``path_cot=None`` gives the gradients of ``inference_vjp_many`` / ``generate_vjp_many`` of the same members -- another
    instantiation on the same forward half: the same steps, outputs at the parity bar, gradients within ``vjp_ref.RTOL`` of their
    scale (the margin of the single-model test) --, and so does the C call that asks for no slices at all."""
    case = BY[name]
    icnf = _icnf(case)
    ps, xs, z0, eps = _inputs(name)
    mode = _mode(case.train)
    worst = 0.0
    for sampling in (False, True):
        span = _span(case, sampling)
        sv = np.asarray([span[0], span[1]], np.float32)
        cots = _member_cots(case, 2, sampling, "terminal")
        got = _vjp(icnf, case, sampling, sv, cots)
        if sampling:
            c = (_dev(np.stack([a[0][0] for a in cots])), _dev(np.stack([a[0][1] for a in cots])))
            x, lq, g, gz, info = cnf.generate_vjp_many(icnf, mode, _dev(ps), {}, case.B, c, z0=_dev(z0), eps=_dev(eps), with_z0=True,
                                                       with_steps=True)
            assert_parity(got["x"], _np(x), f"{name} xs")
            assert_parity(got["logq"], _np(lq), f"{name} logq")
        else:
            st = np.stack([a[0] for a in cots])
            c = (_dev(st[:, 0]), tuple(_dev(st[:, r]) for r in (1, 2, 3)))
            lp, rg, g, gz, info = cnf.inference_vjp_many(icnf, mode, _dev(xs), _dev(ps), {}, c, eps=_dev(eps) if case.train else None,
                                                         with_x=True, with_steps=True)
            assert_parity(got["logpx"], _np(lp), f"{name} logpx")
        for m in range(M):
            assert np.array_equal(info["steps"][m], got["steps"][m][1])
            worst = max(worst, _block_err(got["grad"][m], _np(g[m])), _block_err(got["gin"][m], _np(gz[m])))
        l, h = _lib.lib(), icnf.handle()
        B, n_in = case.B, case.cfg.n_in
        if sampling:                                       # the C call with neither a path cotangent nor a place for the slices
            zr, er, pr = _dev(z0.transpose(0, 2, 1)), _dev(eps.transpose(0, 2, 1)), _dev(ps)
            czr, clr = _dev(np.stack([a[0][0] for a in cots]).transpose(0, 2, 1)), _dev(np.stack([a[0][1] for a in cots]))
            x2, lq2 = torch.zeros((M, B, case.cfg.nvars), device="cuda"), torch.zeros((M, B), device="cuda")
            g2, gz2 = torch.zeros((M, ps.shape[1]), device="cuda"), torch.zeros((M, B, n_in), device="cuda")
            status = np.full(M, -1, np.int32)
            opts = cnf.base_icnf._solve_opts(icnf, span)
            rc = l.cnf_generate_path_vjp_many(h, _lib.MODE_TRAIN if case.train else _lib.MODE_TEST, M, pr.data_ptr(), zr.data_ptr(),
                                              er.data_ptr() if case.train else None, B, C.byref(opts), sv.ctypes.data, 2, 0, czr.data_ptr(),
                                              clr.data_ptr(), None, x2.data_ptr(), lq2.data_ptr(), None, g2.data_ptr(), gz2.data_ptr(),
                                              status.ctypes.data, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            assert rc == _lib.OK and not status.any()
            assert np.array_equal(_np(g2), got["grad"]) and np.array_equal(_np(lq2), got["logq"])
            assert np.array_equal(_np(x2).transpose(0, 2, 1), got["x"]) and np.array_equal(_np(gz2).transpose(0, 2, 1), got["gin"])
        else:
            xr, er = _dev(xs.transpose(0, 2, 1)), _dev(eps.transpose(0, 2, 1))
            cm, pr = _dev(st), _dev(ps)
            lp2, rg2 = torch.zeros((M, B), device="cuda"), torch.zeros((M, 3, B), device="cuda")
            g2, gx2 = torch.zeros((M, ps.shape[1]), device="cuda"), torch.zeros((M, B, n_in), device="cuda")
            status = np.full(M, -1, np.int32)
            opts = cnf.base_icnf._solve_opts(icnf, icnf.tspan)
            rc = l.cnf_inference_path_vjp_many(h, _lib.MODE_TRAIN if case.train else _lib.MODE_TEST, M, pr.data_ptr(), xr.data_ptr(),
                                               er.data_ptr() if case.train else None, B, C.byref(opts), sv.ctypes.data, 2, 0, cm.data_ptr(),
                                               None, lp2.data_ptr(), rg2.data_ptr(), None, g2.data_ptr(), gx2.data_ptr(), status.ctypes.data,
                                               None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            assert rc == _lib.OK and not status.any()
            assert np.array_equal(_np(g2), got["grad"]) and np.array_equal(_np(lp2), got["logpx"])
            assert np.array_equal(_np(gx2)[:, :, :case.cfg.nvars].transpose(0, 2, 1), got["gin"])
    helpers.note(f"ensemble path vjp without a path cotangent vs the ensemble vjp, {name}: gradients differ by {worst:.2e} of their scale")
    assert worst <= V.RTOL, worst
    icnf.close()


@pytest.mark.parametrize("name", ["path-readme-vjp-B33", "path-regr-test-B17"])
def test_autograd_is_one_forward_and_one_backward_ensemble_call(name):
    case = BY[name]
    icnf = _icnf(case)
    ps, xs, z0, eps = _inputs(name)
    mode = _mode(case.train)
    # a loss over z (M, K, ...) and dlogp of the inference direction
    first, shared, own = _save_time_sets(icnf, case, False)
    K = own.shape[1]
    cots = _member_cots(case, K, False, "all")
    cots = [(c * np.array([1, 0, 0, 0], np.float32)[:, None], {k: v for k, v in pc.items() if k in ("z", "dlogp")}) for c, pc in cots]
    pt, xt = _dev(ps).requires_grad_(True), _dev(xs).requires_grad_(True)
    lp, regs, path = cnf.differentiable_inference_path_many(icnf, mode, xt, pt, {}, saveat=own, eps=_dev(eps) if case.train else None)
    assert tuple(path["z"].shape) == (M, K, case.cfg.n_in, case.B) and tuple(path["dlogp"].shape) == (M, K, case.B)
    fi = icnf.last_forward_info
    assert fi["launches"] == 1 and fi["calls"] == 1 and not fi["rerun"]
    wz, wd, wl = (_dev(np.stack([c[1]["z"] for c in cots])), _dev(np.stack([c[1]["dlogp"] for c in cots])),
                  _dev(np.stack([c[0][0] for c in cots])))
    obj = (wz * path["z"]).sum() + (wd * path["dlogp"]).sum() + (wl * lp).sum()
    g_ps, g_xs = torch.autograd.grad(obj, (pt, xt))
    bi = icnf.last_backward_info
    assert bi["launches"] == 2 and bi["calls"] == 1 and not bi["rerun"]
    got = _vjp(icnf, case, False, own, cots)
    assert np.array_equal(_np(g_ps), got["grad"]) and np.array_equal(_np(g_xs), got["gin"])
    # a loss over logq (M, K, n) and z of the sampling direction, into ps and a z0 that requires grad
    first, shared, own = _save_time_sets(icnf, case, True)
    K = own.shape[1]
    cots = _member_cots(case, K, True, "all")
    nv = case.cfg.nvars
    for (cz, cl), _ in cots:
        cz[nv:] = 0                                        # (xs has nvars rows)
    pt, zt = _dev(ps).requires_grad_(True), _dev(z0).requires_grad_(True)
    x, lq, path = cnf.differentiable_generate_path_many(icnf, mode, pt, {}, case.B, saveat=own, z0=zt, eps=_dev(eps))
    assert tuple(path["logq"].shape) == (M, K, case.B) and tuple(path["z"].shape) == (M, K, case.cfg.n_in, case.B)
    fi = icnf.last_forward_info
    assert fi["launches"] == 2 and fi["calls"] == 1 and not fi["rerun"]
    obj = (_dev(np.stack([c[1]["z"] for c in cots])) * path["z"]).sum() + (_dev(np.stack([c[1]["logq"] for c in cots])) * path["logq"]).sum() + \
        (_dev(np.stack([c[0][1] for c in cots])) * lq).sum() + (_dev(np.stack([c[0][0][:nv] for c in cots])) * x).sum()
    g_ps, g_z0 = torch.autograd.grad(obj, (pt, zt))
    bi = icnf.last_backward_info
    assert bi["launches"] == 4 and bi["calls"] == 1 and not bi["rerun"]
    got = _vjp(icnf, case, True, own, cots)
    assert np.array_equal(_np(g_ps), got["grad"]) and np.array_equal(_np(g_z0), got["gin"])
    icnf.close()


def test_above_the_capacity_the_members_are_split_and_the_c_call_refuses():
    """M = capacity + 1 at B = 16, K = 2: two calls whose result equals the two parts called separately, bit for bit; the C call
    itself returns CNF_ERR_UNSUPPORTED with the outputs untouched."""
    case = BY["path-readme-vjp-B33"]
    icnf = _icnf(case)
    T = cnf.TrainMode()
    B, K, n_in, D = 16, 2, 2, 5
    t0, t1 = icnf.tspan
    sv = np.asarray([t0, t1], np.float32)
    base = _inputs(case.name)[0][0]
    l, h = _lib.lib(), icnf.handle()
    for vjp, cap in ((False, cnf.ensemble_path_capacity(icnf, T, B)), (True, cnf.ensemble_path_vjp_capacity(icnf, T, B))):
        assert cap >= M
        Mx = cap + 1
        rng = np.random.default_rng(77)
        ps = _dev(base[None] * (1 + 0.1 * rng.standard_normal((Mx, 1))).astype(np.float32))
        xs, eps = _dev(rng.standard_normal((Mx, 1, B))), _dev(rng.standard_normal((Mx, n_in, B)))
        pc = {"z": _dev(rng.standard_normal((Mx, K, n_in, B)) / B)}

        def call(lo, hi):
            if vjp:
                r = cnf.inference_path_vjp_many(icnf, T, xs[lo:hi], ps[lo:hi], {}, saveat=sv, path_cot={"z": pc["z"][lo:hi]}, eps=eps[lo:hi])
                return [r[0], r[2]["z"], r[2]["dlogp"], r[3]], r[4]
            r = cnf.inference_path_many(icnf, T, xs[lo:hi], ps[lo:hi], {}, saveat=sv, eps=eps[lo:hi])
            return [r[0], r[2]["z"], r[2]["dlogp"]], r[3]

        whole, info = call(0, Mx)
        assert info["calls"] == 2 and info["launches"] == (2 if vjp else 1) and len(info["steps"]) == Mx
        a, ia = call(0, cap)
        b, ib = call(cap, Mx)
        assert ia["calls"] == ib["calls"] == 1
        for w, pa, pb in zip(whole, a, b):
            assert torch.equal(w[:cap], pa) and torch.equal(w[cap:], pb)
        for i in (0, cap - 1):
            assert all(np.array_equal(p, q) for p, q in zip(info["steps"][i], ia["steps"][i]))
        assert all(np.array_equal(p, q) for p, q in zip(info["steps"][cap], ib["steps"][0]))
        # the C call: refused with nothing enqueued
        xr, er = xs.permute(0, 2, 1).contiguous(), eps.permute(0, 2, 1).contiguous()
        lp, rg = torch.full((Mx, B), 7.0, device="cuda"), torch.full((Mx, 3, B), 7.0, device="cuda")
        pth, g = torch.full((Mx, K, B, D), 7.0, device="cuda"), torch.full((Mx, ps.shape[1]), 7.0, device="cuda")
        status = np.full(Mx, -1, np.int32)
        opts = cnf.base_icnf._solve_opts(icnf, icnf.tspan)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if vjp:
            rc = l.cnf_inference_path_vjp_many(h, _lib.MODE_TRAIN, Mx, ps.data_ptr(), xr.data_ptr(), er.data_ptr(), B, C.byref(opts),
                                               sv.ctypes.data, K, 0, None, None, lp.data_ptr(), rg.data_ptr(), pth.data_ptr(), g.data_ptr(), None,
                                               status.ctypes.data, None, st)
        else:
            rc = l.cnf_inference_path_many(h, _lib.MODE_TRAIN, Mx, ps.data_ptr(), xr.data_ptr(), er.data_ptr(), B, C.byref(opts), None,
                                           lp.data_ptr(), rg.data_ptr(), None, status.ctypes.data, None, 0, st, sv.ctypes.data, K, 0, pth.data_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.ERR_UNSUPPORTED and (status == -1).all()
        assert all(bool((t == 7.0).all()) for t in (lp, rg, pth, g))
        assert l.cnf_ensemble_path_steps(h, 0, None, None, 0) == -1
    icnf.close()


def test_members_that_give_up_are_rerun_alone():
    """poll_limit = 1 (the knob of the existing fallback tests: a bounded wait, not a fault): with three tiles per member the
    meetings run out for at least one member; those members are run again alone on the single-model calls, and every member, run
    again or not, meets the reference; a second call needs no rerun."""
    case = BY["path-regr-jvp-B33"]
    icnf = _icnf(case)
    ps, xs, z0, eps = _inputs(case.name)
    mode = _mode(case.train)
    for sampling in (False, True):
        first, shared, own = _save_time_sets(icnf, case, sampling)
        cots = _member_cots(case, own.shape[1], sampling, "all")
        pcs = {k: _dev(np.stack([c[1][k] for c in cots])) for k in cots[0][1]}
        if sampling:
            cot = (_dev(np.stack([c[0][0] for c in cots])), _dev(np.stack([c[0][1] for c in cots])))
            plain = lambda: cnf.generate_path_many(icnf, mode, _dev(ps), {}, case.B, saveat=own, z0=_dev(z0), eps=_dev(eps))
            vjp = lambda: cnf.generate_path_vjp_many(icnf, mode, _dev(ps), {}, case.B, saveat=own, cot=cot, path_cot=pcs, z0=_dev(z0),
                                                     eps=_dev(eps), with_z0=True)
        else:
            st = np.stack([c[0] for c in cots])
            cot = (_dev(st[:, 0]), tuple(_dev(st[:, r]) for r in (1, 2, 3)))
            plain = lambda: cnf.inference_path_many(icnf, mode, _dev(xs), _dev(ps), {}, saveat=own, eps=_dev(eps))
            vjp = lambda: cnf.inference_path_vjp_many(icnf, mode, _dev(xs), _dev(ps), {}, saveat=own, cot=cot, path_cot=pcs, eps=_dev(eps),
                                                      with_x=True)
        icnf.set_solve_wait(poll_limit=1)
        try:
            rp, rv = plain(), vjp()
        finally:
            icnf.set_solve_wait(poll_limit=0x7fffffff)
        # (which members' tiles miss each other within one poll is a matter of timing: at least one does, and whoever does or
        # does not, every member meets the reference below)
        for r in (rp, rv):
            assert r[-1]["rerun"] and set(r[-1]["rerun"]) <= set(range(M)), r[-1]["rerun"]
            assert all(s == _lib.OK for s in r[-1]["status"])
        gp = {"path": _state_path(rp[2], case.train), "steps": rp[-1]["steps"]}
        gv = {"path": _state_path(rv[2], case.train), "steps": rv[-1]["steps"], "grad": _np(rv[3]), "gin": _np(rv[4])}
        if sampling:
            for d, r in ((gp, rp), (gv, rv)):
                d.update(x=_np(r[0]), logq=_np(r[1]), logq_path=_np(r[2]["logq"]))
        else:
            for d, r in ((gp, rp), (gv, rv)):
                d.update(logpx=_np(r[0]), regs=np.stack([_np(a) for a in r[1]], axis=1))
        for m in range(M):
            what = f"ensemble path rerun {'sampling' if sampling else 'inference'} member {m}"
            _check_member(case, sampling, gp, m, own[m], None, None, what + " plain", grads=False)
            _check_member(case, sampling, gv, m, own[m], cots[m][0], cots[m][1], what + " vjp", grads=True)
        assert not plain()[-1]["rerun"] and not vjp()[-1]["rerun"]
    icnf.close()


def test_the_handle_afterwards_is_what_it_was():
    """A single-model ``inference``, ``loss_and_grad`` and ``inference_path_vjp`` on the same model before and after the ensemble
    path calls return identical bits, and the steps of the single-model path calls are not overwritten by the ensemble calls'."""
    case = BY["path-readme-vjp-B33"]
    icnf = _icnf(case)
    T = cnf.TrainMode()
    ps, xs, z0, eps = _inputs(case.name)
    span = case.cfg.tspan
    sv1 = np.asarray([span[0], 0.5 * (span[0] + span[1]), span[1]], np.float32)

    def singles():
        lp, rg = cnf.inference(icnf, T, _dev(xs[0]), ps[0], {}, eps=_dev(eps[0]))
        val, g = cnf.loss_and_grad(icnf, T, _dev(xs[0]), ps[0], {}, eps=_dev(eps[0]))
        r = cnf.inference_path_vjp(icnf, T, _dev(xs[0]), _dev(ps[0]), {}, saveat=sv1, path_cot={"z": torch.ones((3, 2, case.B), device="cuda")},
                                   eps=_dev(eps[0]))
        return [_np(lp)] + [_np(a) for a in rg] + [np.asarray(val), _np(torch.as_tensor(g)), _np(r[0]), _np(r[2]["z"]), _np(r[3])]

    before = singles()
    cnf.inference_path(icnf, T, _dev(xs[0]), ps[0], {}, saveat=sv1, eps=_dev(eps[0]))
    steps_plain, steps_vjp = cnf.path.path_steps(icnf), cnf.path_vjp_steps(icnf)
    assert steps_plain is not None and steps_vjp is not None
    first, shared, own = _save_time_sets(icnf, case, False)
    cots = _member_cots(case, own.shape[1], False, "all")
    _vjp(icnf, case, False, own, cots)
    _plain(icnf, case, True, np.asarray([span[1], span[0]], np.float32))
    _vjp(icnf, case, True, np.asarray([span[1], span[0]], np.float32), _member_cots(case, 2, True, "all"))
    for a, b in ((steps_plain, cnf.path.path_steps(icnf)), (steps_vjp, cnf.path_vjp_steps(icnf))):
        assert b is not None and all(np.array_equal(p, q) for p, q in zip(a, b)), "an ensemble call overwrote the single call's steps"
    after = singles()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    icnf.close()
