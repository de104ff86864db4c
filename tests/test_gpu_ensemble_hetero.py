"""Heterogeneous ensembles on the device: per-member batch size (``counts``), regularisers (``lambdas``) and tolerances
(``reltol`` / ``abstol``) in the five ensemble calls, ``fit_many`` and ``EnsembleDist.rand(ragged=True)``
(cnf_ensemble_set_members, include/cnfhip_ensemble_hetero.h).

Cases: the network 2 -> 6 -> 2 (nvars 1, one augmented row), tspan (0, 1), M = 5 members in a rectangle of B = 40 columns with
``counts = (40, 33, 17, 16, 1)`` -- three, three, two, one and one tile: both sides of the 16 and 32 edges, a one-column member,
members whose second and third workgroups leave at once --, each member with its own lambdas and tolerances; once each also
4 -> 20 -> 4 (two hidden tiles), the JVP compute mode and TestMode.

References and bars, taken over from the existing ensemble tests unchanged:
  * the float64 oracles replaying the member's own accepted steps at the member's count, lambdas and tolerances -- the loss within
    ``1e-5 max(1, |ref|)`` and the gradient within ``1e-4 (max |ref| + rms ref)`` (tests/test_gpu_ensemble.py); ``logpx``, the
    regularisers, the samples and ``logq`` at ``helpers.assert_parity`` with the attempts replayed by
    ``ensemble_eval_ref.replay_attempts`` (tests/test_gpu_ensemble_eval.py); the two VJPs at ``vjp_ref.assert_vjp``
    (tests/test_gpu_ensemble_vjp.py, tests/test_gpu_ensemble_gen_vjp.py);
  * the existing homogeneous call with M = 1 and B = ``counts[m]`` on ``member_twin`` of the model, which passes no new argument:
    bit for bit;
  * everything else (padding, one-shot state, splits, ``fit_many`` against the hand-written loop, the default ``rand``) bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from continuousnf.jl_amd import ensemble as ens_mod
from oracle import cnf_grad_oracle as G
from oracle import cnf_oracle as O
from tests import ensemble_eval_ref as R
from tests import gen_vjp_ref as GR
from tests import grad_terms as GT
from tests import helpers
from tests import vjp_ref as V
from tests.helpers import assert_parity, make_icnf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TANH2 = (O.ACT_TANH,) * 2
COUNTS = np.asarray((40, 33, 17, 16, 1), dtype=np.int32)
M, B = len(COUNTS), int(COUNTS.max())
LAMS = np.asarray([(1e-2, 1e-2, 1e-2), (1.0, 1.0, 1.0), (0.01, 0.05, 0.2), (0.3, 0.01, 0.01), (0.05, 0.02, 0.03)], dtype=np.float32)
RELTOL = np.asarray((1e-3, 1e-4, 1e-2, 1e-3, 1e-5), dtype=np.float32)
ABSTOL = np.asarray((1e-6, 1e-7, 1e-6, 1e-5, 1e-6), dtype=np.float32)
HET = dict(counts=COUNTS, reltol=RELTOL, abstol=ABSTOL)
# name -> (network, nvars, naugs, train, jvp)
VARIANTS = {
    "base": ((2, 6, 2), 1, 1, True, False),
    "4-20-4": ((4, 20, 4), 2, 2, True, False),
    "jvp": ((2, 6, 2), 1, 1, True, True),
    "testmode": ((2, 6, 2), 1, 1, False, False),
}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _mode(train):
    return cnf.TrainMode() if train else cnf.TestMode()


def _cfg(name, lam=(1e-2, 1e-2, 1e-2), tspan=(0.0, 1.0)):
    dims, nvars, naugs, train, jvp = VARIANTS[name]
    return O.Cfg(O.Net(dims, TANH2), nvars, naugs, float(lam[0]), float(lam[1]), float(lam[2]), use_jvp=jvp, tspan=tspan)


def _icnf(name, sol_kwargs=None, **kw):
    return make_icnf(cnf, _cfg(name, **kw), jvp=VARIANTS[name][4], kernel="mfma", sol_kwargs=dict(sol_kwargs or {}))


@functools.lru_cache(maxsize=None)
def _inputs(name, seed=4100):
    """float32: ps (M, n_params), xs (M, nvars, B), eps, z0 (M, n_in, B), the cotangents cw (M, 4, B) of inference -- zero on the rows
    the mode does not integrate --, gx (M, nvars, B) and gl (M, B) of sampling.  Every member's columns are drawn full; the
    tests overwrite the ones at and behind its count."""
    cfg, train = _cfg(name), VARIANTS[name][3]
    rng = np.random.default_rng(seed + sorted(VARIANTS).index(name))
    ps = np.stack([O.glorot_params(cfg.net, rng, np.float32, 0.5) for _ in range(M)])
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    xs, eps, z0 = f32(M, cfg.nvars, B), f32(M, cfg.n_in, B), f32(M, cfg.n_in, B)
    cw = (f32(M, 4, B) / B).astype(np.float32)
    if not train:
        cw[:, 1:] = 0
    return ps, xs, eps, z0, cw, (f32(M, cfg.nvars, B) / B).astype(np.float32), (f32(M, B) / B).astype(np.float32)


def _padded(a, fill, counts=COUNTS):
    """The columns (last axis) at and behind each member's count overwritten with ``fill``."""
    a = a.copy()
    for m, k in enumerate(counts):
        a[m, ..., k:] = fill
    return a


def _run_all(icnf, name, arrays, het, members=None):
    """The five calls on the members ``members`` (default: all) of ``arrays`` -> a dict of numpy results and infos."""
    train = VARIANTS[name][3]
    sel = slice(None) if members is None else members
    ps, xs, eps, z0, cw, gx, gl = (_dev(a[sel]) for a in arrays)
    mode, e = _mode(train), dict(eps=eps) if train else {}
    lam = dict(lambdas=het["lambdas"]) if het.get("lambdas") is not None else {}
    het = {k: v for k, v in het.items() if k != "lambdas"}
    n = xs.shape[2]
    out = {}
    val, grad, info = cnf.loss_and_grad_many(icnf, mode, xs, ps, {}, with_steps=True, **e, **het, **lam)
    out["loss_grad"] = dict(val=val.copy(), grad=grad.cpu().numpy(), info=info)
    lp, regs, info = cnf.inference_many(icnf, mode, xs, ps, {}, with_steps=True, **e, **het, **lam)
    out["inference"] = dict(rows=torch.stack([lp, *regs], dim=1).cpu().numpy(), losses=info["losses"].copy(), info=info)
    x, lq = cnf.generate_many(icnf, mode, ps, {}, n, z0=z0, eps=eps, with_logp=True, with_steps=True, **het)
    out["generate"] = dict(xs=x.cpu().numpy(), logq=lq.cpu().numpy(), info=icnf.last_ensemble_info)
    lp, regs, g, dx, info = cnf.inference_vjp_many(icnf, mode, xs, ps, {}, (cw[:, 0], (cw[:, 1], cw[:, 2], cw[:, 3])), with_x=True,
                                                  with_steps=True, **e, **het)
    out["inference_vjp"] = dict(rows=torch.stack([lp, *regs], dim=1).cpu().numpy(), grad=g.cpu().numpy(), gx=dx.cpu().numpy(), info=info)
    x, lq, g, dz, info = cnf.generate_vjp_many(icnf, mode, ps, {}, n, (gx, gl), z0=z0, eps=eps, with_z0=True, with_steps=True, **het)
    out["generate_vjp"] = dict(xs=x.cpu().numpy(), logq=lq.cpu().numpy(), grad=g.cpu().numpy(), gz=dz.cpu().numpy(), info=info)
    return out


def _assert_grad(grad, rgrad, what, rtol=1e-4):
    assert np.isfinite(grad).all(), what
    scale = np.sqrt(np.mean(rgrad ** 2))
    err = np.abs(grad - rgrad).max()
    assert err <= rtol * (np.abs(rgrad).max() + scale), (what, err, np.abs(rgrad).max(), scale)


ALL_CALLS = ("loss_grad", "inference", "generate", "inference_vjp", "generate_vjp")


def _check_against_the_oracle(name, arrays, out, lams, abstol, reltol, counts=COUNTS, members=None, what="", calls=ALL_CALLS):
    """Every member of every one of the five calls (``calls``) against the float64 oracle on the member's own steps, at its own
    count, lambdas and tolerances.  No member is left out."""
    train = VARIANTS[name][3]
    ps, xs, eps, z0, cw, gx, gl = arrays
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    for i, m in enumerate(range(len(counts)) if members is None else members):
        k = int(counts[i])
        cfg = _cfg(name, lams[i])
        tol = dict(abstol=float(abstol[i]), reltol=float(reltol[i]))
        e = eps[m][:, :k] if train else None
        w = f"{what}{name} member {m} (count {k})"
        if "loss_grad" in calls:
            o = out["loss_grad"]
            dts = [float(d) for d in o["info"]["steps"][i]]
            assert len(dts) == o["info"]["stats"][i]["naccept"] > 0, w
            if train:
                rval, rgrad = G.loss_and_grad(cfg, f64(ps[m]), f64(xs[m][:, :k]), f64(e), None, dts=dts)[:2]
            else:
                rval, rgrad = G.loss_and_grad_test(cfg, f64(ps[m]), f64(xs[m][:, :k]), None, dts=dts)[:2]
            assert abs(o["val"][i] - rval) <= 1e-5 * max(1.0, abs(rval)), (w, o["val"][i], rval)
            _assert_grad(o["grad"][i], rgrad, w + " loss gradient")
        if "inference" in calls:
            o = out["inference"]
            att = o["info"]["steps"][i]
            st = o["info"]["stats"][i]
            assert len(att) == st["naccept"] + st["nreject"] > 0 and int(att[:, 3].sum()) == st["naccept"], (w, st)
            u = R.replay_attempts(cfg, train, ps[m], xs[m][:, :k], e, att, tol)
            ref, rloss = R.rows_of_state(cfg, u, train)
            assert_parity(o["rows"][i][:, :k], ref, w + ": logpx and regularisers", trace_row=0)
            assert_parity(np.asarray([o["losses"][i]]), np.asarray([rloss]), w + ": loss of inference_many")
            # ... and it is the mean over the member's own count with the member's own lambdas of what the launch itself returned
            # (the bar of tests/test_gpu_ensemble_vjp.py for a loss recomputed from logpx and the regularisers)
            r64 = o["rows"][i][:, :k].astype(np.float64)
            mine = O.loss(cfg, r64[0], tuple(r64[1:]), train)
            assert abs(mine - o["losses"][i]) <= 1e-5 * max(1.0, abs(mine)), (w, mine, o["losses"][i])
        if "generate" in calls:
            o = out["generate"]
            att = o["info"]["steps"][i]
            u0 = np.vstack([z0[m][:, :k], np.zeros((cfg.D(train) - cfg.n_in, k), dtype=np.float32)])
            crev = R.cfg_of(cfg, (cfg.tspan[1], cfg.tspan[0]), cfg.use_jvp)
            R.replay_attempts(crev, train, ps[m], None, e, att, tol, u0=u0)
            rx, rq = R.replay_generate(cfg, train, ps[m], z0[m][:, :k], e, att[att[:, 3] > 0, 1])
            assert_parity(o["xs"][i][:, :k], rx, w + ": samples")
            assert_parity(o["logq"][i][None, :k], rq[None], w + ": logq", trace_row=0)
        if "inference_vjp" in calls:
            o = out["inference_vjp"]
            dts = [float(d) for d in o["info"]["steps"][i]]
            c = cw[m][:, :k]
            r64 = V.vjp64(cfg, ps[m], xs[m][:, :k], e, c, dts, train=train)
            r32 = V.vjp32(cfg, ps[m], xs[m][:, :k], e, c, dts, train=train)
            assert_parity(o["rows"][i][0, :k], r64[0][0], w + ": logpx of the vjp launch")
            if train:
                assert_parity(o["rows"][i][1:, :k], r64[0][1:], w + ": regularisers of the vjp launch")
            V.assert_vjp(o["grad"][i], o["gx"][i][:, :k], r64[1:], r32[1:], cfg.net, w + " inference vjp")
        if "generate_vjp" in calls:
            o = out["generate_vjp"]
            dts = [float(d) for d in o["info"]["steps"][i]]
            z, q, g64, z64, _ = GR.vjp64(cfg, ps[m], z0[m][:, :k], e, gx[m][:, :k], gl[m][:k], dts, train=train)
            _, _, g32, z32, _ = GR.vjp32(cfg, ps[m], z0[m][:, :k], e, gx[m][:, :k], gl[m][:k], dts, train=train)
            assert_parity(o["xs"][i][:, :k], z[: cfg.nvars], w + ": samples of the vjp launch")
            assert_parity(o["logq"][i][None, :k], q[None], w + ": logq of the vjp launch", trace_row=0)
            V.assert_vjp(o["grad"][i], o["gz"][i][:, :k], (g64, z64), (g32, z32), cfg.net, w + " generate vjp")


@functools.lru_cache(maxsize=None)
def _hetero(name):
    """The heterogeneous call of a variant, run once and shared (its arrays: NaN behind every member's count)."""
    icnf = _icnf(name)
    arrays = tuple([_inputs(name)[0]] + [_padded(a, np.nan) for a in _inputs(name)[1:]])
    out = _run_all(icnf, name, arrays, dict(HET, lambdas=LAMS))
    icnf.close()
    return arrays, out


# ---- 1. against the float64 oracle ----
@pytest.mark.parametrize("name", list(VARIANTS))
def test_every_member_of_the_five_calls_matches_the_float64_oracle(name):
    arrays, out = _hetero(name)
    for call, o in out.items():
        info = o["info"]
        assert info["calls"] == 1 and not info["rerun"] and (info["status"] == _lib.OK).all(), (call, info)
        assert np.array_equal(info["counts"], COUNTS) and np.array_equal(info["tols"], np.stack([ABSTOL, RELTOL], axis=1)), call
    assert np.array_equal(out["loss_grad"]["info"]["lambdas"], LAMS) and np.array_equal(out["inference"]["info"]["lambdas"], LAMS)
    _check_against_the_oracle(name, arrays, out, LAMS, ABSTOL, RELTOL)
    helpers.note(f"heterogeneous ensemble {name}: accepted steps {[s['naccept'] for s in out['loss_grad']['info']['stats']]} at counts "
                 f"{COUNTS.tolist()}")


# ---- 2. against the parent's code path, bit for bit ----
@pytest.mark.parametrize("name", list(VARIANTS))
def test_every_member_is_the_homogeneous_call_of_its_twin_bit_for_bit(name):
    """Member m of the heterogeneous call = the existing call with M = 1, B = counts[m] and no new argument on a twin model made
    with the member's lambdas and sol_kwargs: losses, gradients, logpx, regulariser rows, xs, logq, grad_x, grad_z0 and steps."""
    arrays, out = _hetero(name)
    icnf = _icnf(name)
    for m in range(M):
        k = int(COUNTS[m])
        twin = cnf.member_twin(icnf, LAMS[m], (ABSTOL[m], RELTOL[m]))
        one = _run_all(twin, name, tuple([arrays[0]] + [a[..., :k] for a in arrays[1:]]), {}, members=[m])
        twin.close()
        w = f"{name} member {m}"
        for call in out:
            a, b = out[call], one[call]
            for key in a:
                if key == "info":
                    assert len(a["info"]["steps"][m]) > 0 and np.array_equal(a["info"]["steps"][m], b["info"]["steps"][0]), (w, call, "steps")
                    sa, sb = a["info"]["stats"][m], b["info"]["stats"][0]
                    assert (sa["naccept"], sa["nreject"], sa["t_final"]) == (sb["naccept"], sb["nreject"], sb["t_final"]), (w, call)
                elif key in ("val", "losses", "grad"):
                    assert np.array_equal(a[key][m], b[key][0]), (w, call, key, a[key][m], b[key][0])
                else:                                          # per-column arrays: the member's own columns
                    assert np.array_equal(a[key][m][..., :k], b[key][0]), (w, call, key)
                    assert np.isfinite(b[key][0]).all(), (w, call, key)
    icnf.close()


# ---- 3. padding is never read ----
def test_padding_is_never_read_and_never_written():
    """NaN and zeros in the padded columns of xs, eps, z0 and every cotangent give identical bits; value outputs there are NaN,
    input gradients 0."""
    name = "base"
    arrays, out = _hetero(name)                                # (NaN padding)
    icnf = _icnf(name)
    zeros = tuple([_inputs(name)[0]] + [_padded(a, 0.0) for a in _inputs(name)[1:]])
    other = _run_all(icnf, name, zeros, dict(HET, lambdas=LAMS))
    icnf.close()
    for call in out:
        for key, a in out[call].items():
            if key == "info":
                for m in range(M):
                    assert np.array_equal(a["steps"][m], other[call]["info"]["steps"][m]), (call, m)
                continue
            assert np.array_equal(a, other[call][key], equal_nan=True), (call, key)
            if key in ("val", "losses", "grad"):
                assert np.isfinite(a).all(), (call, key)
                continue
            for m, k in enumerate(COUNTS):
                live, pad = a[m][..., :k], a[m][..., k:]
                assert np.isfinite(live).all(), (call, key, m)
                assert (pad == 0).all() if key in ("gx", "gz") else np.isnan(pad).all(), (call, key, m)


# ---- 4. independent controllers ----
def test_two_tolerances_on_one_stiff_problem_take_their_own_steps():
    """The stiff case of the adaptive parity test (weights x 5, tspan (0, 2)) twice in one launch, at reltol 1e-2 and 1e-5: each
    member takes the steps its twin takes alone; the float64 oracle alone says that the two step counts differ."""
    name, tspan = "base", (0.0, 2.0)
    cfg = _cfg(name, tspan=tspan)
    rng = np.random.default_rng(4200)
    flat = (O.glorot_params(cfg.net, rng, np.float32, 0.3) * 5.0).astype(np.float32)
    k = 33
    xs, eps = rng.standard_normal((cfg.nvars, k)).astype(np.float32), rng.standard_normal((cfg.n_in, k)).astype(np.float32)
    reltol = np.asarray((1e-2, 1e-5), dtype=np.float32)
    f64 = lambda a: a.astype(np.float64)
    want = [len(O.tsit5_solve(cfg.rhs(f64(flat), f64(eps), True), O.inference_u0(cfg, f64(xs), True), *tspan, abstol=1e-6,
                              reltol=float(r))[1].dts) for r in reltol]
    assert want[1] >= 2 * want[0], want                        # (the oracle alone: the tight member takes at least twice the steps)
    icnf = _icnf(name, tspan=tspan)
    two = lambda a: np.stack([a, a])
    lp, regs, info = cnf.inference_many(icnf, cnf.TrainMode(), _dev(two(xs)), _dev(two(flat)), {}, eps=_dev(two(eps)), with_steps=True,
                                        reltol=reltol)
    val, grad, ginfo = cnf.loss_and_grad_many(icnf, cnf.TrainMode(), _dev(two(xs)), _dev(two(flat)), {}, eps=_dev(two(eps)),
                                              with_steps=True, reltol=reltol)
    acc, gacc = [s["naccept"] for s in info["stats"]], [s["naccept"] for s in ginfo["stats"]]
    assert acc[0] != acc[1] and gacc[0] != gacc[1], (acc, gacc)
    print(f"stiff member at reltol {reltol.tolist()}: accepted steps {acc} (inference), {gacc} (gradient); float64 oracle {want}")
    for m in range(2):
        twin = cnf.member_twin(icnf, tols=(1e-6, reltol[m]))
        lp1, regs1, info1 = cnf.inference_many(twin, cnf.TrainMode(), _dev(xs[None]), _dev(flat[None]), {}, eps=_dev(eps[None]), with_steps=True)
        v1, g1, ginfo1 = cnf.loss_and_grad_many(twin, cnf.TrainMode(), _dev(xs[None]), _dev(flat[None]), {}, eps=_dev(eps[None]), with_steps=True)
        twin.close()
        assert np.array_equal(info["steps"][m], info1["steps"][0]) and torch.equal(lp[m], lp1[0])
        assert np.array_equal(ginfo["steps"][m], ginfo1["steps"][0]) and val[m] == v1[0] and torch.equal(grad[m], g1[0])
    icnf.close()


# ---- 5. lambda sweep ----
def test_a_lambda_sweep_scales_each_part_of_the_gradient():
    """Three lambda rows on identical data and parameters, fixed steps (the gradient is affine in lambda for fixed steps:
    tests/grad_terms.py): every row's loss and gradient are the float64 oracle's at that row's lambdas (the bars of
    tests/test_gpu_ensemble.py), and the difference of two rows' gradients is ``sum_k (lam_a - lam_b)_k part_k`` of the oracle's
    parts -- within the sum of the two rows' own bars, which is what two gradients that each meet their bar can differ by."""
    name = "base"
    sweep = np.asarray([(1.0, 1.0, 1.0), (0.01, 0.05, 0.2), (0.3, 0.01, 0.01)], dtype=np.float32)
    sol_kw = dict(adaptive=False, dt=0.25)
    cfg = _cfg(name)
    rng = np.random.default_rng(4300)
    flat = O.glorot_params(cfg.net, rng, np.float32, 0.5)
    k = 33
    xs, eps = rng.standard_normal((cfg.nvars, k)).astype(np.float32), rng.standard_normal((cfg.n_in, k)).astype(np.float32)
    icnf = _icnf(name, sol_kwargs=sol_kw)
    three = lambda a: np.stack([a] * 3)
    val, grad, info = cnf.loss_and_grad_many(icnf, cnf.TrainMode(), _dev(three(xs)), _dev(three(flat)), {}, eps=_dev(three(eps)),
                                             with_steps=True, lambdas=sweep)
    losses = cnf.loss_many(icnf, cnf.TrainMode(), _dev(three(xs)), _dev(three(flat)), {}, eps=_dev(three(eps)), lambdas=sweep)
    plain, _, _ = cnf.loss_and_grad_many(icnf, cnf.TrainMode(), _dev(three(xs)), _dev(three(flat)), {}, eps=_dev(three(eps)))
    icnf.close()
    grad = grad.cpu().numpy().astype(np.float64)
    assert np.array_equal(info["lambdas"], sweep) and len(set(val.tolist())) == 3 and len(set(plain.tolist())) == 1
    dts = [0.25] * 4
    parts = [GT.term_reference(cfg, flat, xs, eps, None, t, dict(dts=dts)).part for t in (1, 2, 3)]
    refs = []
    for r, lam in enumerate(sweep):
        assert np.array_equal(info["steps"][r], np.asarray(dts, dtype=np.float32))
        rval, rgrad = GT.oracle_run(_cfg(name, lam), flat, xs, eps, None, dts)[:2]
        refs.append(rgrad)
        for got in (val[r], losses[r]):                        # the losses use the member's lambdas
            assert abs(got - rval) <= 1e-5 * max(1.0, abs(rval)), (r, got, rval)
        _assert_grad(grad[r], rgrad, f"lambda row {r}")
    bar = lambda g: 1e-4 * (np.abs(g).max() + np.sqrt(np.mean(g ** 2)))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        d = sweep[a].astype(np.float64) - sweep[b].astype(np.float64)
        want = sum(d[t] * parts[t] for t in range(3))
        assert np.abs(want).max() > 10 * (bar(refs[a]) + bar(refs[b]))       # (the parts are far above what the bar lets through)
        err = np.abs((grad[a] - grad[b]) - want).max()
        assert err <= bar(refs[a]) + bar(refs[b]), (a, b, err, bar(refs[a]), bar(refs[b]))


# ---- 6. one-shot state ----
def test_the_members_arrays_are_consumed_by_the_next_call():
    name = "base"
    arrays, out = _hetero(name)
    ps, xs, eps = (_inputs(name)[i] for i in range(3))
    T = cnf.TrainMode()

    def plain(icnf):
        v, g, i = cnf.loss_and_grad_many(icnf, T, _dev(xs), _dev(ps), {}, eps=_dev(eps), with_steps=True)
        lp, _, _ = cnf.inference_many(icnf, T, _dev(xs), _dev(ps), {}, eps=_dev(eps))
        return v, g.cpu().numpy(), lp.cpu().numpy(), np.concatenate(i["steps"])

    def own(icnf):
        v, g = cnf.loss_and_grad(icnf, T, _dev(xs[0]), ps[0], {}, eps=_dev(eps[0]))
        lp, _ = cnf.inference(icnf, T, _dev(xs[0]), ps[0], {}, eps=_dev(eps[0]))
        return np.float32(v), g.cpu().numpy(), lp.cpu().numpy()

    fresh = _icnf(name)
    want, want_own = plain(fresh), own(fresh)
    fresh.close()
    # a plain call after a heterogeneous one is a fresh handle's
    icnf = _icnf(name)
    het = cnf.loss_and_grad_many(icnf, T, _dev(arrays[1]), _dev(ps), {}, eps=_dev(arrays[2]), lambdas=LAMS, **HET)
    assert np.array_equal(het[0], out["loss_grad"]["val"])
    for a, b in zip(plain(icnf), want):
        assert np.array_equal(a, b)
    # cnf_ensemble_set_members followed by a call with another M: CNF_ERR_BAD_ARG, nothing enqueued, nothing left behind
    l, h = _lib.lib(), icnf.handle()
    xr, er, pr = _dev(xs.transpose(0, 2, 1)), _dev(eps.transpose(0, 2, 1)), _dev(ps)
    g = torch.zeros_like(pr)
    losses, status = np.zeros(M, dtype=np.float32), np.zeros(M, dtype=np.int32)
    opts = cnf.base_icnf._solve_opts(icnf, icnf.tspan)
    call = lambda m: l.cnf_loss_grad_many(h, _lib.MODE_TRAIN, m, pr.data_ptr(), xr.data_ptr(), er.data_ptr(), B, C.byref(opts), None,
                                          losses.ctypes.data, g.data_ptr(), status.ctypes.data, None, None)
    counts3 = np.asarray([3, 2, 1], dtype=np.int32)
    set3 = lambda: l.cnf_ensemble_set_members(h, 3, counts3.ctypes.data_as(C.POINTER(C.c_int)), None, None)
    assert set3() == _lib.OK
    assert call(M) == _lib.ERR_BAD_ARG and not g.any() and not losses.any()
    assert call(M) == _lib.OK                                  # (consumed by the call it failed: this one is a plain call)
    assert np.array_equal(losses, want[0]) and np.array_equal(g.cpu().numpy(), want[1])
    # ... a count above B, and cnf_ensemble_clear_members
    big = np.asarray([B + 1] * M, dtype=np.int32)
    assert l.cnf_ensemble_set_members(h, M, big.ctypes.data_as(C.POINTER(C.c_int)), None, None) == _lib.OK
    assert call(M) == _lib.ERR_BAD_ARG
    bad_tol = np.asarray([[1e-6, 0.0]] * M, dtype=np.float32)
    assert l.cnf_ensemble_set_members(h, M, None, None, bad_tol.ctypes.data) == _lib.OK and call(M) == _lib.ERR_BAD_ARG
    bad_lam = np.asarray([[1e-2, 0.0, 1e-2]] * M, dtype=np.float32)
    assert l.cnf_ensemble_set_members(h, M, None, bad_lam.ctypes.data, None) == _lib.OK and call(M) == _lib.ERR_BAD_ARG
    assert set3() == _lib.OK and l.cnf_ensemble_clear_members(h) == _lib.OK and call(M) == _lib.OK
    assert np.array_equal(losses, want[0]) and np.array_equal(g.cpu().numpy(), want[1])
    # loss_and_grad and inference on the handle afterwards are a fresh handle's
    for a, b in zip(own(icnf), want_own):
        assert np.array_equal(a, b)
    icnf.close()


# ---- 7. split and rerun ----
def test_a_split_above_the_capacity_slices_the_members_arrays(monkeypatch):
    """A capacity of two members per launch (the existing tests' trick): M = 5 is three calls, and equals the parts called
    separately -- which is the unsplit call."""
    name = "base"
    arrays, out = _hetero(name)
    monkeypatch.setattr(ens_mod, "_device_capacity", lambda *a: 2)
    icnf = _icnf(name)
    split = _run_all(icnf, name, arrays, dict(HET, lambdas=LAMS))
    parts = []
    for lo in (0, 2, 4):
        sel = list(range(lo, min(lo + 2, M)))
        parts.append(_run_all(icnf, name, arrays, dict(counts=COUNTS[sel], reltol=RELTOL[sel], abstol=ABSTOL[sel], lambdas=LAMS[sel]),
                              members=sel))
    icnf.close()
    for call in out:
        assert split[call]["info"]["calls"] == 3, call
        for key, a in out[call].items():
            if key == "info":
                for m in range(M):
                    assert np.array_equal(a["steps"][m], split[call]["info"]["steps"][m]), (call, m)
                continue
            assert np.array_equal(split[call][key], a, equal_nan=True), (call, key)
            assert np.array_equal(np.concatenate([p[call][key] for p in parts]), a, equal_nan=True), (call, key)


def test_members_that_give_up_are_rerun_with_their_own_lambdas_and_tolerances():
    """poll_limit = 1 (a bounded wait, not a fault): the members of more than one tile run out of their meetings and are run
    again one at a time -- on a twin with the member's own lambdas and tolerances, at the member's count.  The three gradient
    calls report the steps of a member that was run again: every member is held to the float64 oracle at ITS lambdas and
    tolerances, as in the first test.  ``inference_many`` and ``generate_many`` report none for such a member: it is compared with
    the launch's own result at the 5e-3 at which the suite compares two solves with their own step sequences
    (``ensemble_eval_ref.RESCORE_RTOL``, at tolerances of 1e-5 and tighter, as there)."""
    name = "base"
    arrays = _hetero(name)[0]
    reltol, abstol = np.asarray((1e-5, 2e-6, 1e-6, 1e-5, 1e-5), dtype=np.float32), np.asarray((1e-7, 1e-7, 2e-7, 1e-7, 1e-7), dtype=np.float32)
    het = dict(counts=COUNTS, reltol=reltol, abstol=abstol, lambdas=LAMS)
    icnf = _icnf(name)
    ref = _run_all(icnf, name, arrays, het)
    icnf.set_solve_wait(poll_limit=1)
    try:
        got = _run_all(icnf, name, arrays, het)
    finally:
        icnf.set_solve_wait(poll_limit=0x7fffffff)
    for call, o in got.items():
        rerun = o["info"]["rerun"]
        assert rerun and set(rerun) <= {0, 1, 2} and not ref[call]["info"]["rerun"], (call, rerun)     # (one-tile members have nobody to wait for)
        assert (o["info"]["status"] == _lib.OK).all()
        for key in ("counts", "lambdas", "tols"):
            assert np.array_equal(o["info"][key], ref[call]["info"][key])
    _check_against_the_oracle(name, arrays, got, LAMS, abstol, reltol, what="rerun: ", calls=("loss_grad", "inference_vjp", "generate_vjp"))
    # the member's own tolerances: the launch takes n_own accepted steps at them (``ref``) and n_model at the model's own (the same
    # call without ``reltol`` / ``abstol``); the member that was run again is nearer the first
    a = arrays
    model_tols = cnf.loss_and_grad_many(icnf, cnf.TrainMode(), _dev(a[1]), _dev(a[0]), {}, eps=_dev(a[2]), with_steps=True, counts=COUNTS,
                                        lambdas=LAMS)[2]
    for i in got["loss_grad"]["info"]["rerun"]:
        n_own, n_model = len(ref["loss_grad"]["info"]["steps"][i]), len(model_tols["steps"][i])
        n = len(got["loss_grad"]["info"]["steps"][i])
        assert n_own != n_model and abs(n - n_own) < abs(n - n_model), (i, n, n_own, n_model)
    for call, keys in (("inference", ("rows", "losses")), ("generate", ("xs", "logq"))):
        for i in range(M):
            k = int(COUNTS[i])
            for key in keys:
                a, b = got[call][key][i], ref[call][key][i]
                if i not in got[call]["info"]["rerun"]:
                    assert np.array_equal(a, b, equal_nan=True), (call, key, i)
                    continue
                if key != "losses":
                    assert np.isnan(a[..., k:]).all(), (call, key, i)
                    a, b = a[..., :k], b[..., :k]
                assert_parity(np.atleast_2d(a), np.atleast_2d(b), f"rerun member {i}: {key} of {call} against the launch's",
                              rtol=R.RESCORE_RTOL, trace_row=0 if key in ("rows", "logq") else None)
    for call, keys in (("inference_vjp", ("rows", "gx")), ("generate_vjp", ("xs", "logq", "gz"))):
        for i in got[call]["info"]["rerun"]:
            k = int(COUNTS[i])
            for key in keys:
                pad = got[call][key][i][..., k:]
                assert (pad == 0).all() if key in ("gx", "gz") else np.isnan(pad).all(), (call, key, i)
    # the handle stays usable: the same call again is the launch's
    again = _run_all(icnf, name, arrays, het)
    icnf.close()
    for call in ALL_CALLS:
        assert not again[call]["info"]["rerun"]
    assert np.array_equal(again["loss_grad"]["grad"], ref["loss_grad"]["grad"])


# ---- 8. fit_many ----
def test_fit_many_on_ragged_data_sets_is_the_hand_written_loop():
    """Data sets of 64, 63 and 62 rows at batch_size 32 with three lambda rows: bit for bit a loop of ragged ``loss_and_grad_many``
    calls and optimiser steps.  ``fit`` of a member's twin alone draws its initialisation, shuffles and probes from ONE generator
    where ``fit_many`` gives every member its own for the first two, so no bits can be compared; both are held to what
    tests/test_gpu_ensemble.py asks of ``fit_many``: the mean loss of the last epoch is below the first's."""
    rng = np.random.default_rng(5)
    ns, n_epochs, seeds = (64, 63, 62), 6, [10, 11, 12]
    Xs = [rng.beta(2.0, 4.0, size=(n, 1)).astype(np.float32) for n in ns]
    lams = np.asarray([(1e-2, 1e-2, 1e-2), (0.05, 0.02, 0.03), (0.1, 0.05, 0.02)], dtype=np.float32)
    mk = lambda: cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh")), 1, 1, rng=21, lambda3=1e-2,
                               compute_mode=cnf.HIPVecJacMatrixMode("mfma"))
    icnf = mk()
    model = cnf.ICNFModel(icnf, optimizers=(cnf.Adam(eta=2e-2),), n_epochs=n_epochs, batch_size=32)
    fitres, report = cnf.fit_many(model, 0, Xs, seeds=seeds, lambdas=lams)
    icnf.close()
    # by hand
    icnf = mk()
    gens = [np.random.default_rng(s) for s in seeds]
    ps = _dev(np.stack([cnf.setup(g, icnf.nn)[0] for g in gens]))
    x = [_dev(X.T) for X in Xs]
    opt = cnf.Adam(eta=2e-2)
    state = opt.init(ps)
    curves = []
    for _ in range(n_epochs):
        perm = [g.permutation(n) for g, n in zip(gens, ns)]
        for lo in (0, 32):
            cols = [x[m][:, torch.from_numpy(perm[m][lo:lo + 32]).cuda()] for m in range(3)]
            cnt = np.asarray([c.shape[1] for c in cols])
            xb = cnf.pad_columns(cols, int(cnt.max()), float("nan"))
            val, g, info = cnf.loss_and_grad_many(icnf, cnf.TrainMode(), xb, ps, {}, lambdas=lams, counts=cnt if lo else None)
            assert info["counts"].tolist() == ([32, 31, 30] if lo else [32, 32, 32])
            opt.apply(state, ps, g)
            curves.append(val)
    icnf.close()
    curves = np.stack(curves, axis=1)
    assert np.array_equal(report["losses"], curves) and report["losses"].shape == (3, n_epochs * 2)
    hand = ps.cpu().numpy()
    for m in range(3):
        assert np.array_equal(fitres[m][0], hand[m])
    first, last = report["losses"][:, :2].mean(axis=1), report["losses"][:, -2:].mean(axis=1)
    assert (last < first).all(), (first, last)
    for m in range(3):
        base = mk()
        twin = cnf.member_twin(base, lams[m])
        _, _, rep = cnf.fit(cnf.ICNFModel(twin, optimizers=(cnf.Adam(eta=2e-2),), n_epochs=n_epochs, batch_size=32), 0, Xs[m])
        twin.close(); base.close()
        f1, l1 = rep["losses"][:2].mean(), rep["losses"][-2:].mean()
        print(f"fit_many member {m}: first / last epoch {first[m]:.5f} / {last[m]:.5f}; fit of its twin alone {f1:.5f} / {l1:.5f}")
        assert l1 < f1, (m, f1, l1)


# ---- 9. EnsembleDist.rand(n, ragged=True) ----
def test_ragged_rand():
    name, n = "base", 64
    ps = _inputs(name)[0]
    T = cnf.TestMode()
    # (no augmentation, as in the re-scoring test of tests/test_gpu_ensemble_eval.py: logq is then the density of the sample itself)
    mk = lambda seed=31: cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh")), 2, 0, rng=seed,
                                       compute_mode=cnf.HIPVecJacMatrixMode("mfma"), sol_kwargs=dict(R.RESCORE_TOL))
    w = [0.4, 0.0, 0.3, 0.2, 0.1]
    # the counts come from the same multinomial draw as the default's
    a, b = mk(), mk()
    da, db = cnf.EnsembleDist(a, T, _dev(ps), {}, weights=w), cnf.EnsembleDist(b, T, _dev(ps), {}, weights=w)
    xa, ma = da.rand(n, with_members=True)
    xb, mb = db.rand(n, with_members=True, ragged=True)
    assert np.array_equal(ma, mb) and tuple(xb.shape) == (2, n) and torch.isfinite(xb).all()
    counts = np.bincount(mb, minlength=M)
    assert counts[1] == 0 and counts.sum() == n
    info = b.last_ensemble_info
    live = np.flatnonzero(counts)
    assert len(info["status"]) == len(live) and np.array_equal(info["counts"], counts[live])
    # every returned column's log-density under its own member is the logq sampling produced (the bar of the re-scoring test of
    # tests/test_gpu_ensemble_eval.py: two solves with their own step sequences at the tight tolerances)
    z0, logq = info["z0"], None
    xs2, logq = cnf.generate_many(b, T, _dev(ps[live]), {}, int(counts.max()), z0=z0.contiguous(), with_logp=True, counts=counts[live])
    got = torch.cat([xs2[j, :, :counts[i]] for j, i in enumerate(live)], dim=1)
    assert torch.equal(got, xb)                                # (the same launch again: the same samples)
    lp = db.logpdf_members(xb).cpu().numpy()
    lq = np.concatenate([logq[j, :counts[i]].cpu().numpy() for j, i in enumerate(live)])
    assert_parity(lp[mb, np.arange(n)][None], lq[None], "ragged rand: logpdf of the draws under their own member against logq",
                  rtol=R.RESCORE_RTOL, trace_row=0)
    a.close(); b.close()
    # a one-hot mixture launches one member
    c = mk()
    dc = cnf.EnsembleDist(c, T, _dev(ps), {}, weights=[0, 0, 1, 0, 0])
    xc, mc = dc.rand(n, with_members=True, ragged=True)
    assert (mc == 2).all() and len(c.last_ensemble_info["status"]) == 1 and c.last_ensemble_info["counts"].tolist() == [n]
    assert tuple(xc.shape) == (2, n)
    c.close()
    # the default rand is what it was: one generate_many of max(count) columns per member, the first count_m kept
    d, e = mk(7), mk(7)
    xd = cnf.EnsembleDist(d, T, _dev(ps), {}, weights=w).rand(n)
    cnt = ens_mod.split_counts(e.rng, n, ens_mod.check_weights(w, M))
    xe = cnf.generate_many(e, T, _dev(ps), {}, int(cnt.max()))
    assert torch.equal(xd, torch.cat([xe[i, :, :k] for i, k in enumerate(cnt)], dim=1))
    assert d.rng.bit_generator.state == e.rng.bit_generator.state
    d.close(); e.close()


# ---- 10. autograd through the heterogeneous calls ----
def test_autograd_with_counts_is_the_vjp_call_with_the_cotangents_autograd_produced():
    """``differentiable_inference_many`` and ``reverse_kl_many`` (``differentiable_generate_many``) with ``counts`` / ``reltol`` /
    ``abstol``: the forward is the heterogeneous forward call bit for bit, NaN behind the counts; a loss masked to the members'
    own columns back-propagates finite gradients, zero behind the counts, that are -- bit for bit -- ``inference_vjp_many`` /
    ``generate_vjp_many`` called with the cotangents autograd produced; ``reverse_kl_many`` is the mean over the member's own
    samples."""
    name = "base"
    arrays, out = _hetero(name)
    ps, xs, eps, z0, cw, gx, gl = arrays
    T = cnf.TrainMode()
    live = torch.arange(B, device="cuda")[None, :] < torch.as_tensor(COUNTS, device="cuda")[:, None]
    icnf = _icnf(name)
    # inference: the cotangents of _hetero's inference_vjp_many, as weights of a masked sum
    pt, xt = _dev(ps).requires_grad_(), _dev(xs).requires_grad_()
    logpx, regs = cnf.differentiable_inference_many(icnf, T, xt, pt, {}, eps=_dev(eps), **HET)
    rows = torch.stack([logpx, *regs], dim=1)
    assert np.array_equal(rows.detach().cpu().numpy(), out["inference"]["rows"], equal_nan=True)
    w = _dev(_padded(cw, 0.0))
    obj = torch.where(live[:, None, :], rows * w, torch.zeros_like(rows)).sum()
    g_ps, g_xs = torch.autograd.grad(obj, (pt, xt))
    assert torch.isfinite(g_ps).all() and torch.isfinite(g_xs).all()
    assert np.array_equal(g_ps.cpu().numpy(), out["inference_vjp"]["grad"])
    assert np.array_equal(g_xs.cpu().numpy(), out["inference_vjp"]["gx"])
    for m, k in enumerate(COUNTS):
        assert not g_xs[m, :, k:].any() and g_xs[m, :, :k].any()
    # sampling: reverse KL to a Gaussian target
    mu, sig = 0.3, 1.5
    target = lambda x: -0.5 * (((x - mu) / sig) ** 2).sum(1)
    pt, zt = _dev(ps).requires_grad_(), _dev(z0).requires_grad_()
    losses = cnf.reverse_kl_many(icnf, T, pt, {}, B, target, z0=zt, eps=_dev(eps), **HET)
    assert tuple(losses.shape) == (M,) and torch.isfinite(losses).all()
    fx, fq = out["generate"]["xs"], out["generate"]["logq"]
    for m, k in enumerate(COUNTS):                              # the mean over the member's own samples (the loss bar)
        want = np.mean(fq[m, :k].astype(np.float64) + 0.5 * (((fx[m, :, :k].astype(np.float64) - mu) / sig) ** 2).sum(0))
        assert abs(float(losses[m].detach()) - want) <= 1e-5 * max(1.0, abs(want)), (m, float(losses[m].detach()), want)
    g_ps, g_z0 = torch.autograd.grad(losses.sum(), (pt, zt))
    assert torch.isfinite(g_ps).all() and torch.isfinite(g_z0).all()
    for m, k in enumerate(COUNTS):
        assert not g_z0[m, :, k:].any() and g_z0[m, :, :k].any()
    # ... the direct call with the cotangents autograd produces for the same masked objective of the forward's outputs
    xl, ql = _dev(fx).requires_grad_(), _dev(fq).requires_grad_()
    c = torch.as_tensor(COUNTS, device="cuda")
    t = target(torch.where(live[:, None, :], xl, torch.zeros_like(xl)))
    kl = torch.where(live, ql - t, torch.zeros_like(ql)).sum(dim=1) / c.to(ql.dtype)
    cx, cq = torch.autograd.grad(kl.sum(), (xl, ql))
    for m, k in enumerate(COUNTS):
        assert np.array_equal(cq[m, :k].cpu().numpy(), np.full(k, np.float32(1.0) / np.float32(k))) and not cq[m, k:].any()
    _, _, g, gz, _ = cnf.generate_vjp_many(icnf, T, _dev(ps), {}, B, (cx, cq), z0=_dev(z0), eps=_dev(eps), with_z0=True, **HET)
    assert torch.equal(g, g_ps) and torch.equal(gz, g_z0)
    icnf.close()


# ---- 11. the draws of a host generator ----
def test_host_generator_draws_counts_columns_per_member_as_a_loop_of_single_calls_does():
    """``eps=None`` / ``z0=None`` and ``steer_rate > 0`` on a numpy generator, with ``counts``: member by member ``counts[m]`` columns
    of probes (base samples, then probes) and then the steered time, the order the single calls consume the generator in -- so a
    twin model looping the single call at ``B = counts[m]`` sees the same draws and ends with the generator in the same state."""
    layers = [cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh")]
    mk = lambda seed: cnf.construct(cnf.RNODE, cnf.Chain(*layers), 1, 1, compute_mode=cnf.HIPVecJacMatrixMode("mfma"), tspan=(0.0, 1.0),
                                    steer_rate=0.1, lambda1=1e-2, lambda2=1e-2, lambda3=1e-2, rng=seed)
    ps, xs = _inputs("base")[:2]
    T = cnf.TrainMode()
    icnf, twin = mk(12), mk(12)
    val, grad, info = cnf.loss_and_grad_many(icnf, T, _dev(_padded(xs, np.nan)), _dev(ps), {}, counts=COUNTS)
    for m, k in enumerate(COUNTS):
        v1, _ = cnf.loss_and_grad(twin, T, _dev(xs[m][:, :k]), ps[m], {})
        assert twin.last_stats["t_final"] == float(info["t1"][m]) == info["stats"][m]["t_final"]
        assert abs(v1 - val[m]) <= 1e-5 * max(1.0, abs(v1)), (m, v1, val[m])
    assert len(set(info["t1"].tolist())) == M and icnf.rng.bit_generator.state == twin.rng.bit_generator.state
    icnf.close(); twin.close()
    icnf, twin = mk(13), mk(13)
    got = cnf.generate_many(icnf, T, _dev(ps), {}, B, counts=COUNTS)
    info = icnf.last_ensemble_info
    assert len(set(info["t0"].tolist())) == M
    for m, k in enumerate(COUNTS):
        one = cnf.generate(twin, T, ps[m], {}, int(k))
        one = one.cpu().numpy() if hasattr(one, "cpu") else np.asarray(one)
        assert_parity(got[m, :, :k].cpu().numpy(), one, f"ragged sampling, member {m} against the twin's single call at its count")
        assert torch.isnan(got[m, :, k:]).all()
    assert icnf.rng.bit_generator.state == twin.rng.bit_generator.state
    icnf.close(); twin.close()
