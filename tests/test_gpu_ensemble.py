"""Ensembles on the device: M independent models' losses and gradients from one launch (cnf_loss_grad_many,
``loss_and_grad_many``, ``fit_many``).

Reference: the float64 discrete adjoint of oracle/cnf_grad_oracle.py, replaying for every member the steps that member itself
accepted (cnf_ensemble_steps).  Bars: the ones tests/test_gpu_parity.py::test_loss_grad_wave_local_small_networks applies to one
model -- loss within ``1e-5 max(1, |ref|)``; gradient ``max |g - ref| <= 1e-4 (max |ref| + rms(ref))`` (``_assert_grad`` there,
restated here).  Everything else is exact: permutations, isolation and splits are compared bit for bit.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from oracle import cnf_grad_oracle as G
from oracle import cnf_oracle as O
from tests import helpers
from tests.helpers import make_icnf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TANH2 = (O.ACT_TANH,) * 2
README = O.Cfg(O.Net((2, 6, 2), TANH2), 1, 1, 1e-2, 1e-2, 1e-2)
REGR = O.Cfg(O.Net((16, 48, 16), TANH2), 8, 8, 1e-2, 1e-2, 1e-2)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _mode(train):
    return cnf.TrainMode() if train else cnf.TestMode()


def _assert_grad(grad, rgrad, what, rtol=1e-4):
    assert np.isfinite(grad).all(), what
    scale = np.sqrt(np.mean(rgrad ** 2))
    err = np.abs(grad - rgrad).max()
    assert err <= rtol * (np.abs(rgrad).max() + scale), (what, err, np.abs(rgrad).max(), scale)


def _cfg(cfg, tspan=None, jvp=False):
    return O.Cfg(cfg.net, cfg.nvars, cfg.naugs, cfg.lam1, cfg.lam2, cfg.lam3, use_jvp=jvp, tspan=tspan or cfg.tspan)


def _members(cfg, M, B, seed, scale=0.5):
    """Different parameters, data and probes per member."""
    rng = np.random.default_rng(seed)
    ps = np.stack([O.glorot_params(cfg.net, rng, np.float32, scale) for _ in range(M)])
    xs = rng.standard_normal((M, cfg.nvars, B)).astype(np.float32)
    eps = rng.standard_normal((M, cfg.n_in, B)).astype(np.float32)
    return ps, xs, eps


def _many(icnf, train, xs, ps, eps, **kw):
    val, grad, info = cnf.loss_and_grad_many(icnf, _mode(train), _dev(xs), _dev(ps), {}, eps=_dev(eps) if train else None,
                                             with_steps=True, **kw)
    return val, grad.cpu().numpy(), info


def _oracle(cfg, train, jvp, ps, xs, eps, dts, t1=None):
    c64 = _cfg(cfg, (cfg.tspan[0], float(t1)) if t1 is not None else None, jvp)
    f64 = lambda a: a.astype(np.float64)
    dts = [float(d) for d in dts]
    if train:
        return G.loss_and_grad(c64, f64(ps), f64(xs), f64(eps), None, dts=dts)[:2]
    return G.loss_and_grad_test(c64, f64(ps), f64(xs), None, dts=dts)[:2]


def _check_members(cfg, train, jvp, ps, xs, eps, val, grad, info, what, t1=None):
    for m in range(ps.shape[0]):
        rval, rgrad = _oracle(cfg, train, jvp, ps[m], xs[m], eps[m], info["steps"][m], None if t1 is None else t1[m])
        assert len(info["steps"][m]) == info["stats"][m]["naccept"] > 0, (what, m)
        assert abs(val[m] - rval) <= 1e-5 * max(1.0, abs(rval)), (what, m, val[m], rval)
        _assert_grad(grad[m], rgrad, f"{what}, member {m}")


# (network, tspan, M, B, train, jvp, sol_kwargs): every network, M in {1, 2, 5}, B in {1, 16, 17, 33}, the three modes, fixed and
# adaptive steps (README tolerances = the defaults; tspan (0, 13) once), lambda3 with augmentation and without
CASES = [
    (README, (0.0, 13.0), 5, 33, True, False, dict()),
    (README, None, 1, 33, True, True, dict()),
    (README, None, 2, 16, False, False, dict(adaptive=False, dt=1 / 5)),
    (REGR, None, 2, 17, True, False, dict()),
    (REGR, None, 2, 16, True, True, dict(adaptive=False, dt=1 / 6)),
    (REGR, None, 2, 33, False, False, dict()),
    (O.Cfg(O.Net((16, 64, 16), TANH2), 10, 6, 0.0, 1e-2, 5e-2), None, 5, 1, True, False, dict(adaptive=False, dt=1 / 5)),
    (O.Cfg(O.Net((7, 13, 7), TANH2), 4, 3, 1e-2, 1e-2, 1e-2), (1.0, 0.0), 2, 17, True, False, dict(adaptive=False, dt=1 / 4)),
    (O.Cfg(O.Net((7, 13, 7), TANH2), 7, 0, 1e-2, 1e-2, 0.0), (1.0, 0.0), 1, 16, False, False, dict(adaptive=False, dt=1 / 4)),
    (O.Cfg(O.Net((6, 1, 6), (O.ACT_TANH, O.ACT_IDENTITY)), 6, 0, 1e-2, 1e-2, 0.0), None, 5, 33, True, False, dict(adaptive=False, dt=1 / 5)),
    (O.Cfg(O.Net((6, 1, 6), (O.ACT_TANH, O.ACT_IDENTITY)), 6, 0, 1e-2, 1e-2, 0.0), None, 2, 17, True, True, dict()),
    (O.Cfg(O.Net((6, 1, 6), (O.ACT_TANH, O.ACT_IDENTITY)), 6, 0, 0.0, 0.0, 0.0), None, 1, 16, False, False, dict(adaptive=False, dt=1 / 5)),
]


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_each_member_matches_the_float64_adjoint_on_its_own_steps(ci):
    cfg, tspan, M, B, train, jvp, sol_kw = CASES[ci]
    cfg = _cfg(cfg, tspan)
    icnf = make_icnf(cnf, cfg, jvp=jvp, kernel="mfma", sol_kwargs=dict(sol_kw))
    assert cnf.ensemble_capacity(icnf, _mode(train), B) >= M
    ps, xs, eps = _members(cfg, M, B, 1000 + ci)
    val, grad, info = _many(icnf, train, xs, ps, eps)
    what = f"ensemble {cfg.net.dims} M={M} B={B} {'train' if train else 'test'}{' jvp' if jvp else ''}"
    # (counted by the driver where it launches: the ensemble kernel and the sum of the partials, whatever M)
    assert info["launches"] == 2 and info["calls"] == 1 and not info["rerun"], (what, info)
    assert all(s["launches"] == 2 for s in info["stats"])
    assert (info["status"] == _lib.OK).all()
    _check_members(cfg, train, jvp, ps, xs, eps, val, grad, info, what)
    helpers.note(f"{what}: steps {[s['naccept'] for s in info['stats']]}, {info['launches']} launches")
    icnf.close()


def test_members_run_their_own_controllers():
    """One stiff member (parameters x 3 of a first step of half the span: rejected attempts) beside two easy ones."""
    cfg = _cfg(REGR, (0.0, 6.0))
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(dt=3.0, reltol=1e-4, abstol=1e-6))
    rng = np.random.default_rng(925)
    ps = np.stack([O.glorot_params(cfg.net, rng, np.float32, s) for s in (3.0, 0.2, 0.2)])
    _, xs, eps = _members(cfg, 3, 40, 926)
    val, grad, info = _many(icnf, True, xs, ps, eps)
    st = info["stats"]
    assert st[0]["nreject"] >= 2, st
    assert len({s["naccept"] for s in st}) > 1, st
    assert not info["rerun"]
    _check_members(cfg, True, False, ps, xs, eps, val, grad, info, "independent controllers")
    icnf.close()


def test_offsets_are_exact():
    """Permuting the members permutes everything bit for bit; one member's data touches no other member; calls repeat."""
    cfg = _cfg(REGR)
    icnf = make_icnf(cnf, cfg, kernel="mfma")
    M, B = 3, 17
    ps, xs, eps = _members(cfg, M, B, 77)
    val, grad, info = _many(icnf, True, xs, ps, eps)
    val2, grad2, info2 = _many(icnf, True, xs, ps, eps)
    assert np.array_equal(val, val2) and np.array_equal(grad, grad2)
    perm = [2, 0, 1]
    valp, gradp, infop = _many(icnf, True, xs[perm], ps[perm], eps[perm])
    assert np.array_equal(valp, val[perm]) and np.array_equal(gradp, grad[perm])
    for i, p in enumerate(perm):
        assert np.array_equal(infop["steps"][i], info["steps"][p])
    xs_b = xs.copy()
    xs_b[1] = xs_b[1] * 1.5 + 0.25
    valb, gradb, infob = _many(icnf, True, xs_b, ps, eps)
    for m in (0, 2):
        assert valb[m] == val[m] and np.array_equal(gradb[m], grad[m]) and np.array_equal(infob["steps"][m], info["steps"][m])
    assert valb[1] != val[1]
    icnf.close()


def test_member_agrees_with_the_single_model_call():
    """Fixed dt: both the ensemble's member and ``loss_and_grad`` on the same inputs meet the bar against the oracle (and
    the figures say whether they are the same bits)."""
    cfg = _cfg(REGR)
    sol_kw = dict(adaptive=False, dt=1 / 6)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=sol_kw)
    M, B = 2, 33
    ps, xs, eps = _members(cfg, M, B, 78)
    val, grad, info = _many(icnf, True, xs, ps, eps)
    _check_members(cfg, True, False, ps, xs, eps, val, grad, info, "ensemble vs oracle")
    same = True
    for m in range(M):
        v1, g1 = cnf.loss_and_grad(icnf, cnf.TrainMode(), _dev(xs[m]), ps[m], {}, eps=_dev(eps[m]))
        g1 = g1.cpu().numpy()
        assert np.array_equal(icnf.last_steps, info["steps"][m])
        rval, rgrad = _oracle(cfg, True, False, ps[m], xs[m], eps[m], icnf.last_steps)
        assert abs(v1 - rval) <= 1e-5 * max(1.0, abs(rval))
        _assert_grad(g1, rgrad, f"single call, member {m}")
        same = same and np.float32(v1) == val[m] and np.array_equal(g1, grad[m])
    helpers.note(f"ensemble member vs loss_and_grad on the device: {'bit-identical' if same else 'NOT bit-identical'}")
    print("ensemble member vs single call bit-identical:", same)
    icnf.close()


@pytest.mark.parametrize("sol_kw", [dict(adaptive=False, dt=1 / 4), dict()], ids=["fixed", "adaptive"])
def test_per_member_end_times(sol_kw):
    cfg = _cfg(README)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(sol_kw))
    M, B = 3, 17
    ps, xs, eps = _members(cfg, M, B, 79)
    t1 = np.asarray([0.6, 1.0, 1.7], dtype=np.float32)
    val, grad, info = _many(icnf, True, xs, ps, eps, t1=t1)
    for m in range(M):
        assert abs(info["stats"][m]["t_final"] - t1[m]) <= 1e-6 and abs(np.sum(info["steps"][m], dtype=np.float64) - t1[m]) <= 1e-5
    _check_members(cfg, True, False, ps, xs, eps, val, grad, info, "per-member t1", t1=t1)
    icnf.close()


def test_steering_draws_one_end_time_per_member():
    cfg = _cfg(README)
    layers = [cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh")]
    mk = lambda: cnf.construct(cnf.RNODE, cnf.Chain(*layers), 1, 1, compute_mode=cnf.HIPVecJacMatrixMode("mfma"), tspan=(0.0, 1.0),
                               steer_rate=0.1, lambda1=1e-2, lambda2=1e-2, lambda3=1e-2, rng=11)
    icnf, twin = mk(), mk()
    M, B = 4, 16
    ps, xs, eps = _members(cfg, M, B, 80)
    val, grad, info = _many(icnf, True, xs, ps, eps)
    want = np.asarray([cnf.steer_tspan(twin, cnf.TrainMode())[1] for _ in range(M)], dtype=np.float32)
    assert np.array_equal(info["t1"], want) and len(set(want.tolist())) == M
    assert [s["t_final"] for s in info["stats"]] == want.tolist()
    _check_members(cfg, True, False, ps, xs, eps, val, grad, info, "steered members", t1=want)
    icnf.close(); twin.close()


def test_host_generator_draws_what_a_loop_of_single_calls_draws():
    """eps=None and steer_rate > 0 on a numpy generator: member by member the probes, then the end time -- the order
    ``loss_and_grad`` consumes the generator in -- so a twin model looping over the members sees the same draws."""
    cfg = _cfg(README)
    layers = [cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh")]
    mk = lambda: cnf.construct(cnf.RNODE, cnf.Chain(*layers), 1, 1, compute_mode=cnf.HIPVecJacMatrixMode("mfma"), tspan=(0.0, 1.0),
                               steer_rate=0.1, lambda1=1e-2, lambda2=1e-2, lambda3=1e-2, rng=12)
    icnf, twin = mk(), mk()
    M, B = 3, 17
    ps, xs, _ = _members(cfg, M, B, 86)
    val, grad, info = cnf.loss_and_grad_many(icnf, cnf.TrainMode(), _dev(xs), _dev(ps), {})
    for m in range(M):
        v1, _ = cnf.loss_and_grad(twin, cnf.TrainMode(), _dev(xs[m]), ps[m], {})
        assert twin.last_stats["t_final"] == float(info["t1"][m]) == info["stats"][m]["t_final"]
        assert abs(v1 - val[m]) <= 1e-5 * max(1.0, abs(v1)), (m, v1, val[m])
    assert icnf.rng.bit_generator.state == twin.rng.bit_generator.state
    icnf.close(); twin.close()


def test_device_generator_draws_all_members_probes_at_once():
    """A ``HIPRNG`` model: one draw of M B columns, viewed member by member -- the result is that of the same words passed as
    ``eps``, and members with the same parameters and data differ through their probes alone."""
    cfg = _cfg(README)
    mk = lambda: cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh")), 1, 1, lambda3=1e-2,
                               compute_mode=cnf.HIPVecJacMatrixMode("mfma"), sol_kwargs=dict(adaptive=False, dt=1 / 4), rng=cnf.HIPRNG(5))
    icnf = mk()
    M, B, n_in = 3, 17, 2
    ps, xs, _ = _members(cfg, 1, B, 87)
    ps, xs = np.repeat(ps, M, axis=0), np.repeat(xs, M, axis=0)
    val, grad, info = cnf.loss_and_grad_many(icnf, cnf.TrainMode(), _dev(xs), _dev(ps), {})
    assert val.shape == (M,) and np.isfinite(val).all() and len(set(val.tolist())) == M
    words = cnf.HIPRNG(5).normal(n_in * M * B, torch.device("cuda", 0)).view(M, B, n_in).permute(0, 2, 1)
    val2, grad2, _ = cnf.loss_and_grad_many(icnf, cnf.TrainMode(), _dev(xs), _dev(ps), {}, eps=words)
    assert np.array_equal(val, val2) and torch.equal(grad, grad2)
    icnf.close()


def test_switched_off_routes_report_capacity_zero():
    """CNF_WAVE=0, CNF_WAVE_GRAD=0 and CNF_PERSISTENT=0 are read once per process: fresh children, side by side."""
    code = ("import continuousnf.jl_amd as cnf\n"
            "ic = cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 6, 'tanh'), cnf.Dense(6, 2, 'tanh')), 1, 1, rng=1)\n"
            "print('CAPACITY', cnf.ensemble_capacity(ic, cnf.TrainMode(), 32), cnf.ensemble_capacity(ic, cnf.TestMode(), 32))\n"
            "ic.close()\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = {var: subprocess.Popen([sys.executable, "-c", code], cwd=root, env=dict(os.environ, **({var: "0"} if var else {})),
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for var in ("", "CNF_WAVE", "CNF_WAVE_GRAD", "CNF_PERSISTENT")}
    for var, p in procs.items():
        try:
            out, err = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            p.kill()
            raise
        assert p.returncode == 0, (var, err[-500:])
        caps = [int(v) for v in [l for l in out.splitlines() if l.startswith("CAPACITY")][-1].split()[1:]]
        assert (min(caps) > 0) if not var else caps == [0, 0], (var, caps)


def test_a_nonfinite_member_is_reported_alone():
    cfg = _cfg(REGR)
    icnf = make_icnf(cnf, cfg, kernel="mfma")
    M, B = 3, 17
    ps, xs, eps = _members(cfg, M, B, 81)
    val, grad, _ = _many(icnf, True, xs, ps, eps)
    bad = xs.copy()
    bad[1, 0, 3] = np.nan
    with pytest.raises(cnf.CNFError, match="member 1") as e:
        _many(icnf, True, bad, ps, eps)
    assert e.value.status == _lib.ERR_NONFINITE
    # the C ABI: the other members of that very launch are what they are beside a finite member 1
    l, h = _lib.lib(), icnf.handle()
    xr, er, pr = _dev(bad.transpose(0, 2, 1)), _dev(eps.transpose(0, 2, 1)), _dev(ps)
    g = torch.empty_like(pr)
    losses, status = np.empty(M, dtype=np.float32), np.empty(M, dtype=np.int32)
    opts = cnf.base_icnf._solve_opts(icnf, icnf.tspan)
    _lib.check(l.cnf_loss_grad_many(h, _lib.MODE_TRAIN, M, pr.data_ptr(), xr.data_ptr(), er.data_ptr(), B, C.byref(opts), None,
                                    losses.ctypes.data, g.data_ptr(), status.ctypes.data, None, None), h)
    assert status.tolist() == [_lib.OK, _lib.ERR_NONFINITE, _lib.OK] and np.isnan(losses[1])
    g = g.cpu().numpy()
    assert not g[1].any()
    for m in (0, 2):
        assert losses[m] == val[m] and np.array_equal(g[m], grad[m])
    icnf.close()


def test_members_that_give_up_are_rerun():
    """poll_limit = 1 (the knob of the existing fallback tests: a bounded wait, not a fault): with three tiles per member the
    meetings run out; the members are run again one at a time, fallbacks included, and the handle stays usable."""
    cfg = _cfg(REGR)
    sol_kw = dict(adaptive=False, dt=1 / 4)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=sol_kw)
    M, B = 2, 33
    ps, xs, eps = _members(cfg, M, B, 82)
    icnf.set_solve_wait(poll_limit=1)
    try:
        val, grad, info = _many(icnf, True, xs, ps, eps)
    finally:
        icnf.set_solve_wait(poll_limit=0x7fffffff)
    assert info["rerun"], info
    _check_members(cfg, True, False, ps, xs, eps, val, grad, info, "rerun members")
    val2, grad2, info2 = _many(icnf, True, xs, ps, eps)
    assert not info2["rerun"]
    _check_members(cfg, True, False, ps, xs, eps, val2, grad2, info2, "after the wait was restored")
    icnf.close()


def test_a_member_beyond_its_step_store_is_rerun():
    """More accepted steps than WV_GCAP = 1024: that member alone hands over (the recipe of
    test_loss_grad_wave_local_hands_over_beyond_its_step_store); the member with half the span stays in the launch."""
    cfg = O.Cfg(O.Net((6, 12, 6), TANH2), 6, 0, 1e-2, 1e-2, 0.0)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(adaptive=False, dt=1 / 1100))
    M, B = 2, 20
    ps, xs, eps = _members(cfg, M, B, 951)
    t1 = np.asarray([1.0, 0.5], dtype=np.float32)
    val, grad, info = _many(icnf, True, xs, ps, eps, t1=t1)
    assert info["rerun"] == [0] and info["stats"][0]["naccept"] == 1100 and info["stats"][1]["naccept"] == 550, info["stats"]
    _check_members(cfg, True, False, ps, xs, eps, val, grad, info, "beyond the step store", t1=t1)
    icnf.close()


def test_capacity_split_and_refusals():
    cfg = _cfg(README)
    sol_kw = dict(adaptive=False, dt=1 / 3)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=sol_kw)
    B = 16
    cap = cnf.ensemble_capacity(icnf, cnf.TrainMode(), B)
    assert cap > 0 and cnf.ensemble_capacity(icnf, cnf.TestMode(), 33) > 0
    M = cap + 1
    ps, xs, eps = _members(cfg, M, B, 83)
    # the C ABI refuses, with nothing enqueued (no array is read: these are one member's)
    l, h = _lib.lib(), icnf.handle()
    one = [_dev(a[:1]) for a in (ps, xs.transpose(0, 2, 1), eps.transpose(0, 2, 1))]
    g = torch.zeros(ps.shape[1], device="cuda")
    losses, status = np.zeros(M, dtype=np.float32), np.zeros(M, dtype=np.int32)
    opts = cnf.base_icnf._solve_opts(icnf, icnf.tspan)
    s = l.cnf_loss_grad_many(h, _lib.MODE_TRAIN, M, one[0].data_ptr(), one[1].data_ptr(), one[2].data_ptr(), B, C.byref(opts), None,
                             losses.ctypes.data, g.data_ptr(), status.ctypes.data, None, None)
    assert s == _lib.ERR_UNSUPPORTED and not g.any()
    # Python splits, and the result is that of the two parts called separately
    val, grad, info = _many(icnf, True, xs, ps, eps)
    assert info["calls"] == 2
    va, ga, _ = _many(icnf, True, xs[:cap], ps[:cap], eps[:cap])
    vb, gb, _ = _many(icnf, True, xs[cap:], ps[cap:], eps[cap:])
    assert np.array_equal(val, np.concatenate([va, vb])) and np.array_equal(grad, np.concatenate([ga, gb]))
    icnf.close()
    # what has no ensemble form is refused before anything is drawn
    lay = lambda dims: [cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])]
    models = [
        cnf.construct(cnf.CondRNODE, cnf.Chain(*lay((4, 6, 2))), 1, 1, rng=5),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((2, 6, 2))), 1, 1, rng=5, basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2)),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((2, 6, 2))), 1, 1, rng=5, compute_mode=cnf.HIPVecJacMatrixMode("generic")),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((32, 128, 128, 32))), 32, 0, rng=5),
    ]
    for ic in models:
        before = ic.rng.bit_generator.state
        x = torch.zeros((2, ic.nvars, 16), device="cuda")
        p = torch.zeros((2, ic.nn.n_params_internal), device="cuda")
        with pytest.raises(NotImplementedError):
            cnf.loss_and_grad_many(ic, cnf.TrainMode(), x, p, {})
        assert cnf.ensemble_capacity(ic, cnf.TrainMode(), 16) == 0
        assert ic.rng.bit_generator.state == before
        ic.close()


def test_the_handle_afterwards_is_what_it_was():
    cfg = _cfg(REGR)
    B = 33
    ps, xs, eps = _members(cfg, 3, B, 84)
    mine = O.glorot_params(cfg.net, np.random.default_rng(85), np.float32, 0.5)

    def own(icnf):
        v, g = cnf.loss_and_grad(icnf, cnf.TrainMode(), _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
        lp, _ = cnf.inference(icnf, cnf.TrainMode(), _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
        return v, g.cpu().numpy(), lp.cpu().numpy()

    fresh = make_icnf(cnf, cfg, kernel="mfma")
    want = own(fresh)
    fresh.close()
    icnf = make_icnf(cnf, cfg, kernel="mfma")
    first = own(icnf)
    _many(icnf, True, xs, ps, eps)
    after = own(icnf)
    for a, b in zip(want, first):
        assert np.array_equal(a, b)
    for a, b in zip(want, after):
        assert np.array_equal(a, b)
    # straight after the ensemble call, with nothing uploaded in between
    again = make_icnf(cnf, cfg, kernel="mfma")
    again.set_params(mine)
    _many(again, True, xs, ps, eps)
    lp, _ = cnf.inference(again, cnf.TrainMode(), _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
    assert np.array_equal(lp.cpu().numpy(), want[2])
    icnf.close(); again.close()


def test_fit_many_is_the_hand_written_loop():
    """The README's 1-D example (Beta(2, 4) data, 2-6-2, batches of 32), four members on their own bootstrap replicas."""
    rng = np.random.default_rng(3)
    data = rng.beta(2.0, 4.0, size=(128, 1)).astype(np.float32)
    M, n_epochs, seeds = 4, 6, [10, 11, 12, 13]
    Xs = [data[rng.integers(0, 128, size=128)] for _ in range(M)]
    mk = lambda: cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh")), 1, 1, rng=21,
                               compute_mode=cnf.HIPVecJacMatrixMode("mfma"))
    icnf = mk()
    model = cnf.ICNFModel(icnf, optimizers=(cnf.Adam(eta=2e-2),), n_epochs=n_epochs, batch_size=32)
    fitres, report = cnf.fit_many(model, 0, Xs, seeds=seeds)
    icnf.close()
    # by hand
    icnf = mk()
    gens = [np.random.default_rng(s) for s in seeds]
    ps = _dev(np.stack([cnf.setup(g, icnf.nn)[0] for g in gens]))
    x = torch.stack([_dev(X.T) for X in Xs])
    opt = cnf.Adam(eta=2e-2)
    state = opt.init(ps)
    curves = []
    for _ in range(n_epochs):
        perm = np.stack([g.permutation(128) for g in gens])
        for lo in range(0, 128, 32):
            xb = torch.stack([x[m][:, torch.from_numpy(perm[m, lo:lo + 32]).cuda()] for m in range(M)])
            val, g, _ = cnf.loss_and_grad_many(icnf, cnf.TrainMode(), xb, ps, {})
            opt.apply(state, ps, g)
            curves.append(val)
    icnf.close()
    curves = np.stack(curves, axis=1)
    assert np.array_equal(report["losses"], curves) and report["losses"].shape == (M, n_epochs * 4)
    hand = ps.cpu().numpy()
    for m in range(M):
        assert np.array_equal(fitres[m][0], hand[m])
    first, last = report["losses"][:, :4].mean(axis=1), report["losses"][:, -4:].mean(axis=1)
    print("fit_many: mean loss of the first epoch", first, "of the last", last)
    assert (last < first).all(), (first, last)
    assert len({fitres[m][0].tobytes() for m in range(M)}) == M
