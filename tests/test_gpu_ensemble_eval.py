"""Ensemble inference and sampling on the device: M independent models scored (cnf_inference_many, ``inference_many``,
``loss_many``) or sampled (cnf_generate_many, ``generate_many``) by one launch, and the bagged density ``EnsembleDist``.

Reference: the float64 oracle replaying, for every member, the step attempts that member itself made
(cnf_ensemble_eval_steps), at the bar of ``helpers.assert_parity``; the row derived from dlogp (logpx, logq) is the ``trace_row``
of that bar.  The inputs of every case live in tests/ensemble_eval_ref.py, where tests/test_ensemble_eval_host.py holds each to
the float32 floor with 4x to spare.  Everything else is exact: permutations, isolation, splits, repeats and the comparison with
the single call are bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from oracle import cnf_oracle as O
from tests import ensemble_eval_ref as R
from tests import helpers
from tests.helpers import assert_parity, make_icnf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _mode(train):
    return cnf.TrainMode() if train else cnf.TestMode()


def _tol(sol_kw):
    if not sol_kw.get("adaptive", True):
        return None
    t = dict(R.DEFAULT_TOL)
    t.update({k: v for k, v in sol_kw.items() if k in ("abstol", "reltol")})
    return t


def _many(icnf, train, xs, ps, eps, with_steps=True, **kw):
    """-> ((M, 4, B) rows logpx; E; n; A, losses, info)"""
    lp, regs, info = cnf.inference_many(icnf, _mode(train), _dev(xs), _dev(ps), {}, eps=_dev(eps) if train else None,
                                        with_steps=with_steps, **kw)
    rows = torch.stack([lp, *regs], dim=1).cpu().numpy()
    return rows, info["losses"].copy(), info


def _check_members(cfg, train, ps, xs, eps, rows, losses, info, what, tol, t1=None):
    for m in range(ps.shape[0]):
        att = info["steps"][m]
        st = info["stats"][m]
        assert len(att) == st["naccept"] + st["nreject"] > 0 and int(att[:, 3].sum()) == st["naccept"], (what, m, st)
        x = xs[m] if xs.ndim == 3 else xs
        u = R.replay_attempts(cfg, train, ps[m], x, eps[m], att, tol, t1=None if t1 is None else t1[m])
        ref, rloss = R.rows_of_state(cfg, u, train)
        print(f"{what}, member {m}: {helpers.parity_err(rows[m], ref, trace_row=0):.3f} of the bar, loss {losses[m]:.7g} / {rloss:.7g}")
        assert_parity(rows[m], ref, f"{what}, member {m}: logpx and regularisers on its own steps", trace_row=0)
        assert_parity(np.asarray([losses[m]]), np.asarray([rloss]), f"{what}, member {m}: loss")


@pytest.mark.parametrize("ci", range(len(R.INFERENCE_CASES)))
def test_each_member_matches_the_float64_oracle_on_its_own_steps(ci):
    cfg, tspan, M, B, train, jvp, sol_kw = R.INFERENCE_CASES[ci]
    cfg = R.cfg_of(cfg, tspan, jvp)
    icnf = make_icnf(cnf, cfg, jvp=jvp, kernel="mfma", sol_kwargs=dict(sol_kw))
    assert cnf.ensemble_eval_capacity(icnf, _mode(train), B) >= M
    ps, xs, eps = R.members(cfg, M, B, 2000 + ci)
    rows, losses, info = _many(icnf, train, xs, ps, eps)
    what = f"ensemble inference {cfg.net.dims} M={M} B={B} {'train' if train else 'test'}{' jvp' if jvp else ''}"
    assert info["launches"] == 1 and info["calls"] == 1 and not info["rerun"], (what, info)
    assert all(s["launches"] == 1 for s in info["stats"]) and (info["status"] == _lib.OK).all()
    _check_members(cfg, train, ps, xs, eps, rows, losses, info, what, _tol(sol_kw))
    assert np.array_equal(cnf.loss_many(icnf, _mode(train), _dev(xs), _dev(ps), {}, eps=_dev(eps) if train else None), losses)
    helpers.note(f"{what}: attempts {[len(s) for s in info['steps']]}, {info['launches']} launch")
    icnf.close()


def test_members_run_their_own_controllers():
    """One stiff member (parameters x 3, a first step of half the span: rejected attempts) beside two easy ones."""
    name, cfg, tspan, train, seed, M, B, scales, sol_kw = R.OTHER["stiff member"]
    cfg = R.cfg_of(cfg, tspan)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(sol_kw))
    ps, xs, eps = R.members(cfg, M, B, seed, scales=scales)
    rows, losses, info = _many(icnf, True, xs, ps, eps)
    st = info["stats"]
    assert st[0]["nreject"] >= 2, st
    assert len({s["naccept"] for s in st}) > 1, st
    assert not info["rerun"] and info["launches"] == 1
    _check_members(cfg, True, ps, xs, eps, rows, losses, info, "independent controllers", _tol(sol_kw))
    icnf.close()


def test_offsets_are_exact():
    """Permuting the members permutes every output bit for bit; one member's data or parameters touch no other member; calls
    repeat."""
    name, cfg, tspan, train, seed, M, B, scales, sol_kw = R.OTHER["offsets"]
    cfg = R.cfg_of(cfg, tspan)
    icnf = make_icnf(cnf, cfg, kernel="mfma")
    ps, xs, eps = R.members(cfg, M, B, seed)
    rows, losses, info = _many(icnf, True, xs, ps, eps)
    rows2, losses2, info2 = _many(icnf, True, xs, ps, eps)
    assert np.array_equal(rows, rows2) and np.array_equal(losses, losses2)
    perm = [2, 0, 1]
    rowsp, lossesp, infop = _many(icnf, True, xs[perm], ps[perm], eps[perm])
    assert np.array_equal(rowsp, rows[perm]) and np.array_equal(lossesp, losses[perm])
    for i, p in enumerate(perm):
        assert np.array_equal(infop["steps"][i], info["steps"][p])
    xs_b = xs.copy()
    xs_b[1] = xs_b[1] * 1.5 + 0.25
    ps_b = ps.copy()
    ps_b[2] *= 1.25
    for changed, (rb, lb, ib) in ((1, _many(icnf, True, xs_b, ps, eps)), (2, _many(icnf, True, xs, ps_b, eps))):
        for m in range(M):
            same = np.array_equal(rb[m], rows[m]) and lb[m] == losses[m] and np.array_equal(ib["steps"][m], info["steps"][m])
            assert same == (m != changed), (changed, m)
    icnf.close()


def test_capacity_split_equals_the_parts():
    cfg = R.cfg_of(R.README)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(adaptive=False, dt=1 / 3))
    B = 16
    cap = cnf.ensemble_eval_capacity(icnf, cnf.TrainMode(), B)
    assert cap > 0 and cnf.ensemble_eval_capacity(icnf, cnf.TestMode(), 33) > 0
    assert cnf.ensemble_eval_capacity(icnf, cnf.TrainMode(), 8192) >= 1 and cnf.ensemble_eval_capacity(icnf, cnf.TrainMode(), 8193) == 0
    M = cap + 1
    ps, xs, eps = R.members(cfg, M, B, 83)
    # the C ABI refuses, with nothing enqueued (no array is read: these are one member's)
    l, h = _lib.lib(), icnf.handle()
    one = [_dev(a[:1]) for a in (ps, xs.transpose(0, 2, 1), eps.transpose(0, 2, 1))]
    out = torch.zeros(4 * B, device="cuda")
    status = np.zeros(M, dtype=np.int32)
    opts = cnf.base_icnf._solve_opts(icnf, icnf.tspan)
    s = l.cnf_inference_many(h, _lib.MODE_TRAIN, M, one[0].data_ptr(), one[1].data_ptr(), one[2].data_ptr(), B, C.byref(opts), None,
                             out.data_ptr(), out[B:].data_ptr(), None, status.ctypes.data, None, 0, None)
    assert s == _lib.ERR_UNSUPPORTED and not out.any()
    s = l.cnf_generate_many(h, _lib.MODE_TRAIN, M, one[0].data_ptr(), one[2].data_ptr(), one[2].data_ptr(), B, C.byref(opts), None,
                            out.data_ptr(), out[B:].data_ptr(), status.ctypes.data, None, 0, None)
    assert s == _lib.ERR_UNSUPPORTED and not out.any()
    # Python splits, and the result is that of the two parts called separately
    rows, losses, info = _many(icnf, True, xs, ps, eps, with_steps=False)
    assert info["calls"] == 2 and info["launches"] == 1
    ra, la, _ = _many(icnf, True, xs[:cap], ps[:cap], eps[:cap], with_steps=False)
    rb, lb, _ = _many(icnf, True, xs[cap:], ps[cap:], eps[cap:], with_steps=False)
    assert np.array_equal(rows, np.concatenate([ra, rb])) and np.array_equal(losses, np.concatenate([la, lb]))
    icnf.close()


def _single_rows(icnf, train, xs, ps, eps):
    lp, regs = cnf.inference(icnf, _mode(train), _dev(xs), ps, {}, **(dict(eps=_dev(eps)) if train else {}))
    return torch.stack([lp, *regs]).cpu().numpy()


@pytest.mark.parametrize("sol_kw", [dict(adaptive=False, dt=1 / 6), dict()], ids=["fixed", "adaptive"])
def test_a_member_is_the_single_call_bit_for_bit(sol_kw):
    """B = 80 (five tiles): ``inference`` takes the one-wave-per-workgroup form whose body the ensemble form shares."""
    name, cfg, tspan, train, seed, M, B, scales, _ = R.OTHER["single call"]
    cfg = R.cfg_of(cfg, tspan)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(sol_kw))
    ps, xs, eps = R.members(cfg, M, B, seed)
    for tr in (True, False):
        rows, losses, info = _many(icnf, tr, xs, ps, eps)
        for m in range(M):
            one = _single_rows(icnf, tr, xs[m], ps[m], eps[m])
            st = icnf.last_stats
            assert (st["naccept"], st["nreject"]) == (info["stats"][m]["naccept"], info["stats"][m]["nreject"])
            assert np.array_equal(one, rows[m]), (tr, m, np.abs(one - rows[m]).max())
    icnf.close()


_CHILD = r"""
import numpy as np, torch
import continuousnf.jl_amd as cnf
from tests import ensemble_eval_ref as R
from tests.helpers import make_icnf
name, cfg, tspan, train, seed, M, B, scales, sol_kw = R.OTHER["single call, one workgroup"]
cfg = R.cfg_of(cfg, tspan)
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
ps, xs, eps = R.members(cfg, M, B, seed)
same = True
for kw in (sol_kw, dict()):
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(kw))
    lp, regs, info = cnf.inference_many(icnf, cnf.TrainMode(), dev(xs), dev(ps), {}, eps=dev(eps))
    for m in range(M):
        l1, r1 = cnf.inference(icnf, cnf.TrainMode(), dev(xs[m]), ps[m], {}, eps=dev(eps[m]))
        same = same and torch.equal(l1, lp[m]) and all(torch.equal(a, b[m]) for a, b in zip(r1, regs))
    icnf.close()
print("SAME", int(same))
"""


def _start_child(code):
    """A fresh process in which ``inference`` of a small batch takes the one-wave-per-workgroup form (CNF_WAVE_WG is read once)."""
    return subprocess.Popen([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, CNF_WAVE_WG="0"),
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _child_says_same(child):
    try:
        out, err = child.communicate(timeout=120)
    except subprocess.TimeoutExpired:
        child.kill()
        raise
    assert child.returncode == 0, err[-800:]
    assert [l for l in out.splitlines() if l.startswith("SAME")][-1] == "SAME 1", out


def test_a_member_of_a_small_batch_is_the_single_call():
    """B = 33 <= 64: in this process ``inference`` runs the waves of ONE workgroup, which meet through LDS in another form of the
    kernel: held to the parity bar here, and bit for bit in a child process with CNF_WAVE_WG=0 (read once per process)."""
    name, cfg, tspan, train, seed, M, B, scales, sol_kw = R.OTHER["single call, one workgroup"]
    cfg = R.cfg_of(cfg, tspan)
    child = _start_child(_CHILD)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(sol_kw))
    ps, xs, eps = R.members(cfg, M, B, seed)
    rows, losses, info = _many(icnf, True, xs, ps, eps)
    for m in range(M):
        assert_parity(rows[m], _single_rows(icnf, True, xs[m], ps[m], eps[m]), f"member {m} against the one-workgroup single call", trace_row=0)
    icnf.close()
    _child_says_same(child)


def test_a_long_solve_keeps_its_first_attempts():
    """More attempts than rows of trace (1024): the member's statistics count them all, its steps are the rows that were kept."""
    cfg = R.cfg_of(R.README)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(adaptive=False, dt=1 / 1100))
    ps, xs, eps = R.members(cfg, 2, 17, 92)
    rows, losses, info = _many(icnf, True, xs, ps, eps)
    for m in range(2):
        att = info["steps"][m]
        assert info["stats"][m]["naccept"] == 1100 and att.shape == (1024, 4) and (att[:, 3] == 1).all()
        assert att[0, 0] == 0 and (np.diff(att[:, 0]) > 0).all() and np.allclose(att[:, 1], 1 / 1100, rtol=1e-6)
    assert np.isfinite(rows).all()
    icnf.close()


def test_shared_data_is_the_expanded_call():
    cfg = R.cfg_of(R.REGR)
    icnf = make_icnf(cnf, cfg, kernel="mfma")
    M, B = 3, 33
    ps, xs, eps = R.members(cfg, M, B, 91)
    for train in (True, False):
        e = dict(eps=_dev(eps)) if train else {}
        lp, regs, info = cnf.inference_many(icnf, _mode(train), _dev(xs[0]), _dev(ps), {}, **e)
        lp2, regs2, info2 = cnf.inference_many(icnf, _mode(train), _dev(np.repeat(xs[:1], M, axis=0)), _dev(ps), {}, **e)
        assert lp.shape == (M, B) and torch.equal(lp, lp2) and all(torch.equal(a, b) for a, b in zip(regs, regs2))
        assert np.array_equal(info["losses"], info2["losses"]) and info["launches"] == 1
        assert len({lp[m].cpu().numpy().tobytes() for m in range(M)}) == M
    icnf.close()


@pytest.mark.parametrize("which", ["fixed", "adaptive"])
def test_per_member_end_times(which):
    name, cfg, seed, M, B, sol_kw, t1 = R.END_TIME["end times, " + which]
    cfg = R.cfg_of(cfg)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(sol_kw))
    ps, xs, eps = R.members(cfg, M, B, seed)
    t1 = np.asarray(t1, dtype=np.float32)
    rows, losses, info = _many(icnf, True, xs, ps, eps, t1=t1)
    assert [abs(s["t_final"] - t) <= 1e-6 for s, t in zip(info["stats"], t1)] == [True] * M
    _check_members(cfg, True, ps, xs, eps, rows, losses, info, "per-member t1", _tol(sol_kw), t1=t1)
    icnf.close()


def _steered(seed):
    return R.steered_model(cnf, seed)


_STEER_CHILD = r"""
import numpy as np, torch
import continuousnf.jl_amd as cnf
from tests import ensemble_eval_ref as R
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
icnf, twin = R.steered_model(cnf, 12), R.steered_model(cnf, 12)
M, B = 3, 17
ps, xs, _ = R.members(R.cfg_of(R.README), M, B, 86)
lp, regs, info = cnf.inference_many(icnf, cnf.TrainMode(), dev(xs), dev(ps), {})
same = len(set(info["t1"].tolist())) == M
for m in range(M):
    l1, r1 = cnf.inference(twin, cnf.TrainMode(), dev(xs[m]), ps[m], {})
    same = same and twin.last_stats["t_final"] == float(info["t1"][m])
    same = same and torch.equal(l1, lp[m]) and all(torch.equal(a, b[m]) for a, b in zip(r1, regs))
print("SAME", int(same and icnf.rng.bit_generator.state == twin.rng.bit_generator.state))
"""


def test_host_generator_draws_what_a_loop_of_single_calls_draws():
    """eps=None and steer_rate > 0 on a numpy generator: member by member the probes, then the end time -- the order
    ``inference`` consumes the generator in -- so a twin model looping ``inference`` over the members sees the same draws and
    returns the same numbers: bit for bit in a child process where the twin's B = 17 call takes the one-wave-per-workgroup
    form (CNF_WAVE_WG=0), at the parity bar in this one, where it meets through LDS."""
    child = _start_child(_STEER_CHILD)
    cfg = R.cfg_of(R.README)
    icnf, twin = _steered(12), _steered(12)
    M, B = 3, 17
    ps, xs, _ = R.members(cfg, M, B, 86)
    lp, regs, info = cnf.inference_many(icnf, cnf.TrainMode(), _dev(xs), _dev(ps), {})
    assert len(set(info["t1"].tolist())) == M
    for m in range(M):
        l1, r1 = cnf.inference(twin, cnf.TrainMode(), _dev(xs[m]), ps[m], {})
        assert twin.last_stats["t_final"] == float(info["t1"][m]) == info["stats"][m]["t_final"]
        got = torch.stack([lp[m], *[r[m] for r in regs]]).cpu().numpy()
        assert_parity(got, torch.stack([l1, *r1]).cpu().numpy(), f"steered member {m} against the twin's single call", trace_row=0)
    assert icnf.rng.bit_generator.state == twin.rng.bit_generator.state
    # TestMode never steers and draws nothing
    before = icnf.rng.bit_generator.state
    _, _, info = cnf.inference_many(icnf, cnf.TestMode(), _dev(xs), _dev(ps), {})
    assert icnf.rng.bit_generator.state == before and (info["t1"] == np.float32(1.0)).all()
    icnf.close(); twin.close()
    _child_says_same(child)


# ---- sampling ----
def _generate(icnf, train, ps, z0, eps, **kw):
    xs, logq = cnf.generate_many(icnf, _mode(train), _dev(ps), {}, z0.shape[2], z0=_dev(z0), eps=_dev(eps), with_logp=True,
                                 with_steps=True, **kw)
    return xs.cpu().numpy(), logq.cpu().numpy(), icnf.last_ensemble_info


def _check_samples(cfg, train, ps, z0, eps, xs, logq, info, what, tol, t0=None):
    for m in range(ps.shape[0]):
        att = info["steps"][m]
        start = cfg.tspan[1] if t0 is None else float(t0[m])
        c = R.cfg_of(cfg, (cfg.tspan[0], start), cfg.use_jvp)
        u0 = np.vstack([z0[m], np.zeros((c.D(train) - c.n_in, z0.shape[2]), dtype=np.float32)])
        crev = R.cfg_of(cfg, (start, cfg.tspan[0]), cfg.use_jvp)
        R.replay_attempts(crev, train, ps[m], None, eps[m], att, tol, u0=u0)          # the attempts tile the reversed span
        hs = att[att[:, 3] > 0, 1]
        rx, rq = R.replay_generate(c, train, ps[m], z0[m], eps[m], hs)
        print(f"{what}, member {m}: xs {helpers.parity_err(xs[m], rx):.3f}, logq {helpers.parity_err(logq[m][None], rq[None], trace_row=0):.3f} of the bar")
        assert_parity(xs[m], rx, f"{what}, member {m}: samples on its own steps")
        assert_parity(logq[m][None], rq[None], f"{what}, member {m}: logq on its own steps", trace_row=0)


@pytest.mark.parametrize("ci", range(len(R.GENERATE_CASES)))
def test_each_members_samples_match_the_forward_reference(ci):
    cfg, tspan, M, n, train, jvp, sol_kw = R.GENERATE_CASES[ci]
    cfg = R.cfg_of(cfg, tspan, jvp)
    icnf = make_icnf(cnf, cfg, jvp=jvp, kernel="mfma", sol_kwargs=dict(sol_kw))
    ps, _, eps = R.members(cfg, M, n, 3000 + ci)
    z0 = R.base_draws(cfg, M, n, 3000 + ci)
    xs, logq, info = _generate(icnf, train, ps, z0, eps)
    what = f"ensemble sampling {cfg.net.dims} M={M} n={n} {'train' if train else 'test'}{' jvp' if jvp else ''}"
    assert xs.shape == (M, cfg.nvars, n) and logq.shape == (M, n)
    assert info["launches"] == 2 and info["calls"] == 1 and not info["rerun"] and (info["status"] == _lib.OK).all(), info
    _check_samples(cfg, train, ps, z0, eps, xs, logq, info, what, _tol(sol_kw))
    # without the log-density: the same samples; again: the same bits
    x2 = cnf.generate_many(icnf, _mode(train), _dev(ps), {}, n, z0=_dev(z0), eps=_dev(eps)).cpu().numpy()
    assert np.array_equal(x2, xs)
    icnf.close()


@pytest.mark.parametrize("which", ["7-13-7", "6-1-6"])
def test_scoring_the_samples_returns_their_log_density(which):
    """TestMode, no augmentation: ``inference_many`` of what ``generate_many`` drew is ``logq`` within the solver tolerance (the
    5e-3 at which the suite compares solves whose step sequences differ)."""
    name, cfg, seed, M, n, train, sol_kw, _ = R.START_TIME["re-scoring " + which]
    cfg = R.cfg_of(cfg)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(sol_kw))
    ps, _, eps = R.members(cfg, M, n, seed)
    z0 = R.base_draws(cfg, M, n, seed)
    xs, logq = cnf.generate_many(icnf, cnf.TestMode(), _dev(ps), {}, n, z0=_dev(z0), with_logp=True)
    lp, _, info = cnf.inference_many(icnf, cnf.TestMode(), xs.contiguous(), _dev(ps), {})
    assert_parity(lp.cpu().numpy(), logq.cpu().numpy(), f"{which}: inference_many(generate_many) against logq", rtol=R.RESCORE_RTOL, trace_row=0)
    icnf.close()


def test_steered_members_start_at_their_own_times():
    """Given start times, and the draws of a steered model: member by member the base sample, the probes, the steered time --
    ``generate_prob``'s order -- so a twin looping ``generate`` over the members sees the same draws."""
    name, cfg, seed, M, n, train, sol_kw, t0 = R.START_TIME["start times"]
    cfg = R.cfg_of(cfg)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(sol_kw))
    ps, _, eps = R.members(cfg, M, n, seed)
    z0 = R.base_draws(cfg, M, n, seed)
    t0 = np.asarray(t0, dtype=np.float32)
    xs, logq, info = _generate(icnf, True, ps, z0, eps, t0=t0)
    for m in range(M):
        assert info["steps"][m][0, 0] == t0[m] and abs(info["stats"][m]["t_final"]) <= 1e-6
    _check_samples(cfg, True, ps, z0, eps, xs, logq, info, "per-member start times", _tol(sol_kw), t0=t0)
    icnf.close()
    icnf, twin = _steered(13), _steered(13)
    got = cnf.generate_many(icnf, cnf.TrainMode(), _dev(ps), {}, n)
    info = icnf.last_ensemble_info
    assert len(set(info["t0"].tolist())) == M
    for m in range(M):
        one = cnf.generate(twin, cnf.TrainMode(), ps[m], {}, n)
        one = one.cpu().numpy() if hasattr(one, "cpu") else np.asarray(one)
        assert_parity(got[m].cpu().numpy(), one, f"steered sampling, member {m} against the twin's single call")
    assert icnf.rng.bit_generator.state == twin.rng.bit_generator.state
    icnf.close(); twin.close()


def test_device_generator_draws_all_members_at_once():
    cfg = R.cfg_of(R.README)
    mk = lambda: cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh")), 1, 1, lambda3=1e-2,
                               compute_mode=cnf.HIPVecJacMatrixMode("mfma"), sol_kwargs=dict(adaptive=False, dt=1 / 4), rng=cnf.HIPRNG(5))
    icnf = mk()
    M, n, n_in = 3, 17, 2
    ps = np.repeat(R.members(cfg, 1, n, 97)[0], M, axis=0)
    xs = cnf.generate_many(icnf, cnf.TrainMode(), _dev(ps), {}, n)
    assert icnf.rng.offset == 2 * n_in * M * n
    g = cnf.HIPRNG(5)
    z0 = g.normal(n_in * M * n, torch.device("cuda", 0)).view(M, n, n_in).permute(0, 2, 1)
    eps = g.normal(n_in * M * n, torch.device("cuda", 0)).view(M, n, n_in).permute(0, 2, 1)
    xs2 = cnf.generate_many(icnf, cnf.TrainMode(), _dev(ps), {}, n, z0=z0, eps=eps)
    assert torch.equal(xs, xs2) and len({xs[m].cpu().numpy().tobytes() for m in range(M)}) == M
    icnf.close()


# ---- failures, and the handle afterwards ----
def test_a_nonfinite_member_is_reported_alone():
    cfg = R.cfg_of(R.REGR)
    icnf = make_icnf(cnf, cfg, kernel="mfma")
    M, B = 3, 17
    ps, xs, eps = R.members(cfg, M, B, 81)
    rows, losses, _ = _many(icnf, True, xs, ps, eps)
    bad = xs.copy()
    bad[1, 0, 3] = np.nan
    with pytest.raises(cnf.CNFError, match="member 1") as e:
        _many(icnf, True, bad, ps, eps)
    assert e.value.status == _lib.ERR_NONFINITE
    # the C ABI: the other members of that very launch are what they are beside a finite member 1
    l, h = _lib.lib(), icnf.handle()
    xr, er, pr = _dev(bad.transpose(0, 2, 1)), _dev(eps.transpose(0, 2, 1)), _dev(ps)
    lp, rg = torch.zeros(M, B, device="cuda"), torch.zeros(M, 3, B, device="cuda")
    ls, status = np.empty(M, dtype=np.float32), np.empty(M, dtype=np.int32)
    opts = cnf.base_icnf._solve_opts(icnf, icnf.tspan)
    _lib.check(l.cnf_inference_many(h, _lib.MODE_TRAIN, M, pr.data_ptr(), xr.data_ptr(), er.data_ptr(), B, C.byref(opts), None,
                                    lp.data_ptr(), rg.data_ptr(), ls.ctypes.data, status.ctypes.data, None, 0, None), h)
    assert status.tolist() == [_lib.OK, _lib.ERR_NONFINITE, _lib.OK] and np.isnan(ls[1])
    got = torch.cat([lp[:, None], rg], dim=1).cpu().numpy()
    assert np.isnan(got[1]).all()
    for m in (0, 2):
        assert ls[m] == losses[m] and np.array_equal(got[m], rows[m])
    assert l.cnf_ensemble_eval_steps(h, 1, None, 0) == -1 < l.cnf_ensemble_eval_steps(h, 0, None, 0)   # (the traced call before it)
    z = torch.full((M, B, cfg.n_in), float("nan"), device="cuda")
    with pytest.raises(cnf.CNFError, match="member 0"):
        cnf.generate_many(icnf, cnf.TrainMode(), pr, {}, B, z0=z.permute(0, 2, 1), eps=_dev(eps))
    icnf.close()


def test_members_that_give_up_are_rerun():
    """poll_limit = 1 (the knob of the existing fallback tests: a bounded wait, not a fault): with three tiles per member the
    meetings run out; the members are run again one at a time, fallbacks included, and the handle stays usable."""
    name, cfg, seed, M, B, sol_kw, _ = R.END_TIME["rerun"]           # (R.START_TIME["rerun"]: the same members, sampled)
    cfg = R.cfg_of(cfg)
    icnf = make_icnf(cnf, cfg, kernel="mfma", sol_kwargs=dict(sol_kw))
    ps, xs, eps = R.members(cfg, M, B, seed)
    z0 = R.base_draws(cfg, M, B, seed)
    hs = [0.25] * 4
    want = [R.replay_inference(cfg, True, ps[m], xs[m], eps[m], hs) for m in range(M)]
    wantg = [R.replay_generate(cfg, True, ps[m], z0[m], eps[m], hs) for m in range(M)]
    icnf.set_solve_wait(poll_limit=1)
    try:
        lp, regs, info = cnf.inference_many(icnf, cnf.TrainMode(), _dev(xs), _dev(ps), {}, eps=_dev(eps))
        gx, gq = cnf.generate_many(icnf, cnf.TrainMode(), _dev(ps), {}, B, z0=_dev(z0), eps=_dev(eps), with_logp=True)
        ginfo = icnf.last_ensemble_info
    finally:
        icnf.set_solve_wait(poll_limit=0x7fffffff)
    assert info["rerun"] and ginfo["rerun"], (info, ginfo)
    rows = torch.stack([lp, *regs], dim=1).cpu().numpy()
    for m in range(M):
        assert_parity(rows[m], want[m][0], f"rerun member {m}", trace_row=0)
        assert_parity(np.asarray([info["losses"][m]]), np.asarray([want[m][1]]), f"rerun member {m}: loss")
        assert_parity(gx[m].cpu().numpy(), wantg[m][0], f"rerun member {m}: samples")
        assert_parity(gq[m].cpu().numpy()[None], wantg[m][1][None], f"rerun member {m}: logq", trace_row=0)
    rows2, losses2, info2 = _many(icnf, True, xs, ps, eps)
    assert not info2["rerun"]
    for m in range(M):
        assert_parity(rows2[m], want[m][0], f"member {m} after the wait was restored", trace_row=0)
    icnf.close()


def test_the_handle_afterwards_is_what_it_was():
    name, cfg, tspan, train, seed, M, B, scales, sol_kw = R.OTHER["handle afterwards"]
    cfg = R.cfg_of(cfg, tspan)
    ps, xs, eps = R.members(cfg, M, B, seed)
    z0 = R.base_draws(cfg, M, B, seed)
    mine = O.glorot_params(cfg.net, np.random.default_rng(85), np.float32, 0.5)

    def own(icnf):
        v, g = cnf.loss_and_grad(icnf, cnf.TrainMode(), _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
        lp, _ = cnf.inference(icnf, cnf.TrainMode(), _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
        return v, g.cpu().numpy(), lp.cpu().numpy()

    def ensemble_calls(icnf):
        _many(icnf, True, xs, ps, eps)
        cnf.generate_many(icnf, cnf.TrainMode(), _dev(ps), {}, B, z0=_dev(z0), eps=_dev(eps), with_logp=True)

    fresh = make_icnf(cnf, cfg, kernel="mfma")
    want = own(fresh)
    cot = (torch.ones(B, device="cuda") / B, None)
    cnf.vjp.inference_record(fresh, cnf.TrainMode(), _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
    want_pull = cnf.vjp.inference_pullback(fresh, cot).cpu().numpy()
    fresh.close()
    icnf = make_icnf(cnf, cfg, kernel="mfma")
    ensemble_calls(icnf)
    after = own(icnf)
    for a, b in zip(want, after):
        assert np.array_equal(a, b)
    # straight after the ensemble calls, with nothing uploaded in between
    again = make_icnf(cnf, cfg, kernel="mfma")
    again.set_params(mine)
    ensemble_calls(again)
    lp, _ = cnf.inference(again, cnf.TrainMode(), _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
    assert np.array_equal(lp.cpu().numpy(), want[2])
    # a record made before the ensemble calls still pulls back
    cnf.vjp.inference_record(again, cnf.TrainMode(), _dev(xs[0]), mine, {}, eps=_dev(eps[0]))
    ensemble_calls(again)
    assert np.array_equal(cnf.vjp.inference_pullback(again, cot).cpu().numpy(), want_pull)
    icnf.close(); again.close()


# ---- the bagged density ----
def test_ensemble_dist():
    cfg = R.cfg_of(R.REV0, (0.0, 1.0))
    icnf = make_icnf(cnf, cfg, kernel="mfma", rng=31)
    M, n = 4, 50
    ps, xs, _ = R.members(cfg, M, n, 98)
    w = np.asarray([0.4, 0.0, 0.35, 0.25])
    d = cnf.EnsembleDist(icnf, cnf.TestMode(), _dev(ps), {}, weights=w)
    A = _dev(xs[0])
    lm = cnf.logpdf_members(d, A)
    assert lm.shape == (M, n) and torch.equal(lm, cnf.inference_many(icnf, cnf.TestMode(), A, _dev(ps), {})[0])
    lp = d.logpdf(A)
    ref = cnf.ensemble.mixture_logpdf(lm.cpu().numpy().astype(np.float64), w)
    assert np.all(np.abs(lp.cpu().numpy() - ref) <= 2e-6 * np.maximum(1.0, np.abs(ref)))
    assert torch.equal(d.pdf(A), lp.exp())
    # rand: the seeded count split decides which member every column comes from; the same draws through generate_many
    twin = make_icnf(cnf, cfg, kernel="mfma", rng=31)
    before = icnf.rng.bit_generator.state
    assert tuple(d.rand(0).shape) == (cfg.nvars, 0) and icnf.rng.bit_generator.state == before
    draws, member = d.rand(n, with_members=True)
    counts = cnf.ensemble.split_counts(twin.rng, n, w)
    assert draws.shape == (cfg.nvars, n) and counts.sum() == n and counts[1] == 0
    assert np.array_equal(member, np.repeat(np.arange(M), counts))
    full = cnf.generate_many(twin, cnf.TestMode(), _dev(ps), {}, int(counts.max()))
    assert torch.equal(draws, torch.cat([full[m, :, :c] for m, c in enumerate(counts)], dim=1))
    assert icnf.rng.bit_generator.state == twin.rng.bit_generator.state
    icnf.close(); twin.close()


def test_refusals():
    lay = lambda dims, act="tanh": [cnf.Dense(a, b, act) for a, b in zip(dims[:-1], dims[1:])]
    models = [
        cnf.construct(cnf.CondRNODE, cnf.Chain(*lay((4, 6, 2))), 1, 1, rng=5),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((2, 6, 2))), 1, 1, rng=5, basedist=cnf.DiagNormal(np.zeros(2), np.ones(2) * 2)),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((2, 6, 2))), 1, 1, rng=5, compute_mode=cnf.HIPVecJacMatrixMode("generic")),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((32, 96, 32))), 32, 0, rng=5),
        cnf.construct(cnf.RNODE, cnf.Chain(*lay((2, 6, 2), "softplus")), 1, 1, rng=5),
        cnf.construct(cnf.Planar, cnf.Chain(cnf.PlanarLayer(2, "tanh")), 2, 0, rng=5),
    ]
    for ic in models:
        before = ic.rng.bit_generator.state
        x = torch.zeros((2, ic.nvars, 16), device="cuda")
        p = torch.zeros((2, ic.nn.n_params_internal), device="cuda")
        for mode in (cnf.TrainMode(), cnf.TestMode()):
            with pytest.raises(NotImplementedError):
                cnf.inference_many(ic, mode, x, p, {})
            with pytest.raises(NotImplementedError):
                cnf.generate_many(ic, mode, p, {}, 16)
            with pytest.raises(NotImplementedError):
                cnf.EnsembleDist(ic, mode, p, {})
            assert cnf.ensemble_eval_capacity(ic, mode, 16) == 0
        assert ic.rng.bit_generator.state == before
        ic.close()
