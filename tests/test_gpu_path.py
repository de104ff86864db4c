"""Flow paths on the device (cnf_solve_path; continuousnf.jl_amd/path.py): both routes against the float64 replay of the
device's own accepted steps (tests/path_ref.py), and against the calls without a path.

Solver tolerances, weights and span are those of test_adaptive_solves_on_their_own_step_sequence (reltol = sqrt(eps32),
abstol = eps32, Glorot weights, biases x 0.3, tspan (0, 1)).  The bar is helpers.assert_parity's default with the dlogp row
as ``trace_row``; a case that misses it takes tests/envelope.py's rule -- rtol = max(RTOL, 8 x floor) <= 1e-3, the floor from
the float32 run of the replay against its float64 run -- and says so on stdout (``_check_replay``)."""
import ctypes
import os

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from oracle import cnf_oracle as O
from tests import envelope as E
from tests import helpers
from tests import path_ref as R
from tests.helpers import assert_parity, make_icnf, parity_err

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
KW = dict(reltol=float(np.sqrt(EPS32)), abstol=EPS32)
# start, two times 1e-3 apart, a few spread (most steps serve none), the end
SAVEAT = [0.0, 0.25, 0.251, 0.4, 0.77, 0.93, 1.0]
SAVEAT64 = [float(t) for t in np.linspace(0.0, 1.0, 64)]
f64 = lambda a: None if a is None else np.asarray(a).astype(np.float64)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _one_launch_expected():
    return os.environ.get("CNF_PERSISTENT") != "0" and os.environ.get("CNF_WAVE") != "0"


class Case:
    """A model, its inputs and the float64 right-hand side."""

    def __init__(self, dims, nvars, naugs, mode, B, seed, kernel="mfma", cond=False):
        self.train = mode != "test"
        self.jvp = mode == "jvp"
        self.n_in = nvars + naugs
        self.n_cond = dims[0] - self.n_in
        self.B = B
        net = O.Net(tuple(dims), (O.ACT_TANH,) * (len(dims) - 1))
        self.cfg = O.Cfg(net, nvars, naugs, 1e-2, 1e-2, 1e-2 if naugs else 0.0, self.jvp, (0.0, 1.0))
        rng = np.random.default_rng(seed)
        self.flat = O.glorot_params(net, rng, np.float32, 0.3)
        self.xs = rng.standard_normal((nvars, B)).astype(np.float32)
        self.eps = rng.standard_normal((self.n_in, B)).astype(np.float32)
        self.ys = rng.standard_normal((self.n_cond, B)).astype(np.float32) if cond else None
        self.ic = make_icnf(cnf, self.cfg, jvp=self.jvp, kernel=kernel, tag=cnf.CondRNODE if cond else cnf.RNODE, sol_kwargs=KW)
        self.mode = cnf.TrainMode() if self.train else cnf.TestMode()

    def args(self):
        return (_dev(self.xs),) + ((_dev(self.ys),) if self.ys is not None else ()) + (self.flat, {})

    def prob(self):
        return cnf.inference_prob(self.ic, self.mode, *self.args(), eps=_dev(self.eps))

    def rhs(self, dtype=np.float64):
        c = lambda a: None if a is None else a.astype(dtype)
        return self.cfg.rhs(c(self.flat), c(self.eps) if self.train else None, self.train, c(self.ys))


def _check_replay(case, u0, tspan, info, path, saveat, what):
    """Every slice against the float64 replay of the steps the device took; returns the replay."""
    ts, hs = info["steps"]
    assert len(ts) == info["stats"]["naccept"]
    ref, _ = R.replay(case.rhs(), f64(u0), tspan, ts, hs, saveat)
    got = path.cpu().numpy() if hasattr(path, "cpu") else path
    worst = max(parity_err(got[k], ref[k], trace_row=case.n_in) for k in range(len(saveat)))
    rtol = helpers.RTOL
    if worst > 1.0:
        r32, _ = R.replay(case.rhs(np.float32), np.asarray(u0, dtype=np.float32), tspan, ts, hs, saveat, np.float32)
        floor = helpers.RTOL * max(parity_err(r32[k], ref[k], trace_row=case.n_in) for k in range(len(saveat)))
        rtol = E.rtol_of(floor)
        print(f"{what}: {worst:.2f} x the default bar; float32 floor {floor:.3g} -> rtol {rtol:.3g}")
        assert rtol <= E.RTOL_CAP, (what, floor)
    print(f"{what}: worst slice {worst:.3f} x the default bar, {len(ts)} steps")
    for k in range(len(saveat)):
        assert_parity(got[k], ref[k], f"{what} slice {k}", rtol=rtol, trace_row=case.n_in)
    return ref


IN_LAUNCH = [((2, 6, 2), 1, 1, "mfma"), ((16, 48, 16), 8, 8, "mfma"), ((16, 16), 8, 8, "auto")]


@pytest.mark.parametrize("mode", ["vjp", "jvp", "test"])
@pytest.mark.parametrize("dims,nvars,naugs,kernel", IN_LAUNCH, ids=["2-6-2", "16-48-16", "16-16"])
def test_in_launch_path(dims, nvars, naugs, kernel, mode):
    """B = 68: five tiles, the last with four live columns -- the one-wave-per-workgroup form base_sol takes too, so the solve
    itself is base_sol's bit for bit; every slice meets the replay; 64 save times put many in one step."""
    if not _one_launch_expected():
        pytest.skip("the in-launch route is switched off")
    c = Case(dims, nvars, naugs, mode, 68, 4100 + len(dims) + dims[1] + {"vjp": 0, "jvp": 1, "test": 2}[mode], kernel)
    p0 = c.prob()
    fs0 = cnf.base_sol(c.ic, p0).view().clone()
    st0 = dict(p0.stats)
    lp0, regs0 = cnf.inference_sol(c.ic, c.mode, c.prob())
    paths = {}
    for saveat in (SAVEAT, SAVEAT64):
        p = c.prob()
        u0 = p.u0.view().clone()
        fsol, path, info = cnf.solve_path(c.ic, p, saveat)
        paths[len(saveat)] = path
        st = info["stats"]
        assert st["launches"] == st0["launches"] == 1, (st, st0)
        assert (st["naccept"], st["nreject"]) == (st0["naccept"], st0["nreject"]), (st, st0)
        assert torch.equal(fsol.view(), fs0)
        assert tuple(path.shape) == (len(saveat), c.cfg.D(c.train), 68)
        assert torch.equal(path[-1], fsol.view()) and torch.equal(path[0], u0)
        _check_replay(c, u0.cpu().numpy(), (0.0, 1.0), info, path, saveat, f"in-launch {dims} {mode} K={len(saveat)}")
    logpx, regs, pth = cnf.inference_path(c.ic, c.mode, *c.args(), saveat=SAVEAT, eps=_dev(c.eps))
    assert torch.equal(logpx, lp0) and all(torch.equal(a, b) for a, b in zip(regs, regs0))
    assert c.ic.last_stats["naccept"] == st0["naccept"] and c.ic.last_stats["nreject"] == st0["nreject"]
    assert torch.equal(pth["z"], paths[len(SAVEAT)][:, :c.n_in, :]) and torch.equal(pth["dlogp"], paths[len(SAVEAT)][:, c.n_in, :])
    assert tuple(pth["z"].shape) == (len(SAVEAT), c.n_in, 68) and tuple(pth["dlogp"].shape) == (len(SAVEAT), 68)
    assert ("E" in pth and "n" in pth) == c.train
    c.ic.close()


def test_small_batch_takes_its_own_form():
    """B = 20: base_sol runs the tiles as the waves of one workgroup, the path one tile per workgroup: the final state agrees
    with base_sol's at the parity bar, and the end slice is the call's own final state bit for bit."""
    if not _one_launch_expected():
        pytest.skip("the in-launch route is switched off")
    c = Case((2, 6, 2), 1, 1, "vjp", 20, 4201)
    fs0 = cnf.base_sol(c.ic, c.prob()).view().cpu().numpy()
    p = c.prob()
    u0 = p.u0.view().clone()
    fsol, path, info = cnf.solve_path(c.ic, p, SAVEAT)
    assert info["stats"]["launches"] == 1
    assert_parity(fsol.view().cpu().numpy(), fs0, "B = 20: path solve vs base_sol", trace_row=c.n_in)
    assert torch.equal(path[-1], fsol.view()) and torch.equal(path[0], u0)
    _check_replay(c, u0.cpu().numpy(), (0.0, 1.0), info, path, SAVEAT, "in-launch B=20")
    c.ic.close()


@pytest.mark.parametrize("mode", ["vjp", "test"])
def test_generate_path_runs_the_reverse_direction(mode):
    """generate_path on 2 -> 6 -> 2: the samples and their density are generate(..., with_logp=True)'s -- another kernel form and
    its own step sequence, hence at the solver tolerance (10 x reltol: two sequences that each hold the step error under
    reltol) --, the end slice carries xs, and logq along the path meets the replay."""
    c = Case((2, 6, 2), 1, 1, mode, 20, 4301)
    rng = np.random.default_rng(4302)
    z0 = rng.standard_normal((c.n_in, 20)).astype(np.float32)
    saveat = [1.0, 0.9, 0.5, 0.499, 0.1, 0.0]
    xs, logq, pth = cnf.generate_path(c.ic, c.mode, c.flat, {}, 20, saveat=saveat, z0=_dev(z0), eps=_dev(c.eps))
    steps = pth["steps"]
    xs2, logq2 = cnf.generate(c.ic, c.mode, c.flat, {}, 20, z0=_dev(z0), eps=_dev(c.eps), with_logp=True)
    assert_parity(xs.cpu().numpy(), xs2.cpu().numpy(), "generate_path xs vs generate", rtol=10 * KW["reltol"])
    assert_parity(logq.cpu().numpy(), logq2.cpu().numpy(), "generate_path logq vs generate", rtol=10 * KW["reltol"])
    assert torch.equal(pth["z"][-1][:c.cfg.nvars], xs) and torch.equal(pth["logq"][-1], logq)
    assert torch.equal(pth["z"][0], _dev(z0))
    D = c.cfg.D(c.train)
    u0 = np.zeros((D, 20))
    u0[:c.n_in] = z0
    ref, _ = R.replay(c.rhs(), u0, (1.0, 0.0), steps[0], steps[1], saveat)
    assert np.all(steps[1] < 0)
    lp0 = -0.5 * (np.sum(f64(z0) ** 2, axis=0) + c.n_in * np.log(2 * np.pi))
    got = np.concatenate([pth["z"].cpu().numpy(), pth["dlogp"].cpu().numpy()[:, None, :]], axis=1)
    for k in range(len(saveat)):
        assert_parity(got[k], ref[k][:c.n_in + 1], f"generate_path {mode} slice {k}", trace_row=c.n_in)
        # logq = logpdf(z0) + dlogp: dlogp's own bar, and the float32 roundings of logpdf(z0) and of the sum
        dl = ref[k][c.n_in]
        bar = helpers.RTOL * (np.abs(dl) + np.sqrt(np.mean(dl ** 2))) + helpers.ATOL + 4 * EPS32 * (np.abs(lp0) + np.abs(lp0 + dl))
        assert np.all(np.abs(pth["logq"][k].cpu().numpy() - (lp0 + dl)) <= bar), k
    c.ic.close()


def test_generate_path_with_a_non_default_base_and_host_arrays():
    """logq goes through basedist.logpdf; numpy inputs come back as numpy."""
    rng = np.random.default_rng(4401)
    flat = O.glorot_params(O.Net((2, 6, 2), (O.ACT_TANH,) * 2), rng, np.float32, 0.3)
    eps = rng.standard_normal((2, 8)).astype(np.float32)
    base = cnf.DiagNormal([0.5, -0.25], [1.5, 0.75])
    nn = cnf.Chain(cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh"))
    ic = cnf.construct(cnf.RNODE, nn, 1, 1, compute_mode=cnf.HIPVecJacMatrixMode("mfma"), tspan=(0.0, 1.0), sol_kwargs=KW, basedist=base,
                       rng=3)
    z0 = rng.standard_normal((2, 8)).astype(np.float32)
    xs, logq, pth = cnf.generate_path(ic, cnf.TestMode(), flat, {}, 8, saveat=[1.0, 0.5, 0.0], z0=z0, eps=eps)
    assert isinstance(xs, np.ndarray) and isinstance(pth["z"], np.ndarray) and isinstance(pth["logq"], np.ndarray)
    want = base.logpdf(f64(z0))[None, :] + f64(pth["dlogp"])
    assert np.max(np.abs(pth["logq"] - want)) <= 4 * EPS32 * np.max(np.abs(want))
    assert np.array_equal(pth["logq"][-1], logq) and np.array_equal(pth["z"][0], z0)
    ic.close()


def test_conditional_model_in_launch():
    """CondRNODE 4 -> 6 -> 2 (two conditioning rows), B = 20: the per-sample bias rows stay in the PATH form's registers."""
    if not _one_launch_expected():
        pytest.skip("the in-launch route is switched off")
    c = Case((4, 6, 2), 1, 1, "vjp", 20, 4501, cond=True)
    p = c.prob()
    u0 = p.u0.view().clone()
    fsol, path, info = cnf.solve_path(c.ic, p, SAVEAT)
    assert info["stats"]["launches"] == 1
    assert torch.equal(path[-1], fsol.view()) and torch.equal(path[0], u0)
    _check_replay(c, u0.cpu().numpy(), (0.0, 1.0), info, path, SAVEAT, "conditional in-launch")
    c.ic.close()


STREAMED = [((2, 6, 2), 1, 1, 20, "generic"), ((4, 8, 8, 4), 2, 2, 5, "auto"), ((32, 128, 128, 32), 32, 0, 48, "mfma")]


@pytest.mark.parametrize("mode", ["vjp", "test"])
@pytest.mark.parametrize("dims,nvars,naugs,B,kernel", STREAMED, ids=["2-6-2-generic", "4-8-8-4", "headline"])
def test_streamed_path(dims, nvars, naugs, B, kernel, mode):
    """One attempt at a time, k_dense_out behind every accepted step: slices against their own replay; the end slice is the
    final state and the start slice u0, bit for bit."""
    c = Case(dims, nvars, naugs, mode, B, 4600 + dims[1] + (1 if mode == "test" else 0), kernel)
    for saveat in (SAVEAT, SAVEAT64):
        p = c.prob()
        u0 = p.u0.view().clone()
        fsol, path, info = cnf.solve_path(c.ic, p, saveat)
        st = info["stats"]
        assert st["launches"] > 6 * (st["naccept"] + st["nreject"]), st          # (per-stage launches: the streamed route)
        assert torch.equal(path[-1], fsol.view()) and torch.equal(path[0], u0)
        _check_replay(c, u0.cpu().numpy(), (0.0, 1.0), info, path, saveat, f"streamed {dims} {mode} K={len(saveat)}")
    c.ic.close()


def test_the_two_routes_agree_at_the_solver_tolerance():
    """The same 2 -> 6 -> 2 problem with kernel="generic" (streamed) and in the launch: other kernels, other step sequences, the
    same flow -- 10 x reltol, as two sequences that each hold the step error under reltol."""
    if not _one_launch_expected():
        pytest.skip("the in-launch route is switched off")
    a, b = Case((2, 6, 2), 1, 1, "vjp", 20, 4701, "generic"), Case((2, 6, 2), 1, 1, "vjp", 20, 4701, "mfma")
    _, pa, ia = cnf.solve_path(a.ic, a.prob(), SAVEAT)
    _, pb, ib = cnf.solve_path(b.ic, b.prob(), SAVEAT)
    assert ia["stats"]["launches"] > 1 and ib["stats"]["launches"] == 1
    for k in range(len(SAVEAT)):
        assert_parity(pa[k].cpu().numpy(), pb[k].cpu().numpy(), f"streamed vs in-launch slice {k}", rtol=10 * KW["reltol"], trace_row=a.n_in)
    a.ic.close()
    b.ic.close()


def test_fallback_to_the_streamed_route():
    """Every wait of the one-launch solve gives up at its first poll: the call returns the streamed path."""
    if not _one_launch_expected():
        pytest.skip("the in-launch route is switched off")
    c = Case((2, 6, 2), 1, 1, "vjp", 68, 4801)
    fb0 = c.ic.solve_fallbacks()
    c.ic.set_solve_wait(0, 1)
    p = c.prob()
    u0 = p.u0.view().clone()
    fsol, path, info = cnf.solve_path(c.ic, p, SAVEAT)
    c.ic.set_solve_wait(0, 0x7fffffff)
    assert c.ic.solve_fallbacks() == fb0 + 1
    assert info["stats"]["launches"] > 1
    assert torch.equal(path[-1], fsol.view()) and torch.equal(path[0], u0)
    _check_replay(c, u0.cpu().numpy(), (0.0, 1.0), info, path, SAVEAT, "fallback")
    c.ic.close()


def test_refusals():
    """Lock-step shards have no path; bad save times are CNF_ERR_BAD_ARG through the C ABI with a NULL handle."""
    c = Case((2, 6, 2), 1, 1, "vjp", 20, 4901)
    c.ic.set_shard_reduce(lambda v: 0)
    with pytest.raises(cnf.CNFError) as e:
        cnf.solve_path(c.ic, c.prob(), SAVEAT)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    c.ic.set_shard_reduce(None)
    assert _lib.lib().cnf_path_steps(c.ic.handle(), None, None, 0) == -1
    fsol, path, info = cnf.solve_path(c.ic, c.prob(), SAVEAT)                # ... and works again without them
    assert torch.equal(path[-1], fsol.view())
    c.ic.close()
    l = _lib.lib()
    buf = torch.zeros(64, device="cuda")
    p = buf.data_ptr()
    opts = _lib.cnf_solve_opts(0.0, 1.0, 1e-6, 1e-3, 0.0, 1, 100, _lib.KERNEL_AUTO)
    for bad in ([0.5, float("nan")], [0.5, 0.25], [-0.5], [1.5]):
        sv = np.asarray(bad, dtype=np.float32)
        assert l.cnf_solve_path(None, _lib.MODE_TEST, p, None, p, 4, ctypes.byref(opts), sv.ctypes.data, sv.size, p, None,
                                None) == _lib.ERR_BAD_ARG
    assert l.cnf_solve_path(None, _lib.MODE_TEST, p, None, p, 4, ctypes.byref(opts), None, 0, p, None, None) == _lib.ERR_BAD_ARG
