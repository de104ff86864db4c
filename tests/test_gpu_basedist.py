"""``basedist`` / ``epsdist`` on the MI355X (src/base_icnf.jl:16-25): the Rademacher form of the device generator against
its contract, a general Gaussian base through inference, loss, generate, the gradients and fit, against float64
(scipy, and the oracle's pieces with the base log-density and terminal cotangent of tests/basedist_ref.py).  Bars are the
project's own: ``assert_parity`` at its defaults for forward values, the gradient bar of test_gpu_parity's ``_assert_grad``."""
import ctypes as C
import zlib

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib, configs
from continuousnf.jl_amd.base_icnf import _as_colmajor, _solve_opts, draw_eps, _Buf
from oracle import cnf_grad_oracle as G
from oracle import cnf_oracle as O
from tests import basedist_ref as R
from tests.helpers import ACT_NAME, assert_parity

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = dict(configs.README_TOLERANCES)
U64 = 2 ** 64 - 1


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _assert_grad(grad, rgrad, what):
    from tests.test_gpu_parity import _assert_grad as bar          # the existing gradient tests' bar, not restated
    print(f"{what}: max |err| {np.abs(grad - rgrad).max():.3e}, max |ref| {np.abs(rgrad).max():.3e}, rms {np.sqrt(np.mean(rgrad ** 2)):.3e}")
    bar(grad, rgrad, what)


def _icnf(cfg, basedist=None, epsdist=None, jvp=False, kernel="auto", sol_kwargs=None, rng=0, tag=None, n_cond=0):
    dims = (cfg.net.dims[0] + n_cond,) + tuple(cfg.net.dims[1:])
    layers = [cnf.Dense(i, o, ACT_NAME[a]) for i, o, a in zip(dims[:-1], dims[1:], cfg.net.acts)]
    cm = cnf.HIPJacVecMatrixMode(kernel) if jvp else cnf.HIPVecJacMatrixMode(kernel)
    tag = tag or (cnf.CondRNODE if n_cond else cnf.FFJORD)
    return cnf.construct(tag, cnf.Chain(*layers), cfg.nvars, cfg.naugs, compute_mode=cm, tspan=cfg.tspan, lambda1=cfg.lam1,
                         lambda2=cfg.lam2, lambda3=cfg.lam3, sol_kwargs=sol_kwargs or {}, rng=rng, basedist=basedist, epsdist=epsdist)


def _base(rng, n, kind):
    """(the library's object, the float64 restatement) of one random Gaussian: eigenvalues of Sigma in [0.1, 10]."""
    mean, cov = rng.standard_normal(n), R.random_cov(rng, n, kind)
    return cnf.MvNormal(mean, cov), R.Gauss(mean, cov)


# the solve routes: BASELINE configs 1, 2, 3, 5 and a deeper network for the general MFMA kernels (cnf_mfma.hip)
def _route(name):
    if name == "mfma-deep":
        return O.Cfg(O.Net((24, 64, 48, 40, 24), (O.ACT_TANH, O.ACT_SOFTPLUS, O.ACT_TANH, O.ACT_TANH)), 16, 8, 1e-2, 1e-2, 1e-2)
    return O.baseline_cfg(int(name[3:]))[0]


ROUTES = ["cfg1", "cfg2", "cfg3", "cfg5", "mfma-deep"]
MODES = ["train-vjp", "train-jvp", "test"]


def _inference_state(ic, mode, xs, eps, ps):
    """cnf_inference with the final state returned: (logpx, regs (3, B), u_final (D, B)) as numpy arrays."""
    B = xs.shape[1]
    ic.set_params(ps)
    xb = _as_colmajor(xs, ic.nvars, "xs")
    eb = _as_colmajor(eps, ic.nvars + ic.naugmented, "eps") if eps is not None else None
    D = ic.nvars + ic.naugmented + 1 + (2 if mode.cnf == _lib.MODE_TRAIN else 0)
    lp, regs, uf = (torch.empty(k, dtype=torch.float32, device="cuda") for k in (B, 3 * B, D * B))
    opts, stats, h = _solve_opts(ic, ic.tspan), _lib.cnf_solve_stats(), ic.handle()
    _lib.check(_lib.lib().cnf_inference(h, mode.cnf, xb.ptr, eb.ptr if eb is not None else None, lp.data_ptr(), regs.data_ptr(),
                                        uf.data_ptr(), B, C.byref(opts), C.byref(stats), C.c_void_p(torch.cuda.current_stream().cuda_stream)), h)
    torch.cuda.synchronize()
    return lp.cpu().numpy(), regs.view(3, B).cpu().numpy(), uf.view(B, D).t().cpu().numpy(), stats.as_dict()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the Rademacher draw
# ---------------------------------------------------------------------------------------------------------------------
def _raw(fn, seed, sub, offset, out):
    _lib.check(getattr(_lib.lib(), fn)(0, seed, sub, offset, out.data_ptr(), out.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def test_rademacher_draw_is_bit_exact():
    ns = (1, 3, 4, 5, 1023, 32 * 8192)
    for seed, sub in ((0, 0), (U64, 2 ** 63), (0x0123456789ABCDEF, 7)):
        for off in (0, 1, 2, 3, 5, 4 * 2 ** 32 - 6, 2 ** 40 + 1, 2 ** 63 + 3, U64 - max(ns)):
            ref = R.rademacher(seed, sub, off, max(ns))
            for n in ns:
                for shift in (0, 1, 3):                      # output pointers at every 4-byte alignment
                    buf = torch.full((n + shift + 1,), float("nan"), device="cuda")
                    got = _raw("cnf_draw_rademacher", seed, sub, off, buf[shift:shift + n]).cpu().numpy()
                    assert np.array_equal(got, ref[:n]), (seed, sub, off, n, shift)
                    assert torch.isnan(buf[-1]) and (shift == 0 or torch.isnan(buf[:shift]).all())
    # equal to cnf_draw_uint32 mapped through the contract; any split equals the whole; |mean| <= 5 / sqrt(n)
    seed, sub, off, n = 0xDEADBEEF, 3, 6, 32 * 8192
    words = _raw("cnf_draw_uint32", seed, sub, off, torch.empty(n, dtype=torch.uint32, device="cuda")).cpu().numpy()
    whole = _raw("cnf_draw_rademacher", seed, sub, off, torch.empty(n, device="cuda")).cpu().numpy()
    assert np.array_equal(whole, R.rademacher_of_words(words)) and set(np.unique(whole)) == {-1.0, 1.0}
    cuts = [0, 1, 2, 5, 9, 4097, 4098, 50001, n - 3, n]
    buf = torch.full((n + 1,), float("nan"), device="cuda")
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _raw("cnf_draw_rademacher", seed, sub, off + lo, buf[1 + lo:1 + hi])
    assert np.array_equal(buf[1:].cpu().numpy(), whole)
    print("rademacher mean", whole.mean(), "bar", 5 / np.sqrt(n))
    assert abs(float(whole.astype(np.float64).mean())) <= 5 / np.sqrt(n)
    # argument validation as the other draws; HIPRNG advances by n
    l = _lib.lib()
    assert l.cnf_draw_rademacher(0, 1, 0, 0, None, 0, None) == _lib.OK
    assert l.cnf_draw_rademacher(0, 1, 0, 0, None, 4, None) == _lib.ERR_BAD_ARG
    assert l.cnf_draw_rademacher(0, 1, 0, U64 - 1, buf.data_ptr(), 4, None) == _lib.ERR_BAD_ARG
    assert l.cnf_draw_rademacher(0, 1, 0, 0, buf.data_ptr() + 2, 4, None) == _lib.ERR_BAD_ARG
    g = cnf.HIPRNG(seed, subsequence=sub)
    g.offset = off
    a, b = g.rademacher(1000, 0), g.rademacher(24, 0)
    assert g.offset == off + 1024 and np.array_equal(torch.cat([a, b]).cpu().numpy(), whole[:1024])


# ---------------------------------------------------------------------------------------------------------------------
# 5. closed form: last layer W = 0, bias b  =>  z1 = [x; 0] + (t1 - t0) act(b), dlogp = 0, logpx = logpdf(basedist, z1)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["diag", "full"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("route", ROUTES)
def test_constant_field_gives_the_closed_form_density(route, mode, kind):
    from scipy.stats import multivariate_normal
    cfg = _route(route)
    rng = np.random.default_rng(zlib.crc32(f"{route} {mode} {kind} 5".encode()))
    B, n_in, net = 40, cfg.n_in, cfg.net
    dist, g = _base(rng, n_in, kind)
    train, jvp = mode != "test", mode == "train-jvp"
    m = cnf.TrainMode() if train else cnf.TestMode()
    ic = _icnf(cfg, basedist=dist, jvp=jvp, sol_kwargs=TOL)
    xs = rng.standard_normal((cfg.nvars, B)).astype(np.float32)
    eps = rng.standard_normal((n_in, B)).astype(np.float32) if train else None
    last = len(net.dims) - 2
    for which in ("b = 0", "random b"):
        flat = O.glorot_params(net, rng, np.float32, 0.1)
        b = np.zeros(n_in) if which == "b = 0" else 0.3 * rng.standard_normal(n_in)
        # (the flat layout: per layer weight then bias; the last layer's block is the tail of the vector)
        tail = net.dims[-2] * n_in + n_in
        flat[-tail:-n_in] = 0.0
        flat[-n_in:] = b.astype(np.float32)
        act = O.act_apply(net.acts[last], flat[-n_in:].astype(np.float64)[:, None])
        act = act[0] if isinstance(act, tuple) else act
        z1 = np.vstack([xs.astype(np.float64), np.zeros((cfg.naugs, B))]) + (cfg.tspan[1] - cfg.tspan[0]) * act
        ref = multivariate_normal(g.mean, g.cov).logpdf(z1.T)
        lp, _ = cnf.inference(ic, m, _dev(xs), _dev(flat), {}, eps=None if eps is None else _dev(eps))
        print(route, mode, kind, which, ic.last_stats)
        assert_parity(lp.cpu().numpy(), ref, f"closed form {route} {mode} {kind} {which}")
    ic.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. random weights: logpx against the float64 replay, regulariser rows bit-identical to the default handle's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["diag", "full"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("route", ROUTES)
def test_random_weights_against_the_float64_replay(route, mode, kind):
    cfg = _route(route)
    cfg.tspan = (0.0, 1.0)
    rng = np.random.default_rng(zlib.crc32(f"{route} {mode} {kind} 6".encode()))
    B, n_in = 24, cfg.n_in
    dist, g = _base(rng, n_in, kind)
    train, jvp = mode != "test", mode == "train-jvp"
    m = cnf.TrainMode() if train else cnf.TestMode()
    kw = dict(adaptive=False, dt=1 / 8)
    flat = O.glorot_params(cfg.net, rng, np.float32, 0.1)
    xs = rng.standard_normal((cfg.nvars, B)).astype(np.float32)
    eps = rng.standard_normal((n_in, B)).astype(np.float32) if train else None
    ic, ic0 = _icnf(cfg, basedist=dist, jvp=jvp, sol_kwargs=kw), _icnf(cfg, jvp=jvp, sol_kwargs=kw)
    ici = _icnf(cfg, basedist=cnf.MvNormal(np.zeros(n_in), np.ones(n_in)), jvp=jvp, sol_kwargs=kw)
    dx, de, dp = _dev(xs), (None if eps is None else _dev(eps)), _dev(flat)
    lp, regs, uf, st = _inference_state(ic, m, dx, de, dp)
    lp0, regs0, uf0, st0 = _inference_state(ic0, m, dx, de, dp)
    lpi, regsi, _, _ = _inference_state(ici, m, dx, de, dp)
    assert st["launches"] == st0["launches"] + 1                       # one small launch more than the default handle
    assert np.array_equal(regs, regs0) and np.array_equal(regsi, regs0) and np.array_equal(uf, uf0)
    c64 = O.Cfg(cfg.net, cfg.nvars, cfg.naugs, cfg.lam1, cfg.lam2, cfg.lam3, use_jvp=jvp, tspan=cfg.tspan)
    f64 = lambda a: None if a is None else a.astype(np.float64)
    with R.oracle_with(g):
        _, ref_lp, _, _ = O.inference(c64, f64(flat), f64(xs), f64(eps), train, dt=1 / 8, adaptive=False)
    assert_parity(lp, ref_lp, f"logpx vs float64 {route} {mode} {kind}")
    # the post-pass itself: logpx against c - 1/2 |W (z1 - mu)|^2 - dlogp in float64 from the returned final state
    own = dist.logpdf(uf[:n_in].astype(np.float64)) - uf[n_in].astype(np.float64)
    assert_parity(lp, own, f"logpx vs its own final state {route} {mode} {kind}")
    assert_parity(lpi, lp0.astype(np.float64), f"MvNormal(0, I) vs the default handle {route} {mode}")
    # the public calls agree with the C entry point bit for bit, device and host arrays
    a, ra = cnf.inference(ic, m, dx, dp, {}, eps=de)
    assert np.array_equal(a.cpu().numpy(), lp) and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(ra, regs))
    hb, _ = cnf.inference(ic, m, xs, flat, {}, eps=eps)
    assert_parity(hb, ref_lp, f"host arrays {route} {mode} {kind}")
    for c in (ic, ic0, ici):
        c.close()


def test_headline_case_at_full_batch_and_reset_to_default():
    """B = 8192 on the headline network (the one-launch solve): logpx against float64 from its own final state, submitted
    inferences equal the synchronous ones, and cnf_set_basedist(kind 0) gives the default handle's results back bit for bit."""
    wl = configs.BASELINE[3]
    rng = np.random.default_rng(77)
    dist, g = _base(rng, wl.n_in, "full")
    xs_h, eps_h = configs.synthetic_inputs(wl, wl.batch, 1)
    flat = configs.glorot_params(wl.dims, 3, 0.05)
    cfg = _route("cfg3")
    ic, ic0 = _icnf(cfg, basedist=dist, sol_kwargs=TOL, tag=cnf.RNODE), _icnf(cfg, sol_kwargs=TOL, tag=cnf.RNODE)
    dx, de, dp = _dev(xs_h), _dev(eps_h), _dev(flat)
    m = cnf.TrainMode()
    lp, regs, uf, st = _inference_state(ic, m, dx, de, dp)
    lp0, regs0, uf0, st0 = _inference_state(ic0, m, dx, de, dp)
    print("headline", st, st0)
    assert np.array_equal(regs, regs0) and np.array_equal(uf, uf0) and st["launches"] == st0["launches"] + 1
    n_in = wl.n_in
    assert_parity(lp, dist.logpdf(uf[:n_in].astype(np.float64)) - uf[n_in].astype(np.float64), "headline B = 8192, dense base")
    # with_sums: the sums of the same launch, reproducible; loss from them
    a1 = cnf.inference(ic, m, dx, dp, {}, eps=de, with_sums=True)
    a2 = cnf.inference(ic, m, dx, dp, {}, eps=de, with_sums=True)
    assert np.array_equal(a1[0].cpu().numpy(), lp) and torch.equal(a1[2], a2[2]) and torch.equal(a1[0], a2[0])
    s64 = np.array([lp.astype(np.float64).sum(), regs[0].astype(np.float64).sum(), regs[1].astype(np.float64).sum(),
                    regs[2].astype(np.float64).sum(), wl.batch])
    assert_parity(a1[2].cpu().numpy(), s64, "five loss sums, headline")
    s0 = cnf.inference(ic0, m, dx, dp, {}, eps=de, with_sums=True)[2]
    assert torch.allclose(a1[2][1:], s0[1:], rtol=1e-6, atol=0)        # E, n, A sums: the default handle's (its launch adds in another order)
    assert torch.allclose(a1[2], cnf.loss_sums(ic, a1[0], a1[1]), rtol=1e-6, atol=0)
    val = cnf.loss(ic, m, dx, dp, {}, eps=de)
    assert val == cnf.loss_from_sums(ic, m, a1[2])
    # submitted inferences: the same numbers as the synchronous call
    subs = [cnf.inference_submit(ic, m, dx, dp, {}, eps=de, with_sums=True) for _ in range(3)]
    for _ in subs:
        cnf.inference_collect(ic)
    torch.cuda.synchronize()
    for s in subs:
        assert torch.equal(s[0], a1[0]) and torch.equal(s[2], a1[2]) and all(torch.equal(x, y) for x, y in zip(s[1], a1[1]))
    # back to the default: bit for bit what a handle that never had a base computes, with its launch count
    h = ic.handle()
    _lib.check(_lib.lib().cnf_set_basedist(h, 0, None, None, None, 0.0), h)
    lpr, regsr, _, str_ = _inference_state(ic, m, dx, de, dp)
    assert np.array_equal(lpr, lp0) and np.array_equal(regsr, regs0) and str_["launches"] == st0["launches"]
    # and bad arguments
    l = _lib.lib()
    w = np.ones(n_in, np.float32)
    assert l.cnf_set_basedist(h, 3, w.ctypes.data, w.ctypes.data, w.ctypes.data, 0.0) == _lib.ERR_BAD_ARG
    assert l.cnf_set_basedist(h, 1, None, w.ctypes.data, w.ctypes.data, 0.0) == _lib.ERR_BAD_ARG
    bad = w.copy(); bad[3] = 0.0
    assert l.cnf_set_basedist(h, 1, w.ctypes.data, bad.ctypes.data, w.ctypes.data, 0.0) == _lib.ERR_BAD_ARG
    bad[3] = np.nan
    assert l.cnf_set_basedist(h, 1, bad.ctypes.data, w.ctypes.data, w.ctypes.data, 0.0) == _lib.ERR_BAD_ARG
    lpr2, _, _, _ = _inference_state(ic, m, dx, de, dp)
    assert np.array_equal(lpr2, lp0)                                   # a refused call changes nothing
    ic.close(); ic0.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. sums, loss and column shards (fixed dt: every column's solve is its own)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["train", "test"])
def test_sums_and_loss_of_shards_combine_to_the_whole_batch(mode):
    from continuousnf.jl_amd.parallel import distributed_loss
    cfg = _route("cfg2")
    rng = np.random.default_rng(31)
    B, n_in = 300, cfg.n_in
    dist, g = _base(rng, n_in, "full")
    m = cnf.TrainMode() if mode == "train" else cnf.TestMode()
    flat = _dev(O.glorot_params(cfg.net, rng, np.float32, 0.1))
    xs, eps = _dev(rng.standard_normal((cfg.nvars, B))), _dev(rng.standard_normal((n_in, B)))
    ic = _icnf(cfg, basedist=dist, sol_kwargs=dict(adaptive=False, dt=1 / 16))
    logpx, regs, sums = cnf.inference(ic, m, xs, flat, {}, eps=eps, with_sums=True)
    lp2, regs2 = cnf.inference(ic, m, xs, flat, {}, eps=eps)
    assert torch.equal(logpx, lp2) and all(torch.equal(a, b) for a, b in zip(regs, regs2))
    assert torch.equal(sums, cnf.inference(ic, m, xs, flat, {}, eps=eps, with_sums=True)[2])       # two repeats: bitwise
    ref = cnf.loss_sums(ic, lp2, regs2)
    assert torch.allclose(sums, ref, rtol=1e-6, atol=0) and float(sums[4]) == B
    parts = [cnf.inference(ic, m, xs[:, lo:hi].contiguous(), flat, {}, eps=eps[:, lo:hi].contiguous(), with_sums=True)
             for lo, hi in ((0, 150), (150, 300))]
    assert torch.equal(torch.cat([p[0] for p in parts]), logpx)
    comb = parts[0][2] + parts[1][2]
    assert torch.allclose(comb, sums, rtol=1e-6, atol=0)
    val = cnf.loss(ic, m, xs, flat, {}, eps=eps)
    assert abs(val - cnf.loss_from_sums(ic, m, comb)) <= 1e-6 * max(1.0, abs(val))
    assert abs(distributed_loss(ic, m, xs, flat, {}, eps=eps) - val) <= 1e-6 * max(1.0, abs(val))
    c64 = O.Cfg(cfg.net, cfg.nvars, cfg.naugs, cfg.lam1, cfg.lam2, cfg.lam3, tspan=cfg.tspan)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    with R.oracle_with(g):
        _, rl, rr, _ = O.inference(c64, f64(flat), f64(xs), f64(eps), mode == "train", dt=1 / 16, adaptive=False)
        rval = O.loss(c64, rl, rr, mode == "train")
    assert abs(val - rval) <= 1e-5 * max(1.0, abs(rval)), (val, rval)
    ic.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. generate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["diag", "full"])
def test_generate_draws_from_the_base_distribution(kind):
    cfg = _route("cfg2")
    rng = np.random.default_rng(17)
    n, n_in = 96, cfg.n_in
    dist, g = _base(rng, n_in, kind)
    flat = O.glorot_params(cfg.net, rng, np.float32, 0.05)
    kw = dict(adaptive=False, dt=1 / 32)
    L = np.diag(dist.chol.astype(np.float64)) if kind == "diag" else dist.chol.astype(np.float64)
    mu = dist.mean.astype(np.float64)
    # HIPRNG: z0 from the normals the default would have drawn at the same offsets, through the same kernel -> exact
    ic, ic0 = _icnf(cfg, basedist=dist, sol_kwargs=kw, rng=cnf.HIPRNG(31)), _icnf(cfg, sol_kwargs=kw, rng=cnf.HIPRNG(31))
    x = cnf.generate(ic, cnf.TrainMode(), flat, {}, n)
    assert x.is_cuda and x.shape == (cfg.nvars, n) and ic.rng.offset == 2 * n_in * n
    nrm = cnf.rng.draw_normal(n_in * n, 31, 0, 0)
    eps = cnf.rng.draw_normal(n_in * n, 31, 0, n_in * n).view(n, n_in).t()
    z0 = cnf.base_sample(ic, nrm, n)
    x2 = cnf.generate(ic0, cnf.TrainMode(), flat, {}, n, z0=z0.view(n, n_in).t(), eps=eps)
    assert torch.equal(x, x2)
    z64 = g.sample_from(nrm.view(n, n_in).t().cpu().numpy())
    bound = n_in * 2.0 ** -23 * (np.abs(mu)[:, None] + np.abs(L) @ np.abs(nrm.view(n, n_in).t().cpu().numpy().astype(np.float64)))
    err = np.abs(z0.view(n, n_in).t().cpu().numpy() - z64)
    print("base sample: worst err / bound", (err / bound).max())
    assert np.all(err <= bound)
    assert torch.equal(cnf.base_sample(ic0, nrm, n), nrm)               # the default base: a copy
    # seeded numpy rng: the host normals through the same kernel
    ich, ich0 = _icnf(cfg, basedist=dist, sol_kwargs=kw, rng=5), _icnf(cfg, sol_kwargs=kw, rng=5)
    xh = cnf.generate(ich, cnf.TestMode(), flat, {}, n)
    hn = np.random.default_rng(5).standard_normal((n, n_in)).astype(np.float32)
    zh = cnf.base_sample(ich, _dev(hn).reshape(-1), n).view(n, n_in).t().cpu().numpy()
    assert isinstance(xh, np.ndarray) and np.array_equal(xh, cnf.generate(ich0, cnf.TestMode(), flat, {}, n, z0=zh))
    prob = cnf.generate_prob(_icnf(cfg, basedist=dist, sol_kwargs=kw, rng=5), cnf.TestMode(), flat, {}, n)
    u0 = prob.u0.view()
    zh64 = g.sample_from(hn.T)
    bh = n_in * 2.0 ** -23 * (np.abs(mu)[:, None] + np.abs(L) @ np.abs(hn.T.astype(np.float64)))
    assert u0.shape == (n_in + 1, n) and np.all(np.abs(u0[:n_in] - zh64) <= bh) and not u0[n_in:].any()
    assert prob.tspan == (cfg.tspan[1], cfg.tspan[0])
    # a z0 given by the caller is used as it is
    zc = rng.standard_normal((n_in, n)).astype(np.float32)
    assert np.array_equal(cnf.generate(ich, cnf.TestMode(), flat, {}, n, z0=zc), cnf.generate(ich0, cnf.TestMode(), flat, {}, n, z0=zc))
    for c in (ic, ic0, ich, ich0):
        c.close()
    # x -> z -> x without augmentation (test_generate_matches_backward_oracle_and_inverts_inference's tolerance), and
    # logpx(x) = logpdf(basedist, z) - dlogp
    cfg0 = O.Cfg(O.Net((8, 24, 8), (O.ACT_TANH,) * 2), 8, 0, tspan=(0.0, 1.0))
    d0, g0 = _base(rng, 8, kind)
    flat0 = O.glorot_params(cfg0.net, rng, np.float32, 0.05)
    icr = _icnf(cfg0, basedist=d0, sol_kwargs=dict(adaptive=False, dt=1 / 64))
    xr = rng.standard_normal((8, 50)).astype(np.float32)
    prob = cnf.inference_prob(icr, cnf.TestMode(), xr, flat0, {})
    fs = np.array(cnf.base_sol(icr, prob).view())
    back = cnf.generate(icr, cnf.TestMode(), flat0, {}, 50, z0=fs[:8])
    assert np.max(np.abs(back - xr)) < 5e-5
    lpx, _ = cnf.inference(icr, cnf.TestMode(), xr, flat0, {})
    assert_parity(lpx, g0.logpdf(fs[:8].astype(np.float64)) - fs[8].astype(np.float64), f"round trip logpx {kind}")
    icr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. Rademacher probes through the model
# ---------------------------------------------------------------------------------------------------------------------
def test_rademacher_probes_through_the_model():
    cfg = _route("cfg2")
    rng = np.random.default_rng(9)
    B, n_in, s = 64, cfg.n_in, 0x5EED
    flat = _dev(O.glorot_params(cfg.net, rng, np.float32, 0.1))
    xs = _dev(rng.standard_normal((cfg.nvars, B)))
    ic = _icnf(cfg, epsdist=cnf.Rademacher(), sol_kwargs=TOL, rng=cnf.HIPRNG(s))
    ic.rng.offset = o0 = 1235
    e = draw_eps(ic, _Buf(xs, cfg.nvars, B, torch), B)
    assert set(np.unique(e.arr.cpu().numpy())) == {-1.0, 1.0} and ic.rng.offset == o0 + n_in * B
    eh = draw_eps(_icnf(cfg, epsdist=cnf.Rademacher(), rng=4), _Buf(np.zeros(1, np.float32), cfg.nvars, B), B)
    assert set(np.unique(eh.arr)) == {-1.0, 1.0}
    probes = lambda off: cnf.rng.draw_rademacher(n_in * B, s, 0, off).view(B, n_in).t()
    ic.rng.offset = o0
    lp, regs = cnf.inference(ic, cnf.TrainMode(), xs, flat, {})
    lp2, regs2 = cnf.inference(ic, cnf.TrainMode(), xs, flat, {}, eps=probes(o0))
    assert torch.equal(lp, lp2) and all(torch.equal(a, b) for a, b in zip(regs, regs2)) and ic.rng.offset == o0 + n_in * B
    v, gr = cnf.loss_and_grad(ic, cnf.TrainMode(), xs, flat, {})
    v2, gr2 = cnf.loss_and_grad(ic, cnf.TrainMode(), xs, flat, {}, eps=probes(o0 + n_in * B))
    assert v == v2 and torch.equal(gr, gr2)
    o1 = ic.rng.offset
    x = cnf.generate(ic, cnf.TrainMode(), flat, {}, B)
    z0 = cnf.rng.draw_normal(n_in * B, s, 0, o1).view(B, n_in).t()
    assert torch.equal(x, cnf.generate(ic, cnf.TrainMode(), flat, {}, B, z0=z0, eps=probes(o1 + n_in * B)))
    ic.close()


def test_rademacher_probe_is_unbiased_and_exact_on_a_diagonal_jacobian():
    # the form of test_hutchinson_probe_is_unbiased: K = 256 draws, 5 measured standard errors
    K, B, nv, na = 256, 64, 2, 2
    n_in = nv + na
    nn = cnf.Chain(cnf.Dense(n_in, 16, "tanh"), cnf.Dense(16, n_in, "tanh"))
    ic = cnf.construct(cnf.FFJORD, nn, nv, na, rng=cnf.HIPRNG(77), epsdist=cnf.Rademacher())
    ps = torch.from_numpy(configs.glorot_params((n_in, 16, n_in), 4, 0.3)).cuda()
    u = torch.from_numpy(np.random.default_rng(5).standard_normal((n_in + 3, B)).astype(np.float32)).cuda()
    eps = ic.rng.rademacher(n_in * K * B, 0).view(K * B, n_in).t()
    du = cnf.augmented_f(u.repeat(1, K).contiguous(), ps, 0.0, ic, cnf.TrainMode(), ic.nn, {}, eps)
    exact = cnf.augmented_f(u[:n_in + 1].contiguous(), ps, 0.0, ic, cnf.TestMode(), ic.nn, {}, None)[n_in]
    est = du[n_in].view(K, B).double()
    m, s = est.mean(0), est.std(0) / np.sqrt(K)
    z = ((m - exact.double()).abs() / s).cpu().numpy()
    print("rademacher unbiasedness: worst z", z.max())
    assert np.all(s.cpu().numpy() > 0) and z.max() < 5, z.max()
    ic.close()
    # one Dense layer with a diagonal weight matrix: J is diagonal, eps' J eps = sum J_ii eps_i^2 = tr J for +-1 probes
    n, B = 12, 200
    rng = np.random.default_rng(12)
    for act in ("tanh", "softplus"):
        nn1 = cnf.Chain(cnf.Dense(n, n, act))
        ic1 = cnf.construct(cnf.FFJORD, nn1, n, 0, rng=cnf.HIPRNG(3), epsdist=cnf.Rademacher())
        W = np.diag(rng.uniform(-1.5, 1.5, n)).astype(np.float32)
        ps1 = _dev(np.concatenate([W.T.reshape(-1), 0.2 * rng.standard_normal(n).astype(np.float32)]))
        u1 = _dev(rng.standard_normal((n + 3, B)))
        exact = cnf.augmented_f(u1[:n + 1].contiguous(), ps1, 0.0, ic1, cnf.TestMode(), ic1.nn, {}, None)[n].cpu().numpy()
        rad = cnf.augmented_f(u1, ps1, 0.0, ic1, cnf.TrainMode(), ic1.nn, {}, ic1.rng.rademacher(n * B, 0).view(B, n).t())[n].cpu().numpy()
        gau = cnf.augmented_f(u1, ps1, 0.0, ic1, cnf.TrainMode(), ic1.nn, {}, ic1.rng.normal(n * B, 0).view(B, n).t())[n].cpu().numpy()
        assert_parity(rad, exact.astype(np.float64), f"single Rademacher probe, diagonal Jacobian ({act})")
        bar = 1e-4 * np.abs(exact) + 1e-6
        assert np.mean(np.abs(gau - exact) > bar) > 0.9          # which a Gaussian probe does not
        ic1.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. gradients against the float64 discrete adjoint on the device's own accepted steps
# ---------------------------------------------------------------------------------------------------------------------
def _grad_train(cfg, B, seed, kind, jvp=False, n_cond=0, scale=0.2, split=None):
    rng = np.random.default_rng(seed)
    net = O.Net((cfg.net.dims[0] + n_cond,) + tuple(cfg.net.dims[1:]), cfg.net.acts) if n_cond else cfg.net
    dist, g = _base(rng, cfg.n_in, kind)
    flat = O.glorot_params(net, rng, np.float32, scale)
    xs = rng.standard_normal((cfg.nvars, B)).astype(np.float32)
    eps = rng.standard_normal((cfg.n_in, B)).astype(np.float32)
    ys = rng.standard_normal((n_cond, B)).astype(np.float32) if n_cond else None
    ic = _icnf(cfg, basedist=dist, jvp=jvp, sol_kwargs=TOL, n_cond=n_cond, tag=cnf.CondRNODE if n_cond else cnf.RNODE)
    args = (_dev(ys), _dev(flat), {}) if n_cond else (_dev(flat), {})
    was = _lib.lib().cnf_set_grad_split(split) if split is not None else None
    try:
        val, grad, gx = cnf.loss_and_grad(ic, cnf.TrainMode(), _dev(xs), *args, eps=_dev(eps), with_x=True)
    finally:
        if split is not None:
            _lib.lib().cnf_set_grad_split(was)
    c64 = O.Cfg(net, cfg.nvars, cfg.naugs, cfg.lam1, cfg.lam2, cfg.lam3, use_jvp=jvp, tspan=cfg.tspan)
    f64 = lambda a: None if a is None else a.astype(np.float64)
    with R.oracle_with(g):
        rval, rgrad, st = G.loss_and_grad(c64, f64(flat), f64(xs), f64(eps), f64(ys), dts=[float(d) for d in ic.last_steps])
    print("steps", len(ic.last_steps), "loss", val, rval)
    assert abs(val - rval) <= 1e-5 * max(1.0, abs(rval)), (val, rval)
    what = f"{cfg.net.dims} B={B} {kind} jvp={jvp} cond={n_cond} split={split}"
    _assert_grad(grad.cpu().numpy(), rgrad, "d loss / d ps, " + what)
    from tests.test_gpu_parity import _assert_grad as bar
    bar(gx.cpu().numpy(), st.grad_x, "d loss / d xs, " + what, rtol=2e-4)
    # the same loss value from `loss`, and the default handle's gradient is another one
    assert abs(cnf.loss(ic, cnf.TrainMode(), _dev(xs), *args, eps=_dev(eps)) - val) <= 1e-6 * max(1.0, abs(val))
    return ic, (xs, eps, flat)


@pytest.mark.parametrize("case", ["wave-32", "headline-32", "headline-2048-one", "headline-2048-two", "headline-jvp-32", "cfg5-32",
                                  "conditional"])
def test_loss_grad_with_a_base_distribution(case):
    c3 = _route("cfg3")
    if case == "wave-32":
        ic, (xs, eps, flat) = _grad_train(_route("cfg2"), 32, 500, "full")
        # submitted gradients are refused at once (nothing drawn, nothing enqueued); cnf_loss_grad then succeeds
        with pytest.raises(NotImplementedError):
            cnf.loss_and_grad_submit(ic, cnf.TrainMode(), _dev(xs), _dev(flat), {}, eps=_dev(eps))
        l, h = _lib.lib(), ic.handle()
        out = torch.empty(flat.size + 1, device="cuda")
        opts = _solve_opts(ic, ic.tspan)
        dx, de = _as_colmajor(_dev(xs), ic.nvars), _as_colmajor(_dev(eps), 16)
        rc = l.cnf_loss_grad_submit(h, _lib.MODE_TRAIN, dx.ptr, de.ptr, 32, C.byref(opts), out[-1:].data_ptr(), out.data_ptr(), None)
        assert rc == _lib.ERR_UNSUPPORTED and l.cnf_inference_pending(h) == 0
        v, g2 = cnf.loss_and_grad(ic, cnf.TrainMode(), _dev(xs), _dev(flat), {}, eps=_dev(eps))
        assert np.isfinite(v) and torch.isfinite(g2).all()
    elif case == "headline-32":
        ic, _ = _grad_train(c3, 32, 501, "full", scale=0.1)
    elif case == "headline-2048-one":
        ic, _ = _grad_train(c3, 2048, 502, "diag", scale=0.1, split=0)
    elif case == "headline-2048-two":
        ic, _ = _grad_train(c3, 2048, 502, "full", scale=0.1, split=1)
    elif case == "headline-jvp-32":
        ic, _ = _grad_train(c3, 32, 503, "full", jvp=True, scale=0.1)
    elif case == "cfg5-32":
        ic, _ = _grad_train(_route("cfg5"), 32, 504, "full", scale=0.1)
    else:
        ic, _ = _grad_train(_route("cfg2"), 40, 505, "full", n_cond=5)
    ic.close()


@pytest.mark.parametrize("route", ["cfg2", "mfma-deep"])
def test_testmode_loss_grad_with_a_base_distribution(route):
    cfg = _route(route)
    rng = np.random.default_rng(600)
    B = 32
    dist, g = _base(rng, cfg.n_in, "full")
    flat = O.glorot_params(cfg.net, rng, np.float32, 0.2)
    xs = rng.standard_normal((cfg.nvars, B)).astype(np.float32)
    ic = _icnf(cfg, basedist=dist, sol_kwargs=TOL)
    val, grad, gx = cnf.loss_and_grad(ic, cnf.TestMode(), _dev(xs), _dev(flat), {}, with_x=True)
    c64 = O.Cfg(cfg.net, cfg.nvars, cfg.naugs, cfg.lam1, cfg.lam2, cfg.lam3, tspan=cfg.tspan)
    rval, rgrad, st = R.loss_and_grad_test(g, c64, flat.astype(np.float64), xs.astype(np.float64), [float(d) for d in ic.last_steps])
    assert abs(val - rval) <= 1e-5 * max(1.0, abs(rval)), (val, rval)
    _assert_grad(grad.cpu().numpy(), rgrad, f"TestMode d loss / d ps {route}")
    from tests.test_gpu_parity import _assert_grad as bar
    bar(gx.cpu().numpy(), st.grad_x, "TestMode d loss / d xs", rtol=2e-4)
    ic.close()


# ---------------------------------------------------------------------------------------------------------------------
# 11. fit / transform / ICNFDist
# ---------------------------------------------------------------------------------------------------------------------
def test_fit_with_a_base_and_rademacher_probes_is_the_hand_written_loop():
    data = np.random.default_rng(3).beta(2.0, 4.0, size=(96, 2)).astype(np.float32) * 3.0 + 1.0      # not standardised
    base = lambda: cnf.DiagNormal([1.8, 2.1, 0.0, 0.0], [0.6, 0.5, 1.0, 1.0])
    mk = lambda: cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(4, 12, "tanh"), cnf.Dense(12, 4, "tanh")), 2, 2, tspan=(0.0, 3.0),
                               steer_rate=0.1, lambda3=1e-2, rng=cnf.HIPRNG(8), basedist=base(), epsdist=cnf.Rademacher())
    icf = mk()
    model = cnf.ICNFModel(icf, optimizers=(cnf.Adam(eta=1e-3),), n_epochs=2, batch_size=32)
    (psf, st), _, rep = cnf.fit(model, 0, data)
    assert rep["stats"]["iterations"] == 6 and not rep["stats"]["pipelined"] and icf.rng.offset == 6 * 4 * 32
    # by hand: the same batches, loss_and_grad + the optimiser's step
    ich = mk()
    x = torch.from_numpy(np.ascontiguousarray(data.T)).cuda()
    ps_h, st_h = cnf.setup(ich.rng, ich.nn, init=model.init)
    ps = torch.from_numpy(ps_h).cuda()
    opt = cnf.Adam(eta=1e-3)
    state, losses = opt.init(ps), []
    for _ in range(2):
        perm = torch.from_numpy(ich.rng.permutation(96)).cuda()
        for lo in range(0, 96, 32):
            v, g = cnf.loss_and_grad(ich, cnf.TrainMode(), x[:, perm[lo:lo + 32]], ps, st_h)
            opt.apply(state, ps, g)
            losses.append(v)
    assert np.array_equal(psf, ps.cpu().numpy()) and np.array_equal(rep["losses"], np.asarray(losses))
    assert np.all(np.isfinite(psf)) and np.all(np.isfinite(rep["losses"]))
    # transform and the Distributions front end go through, and evaluate the base that was given
    lp = cnf.transform(model, (psf, st), data)
    d = cnf.ICNFDist(icf, cnf.TestMode(), psf, st)
    assert lp.shape == (96,) and np.array_equal(lp, cnf.logpdf(d, x).cpu().numpy())
    icn = cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(4, 12, "tanh"), cnf.Dense(12, 4, "tanh")), 2, 2, tspan=(0.0, 3.0), lambda3=1e-2)
    lpn = cnf.logpdf(cnf.ICNFDist(icn, cnf.TestMode(), psf, st), x).cpu().numpy()
    assert np.abs(lp - lpn).max() > 0.1
    y = cnf.rand(d, 40)
    assert y.shape == (2, 40) and torch.isfinite(y).all()
    for c in (icf, ich, icn):
        c.close()


def test_lockstep_shards_carry_the_base_distribution_in_their_sums():
    """Two lock-step shards (two handles on two threads, an in-process all-reduce as cnf_set_shard_reduce's callback, as
    test_lockstep_shards_follow_the_unsharded_solve has them): every shard's logpx and loss sums are those of the base
    distribution, they combine to the unsharded batch's at that test's bar, and a repeat gives the same bits."""
    import threading
    cfg = _route("cfg2")
    B, cut = 300, 130
    rng = np.random.default_rng(77)
    dist, g = _base(rng, cfg.n_in, "full")
    flat = O.glorot_params(cfg.net, rng, np.float32, 0.3)
    xs = rng.standard_normal((cfg.nvars, B)).astype(np.float32)
    xs[:, cut:] *= 2.5
    eps = rng.standard_normal((cfg.n_in, B)).astype(np.float32)
    m = cnf.TrainMode()
    full = _icnf(cfg, basedist=dist, sol_kwargs=TOL)
    lp_f, regs_f, sums_f = cnf.inference(full, m, _dev(xs), _dev(flat), {}, eps=_dev(eps), with_sums=True)
    shards = [(0, cut), (cut, B)]

    def run():
        ics = [_icnf(cfg, basedist=dist, sol_kwargs=TOL) for _ in shards]
        bar, bufs = threading.Barrier(2), [None, None]
        out, errs = [None, None], []

        def reducer(r):
            def f(v):
                bufs[r] = v.copy()
                bar.wait()
                tot = bufs[0] + bufs[1]
                bar.wait()
                v[:] = tot
            return f

        def work(r):
            try:
                lo, hi = shards[r]
                ics[r].set_shard_reduce(reducer(r))
                res = cnf.inference(ics[r], m, _dev(xs[:, lo:hi]), _dev(flat), {}, eps=_dev(eps[:, lo:hi]), with_sums=True)
                torch.cuda.synchronize()
                out[r] = (res[0].cpu().numpy(), res[2].cpu().numpy(), dict(ics[r].last_stats))
            except Exception as e:            # pragma: no cover
                errs.append(e)
                bar.abort()
        th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(120)
        assert not errs, errs
        for c in ics:
            c.close()
        return out

    a, b = run(), run()
    assert a[0][2]["naccept"] == a[1][2]["naccept"] and a[0][2]["dt_last"] == a[1][2]["dt_last"]      # lock step
    for r in range(2):
        assert np.array_equal(a[r][0], b[r][0]) and np.array_equal(a[r][1], b[r][1])                  # two repeats: bitwise
        lo, hi = shards[r]
        assert a[r][1][4] == hi - lo
        assert abs(a[r][1][0] - a[r][0].astype(np.float64).sum()) <= 1e-6 * abs(a[r][1][0])            # the sums hold the new logpx
    assert_parity(np.concatenate([a[0][0], a[1][0]]), lp_f.cpu().numpy().astype(np.float64), "lock-step shards' logpx vs unsharded, dense base")
    comb = a[0][1].astype(np.float64) + a[1][1].astype(np.float64)
    assert_parity(comb, sums_f.cpu().numpy().astype(np.float64), "lock-step shards' loss sums vs unsharded, dense base")
    # and they are not the N(0, I) sums
    s0 = cnf.inference(_icnf(cfg, sol_kwargs=TOL), m, _dev(xs), _dev(flat), {}, eps=_dev(eps), with_sums=True)[2]
    assert abs(float(s0[0]) - float(sums_f[0])) > 1.0
    full.close()
