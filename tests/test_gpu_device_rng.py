"""The device generator on the MI355X: cnf_draw_uint32 / cnf_draw_normal against the numpy
restatement of the contract (tests/philox_ref.py), its statistics, and HIPRNG through inference, loss_and_grad, generate
and fit -- each call with a HIPRNG must compute exactly what the same call computes given the tensors the generator
produces."""
import ctypes as C

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib, configs
from tests import philox_ref as P
from tests.helpers import assert_parity

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U64 = 2 ** 64 - 1


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw(fn, seed, sub, offset, out):
    """The C entry point itself, into a caller-owned (possibly offset) slice."""
    _lib.check(getattr(_lib.lib(), fn)(0, seed, sub, offset, out.data_ptr(), out.numel(), _stream()))
    return out


def _words(seed, sub, offset, n):
    return _raw("cnf_draw_uint32", seed, sub, offset, torch.empty(n, dtype=torch.uint32, device="cuda")).cpu().numpy()


def _normals(seed, sub, offset, n):
    return _raw("cnf_draw_normal", seed, sub, offset, torch.empty(n, dtype=torch.float32, device="cuda")).cpu().numpy()


def _within_one_ulp(got, ref64, what):
    assert np.all(np.isfinite(got)), f"{what}: NaN or Inf"
    ulp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref64)
    assert np.all(err <= ulp), f"{what}: worst {np.max(err / ulp):.2f} ulp at {int(np.argmax(err / ulp))}"


def test_words_are_bit_identical_to_the_restatement():
    ns = (1, 3, 4, 1000, 262147)
    for seed in (0, 1, U64, 0x0123456789ABCDEF):
        for sub in (0, 7, 2 ** 63):
            for off in (0, 1, 2, 3, 5, 4 * 2 ** 32 - 6, 2 ** 40 + 1):
                ref = P.uint32(seed, sub, off, max(ns))
                for n in ns:
                    got = _words(seed, sub, off, n)
                    assert np.array_equal(got, ref[:n]), (seed, sub, off, n)


def test_normals_are_within_one_ulp_of_the_float64_restatement():
    for seed, sub, off, n in ((0, 0, 0, 262147), (U64, 2 ** 63, 4 * 2 ** 32 - 6, 4099), (0x0123456789ABCDEF, 7, 5, 1001),
                              (1, 0, 2 ** 40 + 1, 3)):
        _within_one_ulp(_normals(seed, sub, off, n), P.normal64(seed, sub, off, n), f"normal {seed}/{sub}/{off}/{n}")
    # the blocks whose u1 is at the top of (0, 1]: w_even >= 2^32 - 4096 (where a float u1 would round to 1), and
    # w_even = 2^32 - 1 itself (u1 = 1 exactly: r = 0), found by scanning the word stream on the device
    seed, chunk = 5, 1 << 28
    words = torch.empty(chunk, dtype=torch.uint32, device="cuda")
    near, top = [], []
    for k in range(256):
        w = _raw("cnf_draw_uint32", seed, 0, k * chunk, words).view(torch.int32)
        if k == 0:
            i = torch.nonzero((w[: 1 << 24] < 0) & (w[: 1 << 24] >= -4096)).flatten().cpu().numpy()
            near = [int(e) for e in i if e % 2 == 0]
        i = torch.nonzero(w == -1).flatten().cpu().numpy()
        top += [k * chunk + int(e) for e in i if e % 2 == 0]
        if len(top) >= 2:
            break
    del words
    assert len(near) >= 2 and len(top) >= 1, (len(near), len(top))
    for e in near + top:
        assert int(P.uint32(seed, 0, e, 1)[0]) >= 0xFFFFF000
        _within_one_ulp(_normals(seed, 0, e, 2), P.normal64(seed, 0, e, 2), f"normal at u1 ~ 1, element {e}")
    for e in top:
        z = _normals(seed, 0, e, 2)
        assert z[0] == 0.0 and z[1] == 0.0


def test_draws_are_deterministic_and_split_into_consecutive_pieces():
    seed, sub, off, n = 0xDEADBEEF, 3, 6, 100003
    a, b = _words(seed, sub, off, n), _words(seed, sub, off, n)
    assert np.array_equal(a, b)
    whole = _normals(seed, sub, off, n)
    assert np.array_equal(whole, _normals(seed, sub, off, n))
    cuts = [0, 1, 2, 5, 9, 4097, 4098, 50001, n - 3, n]
    buf = torch.full((n + 1,), float("nan"), device="cuda")       # a slice at every alignment (the 4-byte store path too)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _raw("cnf_draw_normal", seed, sub, off + lo, buf[1 + lo:1 + hi])
    assert np.array_equal(buf[1:].cpu().numpy(), whole) and torch.isnan(buf[0])
    wbuf = torch.zeros(n + 3, dtype=torch.int32, device="cuda")
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _raw("cnf_draw_uint32", seed, sub, off + lo, wbuf[3 + lo:3 + hi])
    assert np.array_equal(wbuf[3:].cpu().numpy().view(np.uint32), a) and int(wbuf[:3].abs().sum()) == 0
    assert not np.array_equal(_normals(seed + 1, sub, off, 1000), whole[:1000])
    assert not np.array_equal(_normals(seed, sub + 1, off, 1000), whole[:1000])
    h = cnf.rng.draw_normal(1000, seed, sub, off)
    assert h.is_cuda and np.array_equal(h.cpu().numpy(), whole[:1000])


def test_statistics_at_four_million():
    from scipy.stats import kstest
    n, n_in = 1 << 22, 32
    z = _normals(2024, 1, 0, n).astype(np.float64)
    se = 1.0 / np.sqrt(n)
    assert abs(z.mean()) < 5 * se
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / n)
    assert kstest(z, "norm").pvalue > 1e-6
    for lag in (1, n_in):
        c = np.corrcoef(z[:-lag], z[lag:])[0, 1]
        assert abs(c) < 5 / np.sqrt(n - lag), (lag, c)


def test_hutchinson_probe_is_unbiased():
    """The mean of the TrainMode dlogp row over K = 256 device probes lies within 5 standard errors of the exact trace."""
    K, B, nv, na = 256, 64, 2, 2
    n_in = nv + na
    nn = cnf.Chain(cnf.Dense(n_in, 16, "tanh"), cnf.Dense(16, n_in, "tanh"))
    ic = cnf.construct(cnf.FFJORD, nn, nv, na, rng=cnf.HIPRNG(77))
    ps = torch.from_numpy(configs.glorot_params((n_in, 16, n_in), 4, 0.3)).cuda()
    u = torch.from_numpy(np.random.default_rng(5).standard_normal((n_in + 3, B)).astype(np.float32)).cuda()
    eps = ic.rng.normal(n_in * K * B, 0).view(K * B, n_in).t()
    du = cnf.augmented_f(u.repeat(1, K).contiguous(), ps, 0.0, ic, cnf.TrainMode(), ic.nn, {}, eps)
    exact = cnf.augmented_f(u[:n_in + 1].contiguous(), ps, 0.0, ic, cnf.TestMode(), ic.nn, {}, None)[n_in]
    est = du[n_in].view(K, B).double()
    m, s = est.mean(0), est.std(0) / np.sqrt(K)
    z = ((m - exact.double()).abs() / s).cpu().numpy()
    assert np.all(s.cpu().numpy() > 0) and z.max() < 5, z.max()
    ic.close()


def _headline(jvp=False, rng=0):
    wl = configs.BASELINE[3]
    return wl, configs.build(wl, jvp=jvp, sol_kwargs=configs.README_TOLERANCES, rng=rng)


def _inputs(wl, B):
    xs_h, _ = configs.synthetic_inputs(wl, B, 1)
    ps_h = configs.glorot_params(wl.dims, 3, 0.05)
    return xs_h, torch.from_numpy(np.ascontiguousarray(xs_h.T)).cuda().t(), ps_h, torch.from_numpy(ps_h).cuda()


def _eps(seed, offset, n_in, B, sub=0):
    out = torch.empty(n_in * B, dtype=torch.float32, device="cuda")
    return _raw("cnf_draw_normal", seed, sub, offset, out).view(B, n_in).t()


def test_inference_with_hiprng_is_inference_with_the_drawn_probes():
    s = 0x5EED
    wl, ic = _headline(rng=cnf.HIPRNG(s))
    B, n_in = wl.batch, wl.n_in
    xs_h, xs, ps_h, ps = _inputs(wl, B)
    ic.rng.offset = o0 = 12345                                   # any position of the stream
    lp, regs = cnf.inference(ic, cnf.TrainMode(), xs, ps, {})
    assert ic.rng.offset == o0 + n_in * B
    eps = _eps(s, o0, n_in, B)
    lp2, regs2 = cnf.inference(ic, cnf.TrainMode(), xs, ps, {}, eps=eps)
    assert ic.rng.offset == o0 + n_in * B                        # an explicit eps draws nothing
    assert torch.equal(lp, lp2) and all(torch.equal(a, b) for a, b in zip(regs, regs2))
    lp3, _ = cnf.inference(ic, cnf.TrainMode(), xs, ps, {})
    assert ic.rng.offset == o0 + 2 * n_in * B and not torch.equal(lp3, lp)
    ic.close()
    # host xs: the same probes (drawn on the device, copied back), the same numbers at the parity bar
    wl, ich = _headline(rng=cnf.HIPRNG(s))
    ich.rng.offset = o0
    lph, _ = cnf.inference(ich, cnf.TrainMode(), xs_h, ps_h, {})
    assert isinstance(lph, np.ndarray) and ich.rng.offset == o0 + n_in * B
    lph2, _ = cnf.inference(ich, cnf.TrainMode(), xs_h, ps_h, {}, eps=eps.cpu().numpy())
    assert np.array_equal(lph, lph2)
    assert_parity(lph, lp.cpu().numpy().astype(np.float64), "HIPRNG inference: host xs vs device xs")
    ich.close()


@pytest.mark.parametrize("jvp", [False, True], ids=["vjp", "jvp"])
def test_loss_and_grad_with_hiprng_is_loss_and_grad_with_the_drawn_probes(jvp):
    s = 99
    wl, ic = _headline(jvp=jvp, rng=cnf.HIPRNG(s, subsequence=1))
    B, n_in = wl.batch, wl.n_in
    _, xs, _, ps = _inputs(wl, B)
    v, g = cnf.loss_and_grad(ic, cnf.TrainMode(), xs, ps, {})
    assert ic.rng.offset == n_in * B
    v2, g2 = cnf.loss_and_grad(ic, cnf.TrainMode(), xs, ps, {}, eps=_eps(s, 0, n_in, B, sub=1))
    assert v == v2 and torch.equal(g, g2)
    v3, _ = cnf.loss_and_grad(ic, cnf.TrainMode(), xs, ps, {})
    assert ic.rng.offset == 2 * n_in * B and v3 != v
    ic.close()


def test_generate_and_rand_with_hiprng():
    s, n = 31, 512
    wl, ic = _headline(rng=cnf.HIPRNG(s))
    n_in = wl.n_in
    _, _, _, ps = _inputs(wl, 8)
    x = cnf.generate(ic, cnf.TrainMode(), ps, {}, n)
    assert torch.is_tensor(x) and x.is_cuda and x.shape == (wl.nvars, n) and ic.rng.offset == 2 * n_in * n
    z0, eps = _eps(s, 0, n_in, n), _eps(s, n_in * n, n_in, n)
    x2 = cnf.generate(ic, cnf.TrainMode(), ps, {}, n, z0=z0, eps=eps)
    assert torch.equal(x, x2)
    d = cnf.ICNFDist(ic, cnf.TrainMode(), ps, {})
    y = cnf.rand(d, n)
    assert y.is_cuda and ic.rng.offset == 4 * n_in * n
    y2 = cnf.generate(ic, cnf.TrainMode(), ps, {}, n, z0=_eps(s, 2 * n_in * n, n_in, n), eps=_eps(s, 3 * n_in * n, n_in, n))
    assert torch.equal(y, y2)
    ic.close()


def test_fit_with_hiprng_is_reproducible():
    """Three pipelined iterations at batch 32: the same seed gives the same parameters bit for bit (the pipelined loop is
    bit-reproducible: test_gpu_parity compares it with the synchronous one by array_equal), another seed other ones."""
    data = np.random.default_rng(3).beta(2.0, 4.0, size=(96, 2)).astype(np.float32)
    res = []
    for seed in (8, 8, 9):
        nn = cnf.Chain(cnf.Dense(4, 12, "tanh"), cnf.Dense(12, 4, "tanh"))
        icf = cnf.construct(cnf.RNODE, nn, 2, 2, tspan=(0.0, 3.0), steer_rate=0.1, lambda3=1e-2, rng=cnf.HIPRNG(seed))
        model = cnf.ICNFModel(icf, optimizers=(cnf.Adam(eta=1e-3),), n_epochs=1, batch_size=32)
        (psf, _), _, rep = cnf.fit(model, 0, data)
        assert rep["stats"]["iterations"] == 3 and icf.rng.offset == 3 * 4 * 32
        res.append((psf, rep["losses"]))
        icf.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert not np.array_equal(res[0][0], res[2][0])
