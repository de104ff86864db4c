"""``basedist`` / ``epsdist`` without a GPU (src/base_icnf.jl:16-25): the float64 restatement against scipy, the
(mu, W, c) reduction of continuousnf.jl_amd/distributions.py against both, the Rademacher contract on the Philox
known-answer words, and what ``construct`` accepts."""
import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import distributions as D
from tests import basedist_ref as R
from tests import philox_ref as P

F = 0xFFFFFFFF


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.mark.parametrize("kind", ["scalar", "diag", "full"])
@pytest.mark.parametrize("n", [2, 4, 32, 128])
def test_logpdf_restatement_and_reduction_equal_scipy(n, kind):
    from scipy.stats import multivariate_normal
    rng = np.random.default_rng(1000 + n)
    mean = rng.standard_normal(n)
    cov = R.random_cov(rng, n, kind)
    z = mean[:, None] + 3.0 * rng.standard_normal((n, 17))
    full = cov * np.eye(n) if kind == "scalar" else (np.diag(cov) if kind == "diag" else cov)
    ref = multivariate_normal(mean, full).logpdf(z.T)
    assert _rel(R.Gauss(mean, cov).logpdf(z), ref) <= 1e-12
    d = cnf.MvNormal(mean, cov)
    assert d.kind == (D.KIND_DENSE if kind == "full" else D.KIND_DIAG) and len(d) == n
    assert _rel(d.logpdf(z), ref) <= 1e-12                      # the (mu, W, c) form, float64
    # its pieces: Sigma = L L', W = inv(L), c = sum log W_ii - n/2 log 2 pi, sample = mu + L n
    L = np.diag(d.chol64) if d.kind == D.KIND_DIAG else d.chol64
    W = np.diag(d.whiten64) if d.kind == D.KIND_DIAG else d.whiten64
    assert np.allclose(L @ L.T, full, rtol=1e-12, atol=1e-13) and np.allclose(W @ L, np.eye(n), atol=1e-12)
    assert np.array_equal(np.triu(W, 1), np.zeros((n, n)))
    assert abs(d.logconst64 - (np.sum(np.log(np.diag(W))) - 0.5 * n * np.log(2 * np.pi))) <= 1e-12 * n
    nrm = rng.standard_normal((n, 5))
    assert np.allclose(d.sample_from(nrm), R.Gauss(mean, cov).sample_from(nrm), rtol=1e-12, atol=1e-12)
    # -d logpdf / dz = W' W (z - mu)
    assert np.allclose(W.T @ W @ (z - mean[:, None]), R.Gauss(mean, cov).neg_grad(z), rtol=1e-10, atol=1e-10)
    # what the device gets: float32, rounded once from the float64 values
    assert d.mean.dtype == d.whiten.dtype == d.chol.dtype == np.float32
    assert np.array_equal(d.whiten, d.whiten64.astype(np.float32)) and d.logconst == float(np.float32(d.logconst64))
    assert d.whiten.flags["C_CONTIGUOUS"] and d.chol.flags["C_CONTIGUOUS"]


def test_diagnormal_is_the_diagonal_case():
    rng = np.random.default_rng(3)
    mean, std = rng.standard_normal(6), np.exp(rng.uniform(-1, 1, 6))
    a, b = cnf.DiagNormal(mean, std), cnf.MvNormal(mean, std ** 2)
    z = rng.standard_normal((6, 9))
    assert a.kind == D.KIND_DIAG and np.array_equal(a.chol64, std)
    assert _rel(a.logpdf(z), b.logpdf(z)) <= 1e-12
    s = cnf.DiagNormal(mean, 2.0)
    assert np.array_equal(s.chol64, np.full(6, 2.0)) and _rel(s.logpdf(z), cnf.MvNormal(mean, 4.0).logpdf(z)) <= 1e-12
    i = cnf.MvNormal(np.zeros(4), np.ones(4))                 # the explicit identity
    assert np.array_equal(i.whiten, np.ones(4, np.float32)) and abs(i.logconst64 + 2 * np.log(2 * np.pi)) < 1e-15


def test_validation_errors():
    ok = np.zeros(3)
    for bad in (lambda: cnf.MvNormal(ok, np.ones(4)),                               # wrong length
                lambda: cnf.MvNormal(ok, np.eye(4)),
                lambda: cnf.MvNormal([0.0, np.nan, 0.0], np.ones(3)),              # non-finite
                lambda: cnf.MvNormal(ok, [1.0, np.inf, 1.0]),
                lambda: cnf.MvNormal(ok, [1.0, 0.0, 1.0]),                          # variance <= 0
                lambda: cnf.MvNormal(ok, -1.0),
                lambda: cnf.DiagNormal(ok, [1.0, -2.0, 1.0]),                       # std <= 0
                lambda: cnf.DiagNormal(ok, 0.0),
                lambda: cnf.DiagNormal(ok, [1.0, 1.0]),
                lambda: cnf.DiagNormal(ok, [1.0, np.nan, 1.0]),
                lambda: cnf.MvNormal(ok, np.array([[1.0, 0.5, 0], [0.4, 1.0, 0], [0, 0, 1.0]])),   # not symmetric
                lambda: cnf.MvNormal(ok, np.array([[1.0, 2.0, 0], [2.0, 1.0, 0], [0, 0, 1.0]])),   # not positive definite
                lambda: cnf.MvNormal(ok, np.ones((3, 3, 3))),
                lambda: cnf.MvNormal([], [])):
        with pytest.raises(ValueError):
            bad()


def test_rademacher_contract_on_the_known_answer_words():
    """Element e is +1.0f if bit 31 of word e is 0 and -1.0f if it is 1: 1 - 2 (word >> 31)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((F, F, F, F), (F, F), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        words = P.philox4x32_10([np.uint32(c) for c in ctr], key)
        assert [int(w) for w in words] == list(out)
        got = R.rademacher_of_words(words)
        assert got.dtype == np.float32 and [float(v) for v in got] == [1.0 - 2.0 * (w >> 31) for w in out]
    # the first vector is block 0 of stream (seed 0, subsequence 0)
    assert [float(v) for v in R.rademacher(0, 0, 0, 4)] == [1.0, -1.0, -1.0, -1.0]
    r = R.rademacher(11, 2, 5, 4099)
    assert set(np.unique(r)) == {-1.0, 1.0} and abs(float(r.mean())) <= 5 / np.sqrt(r.size)
    assert np.array_equal(np.concatenate([R.rademacher(11, 2, 5, 7), R.rademacher(11, 2, 12, 4092)]), r)


def _nn(n):
    return cnf.Chain(cnf.Dense(n, 6, "tanh"), cnf.Dense(6, n, "tanh"))


def test_construct_accepts_the_supported_distributions():
    d = cnf.DiagNormal([0.5, -1.0], [2.0, 0.5])
    m = cnf.MvNormal([0.0, 0.0], [[2.0, 0.3], [0.3, 1.0]])
    ic = cnf.construct(cnf.RNODE, _nn(2), 1, 1, basedist=d, epsdist=cnf.Rademacher())
    assert ic.basedist is d and isinstance(ic.epsdist, cnf.Rademacher)
    assert cnf.construct(cnf.FFJORD, _nn(2), 2, basedist=m).basedist is m
    assert cnf.construct(cnf.FFJORD, _nn(2), 2, epsdist=cnf.StdNormal()).epsdist is None      # the default, spelled out
    e = cnf.construct(cnf.FFJORD, _nn(2), 2, basedist=cnf.MvNormal(np.zeros(2), np.ones(2)))  # explicit identity: the new path
    assert e.basedist is not None and e.basedist.kind == D.KIND_DIAG
    for kw in (dict(basedist="Laplace"), dict(epsdist="Laplace"), dict(basedist=cnf.Rademacher()), dict(epsdist=d),
               dict(epsdist=object())):
        with pytest.raises(NotImplementedError) as err:
            cnf.construct(cnf.RNODE, _nn(2), 1, 1, **kw)
        assert "MvNormal" in str(err.value) and "Rademacher" in str(err.value)      # names what is supported
    with pytest.raises(ValueError):                                                  # length != nvars + naugmented
        cnf.construct(cnf.RNODE, _nn(2), 1, 1, basedist=cnf.DiagNormal(np.zeros(3), 1.0))


def test_default_handle_fields_are_what_they_were():
    a = cnf.construct(cnf.RNODE, _nn(2), 1, 1, rng=3)
    b = cnf.construct(cnf.RNODE, _nn(2), 1, 1, rng=3, basedist=None, epsdist=None)
    assert a.basedist is None and a.epsdist is None and b.basedist is None and b.epsdist is None
    for f in ("tag", "nvars", "naugmented", "inplace", "tspan", "steer_rate", "sol_kwargs", "lambda1", "lambda2", "lambda3",
              "device", "cond", "n_cond"):
        assert getattr(a, f) == getattr(b, f)
    assert a._handle is None and b._handle is None


def test_host_rademacher_probes_are_plus_minus_one():
    from continuousnf.jl_amd.base_icnf import _Buf, draw_eps
    ic = cnf.construct(cnf.FFJORD, _nn(4), 2, 2, rng=5, epsdist=cnf.Rademacher())
    e = draw_eps(ic, _Buf(np.zeros(8, np.float32), 2, 4), 1000)
    assert e.arr.dtype == np.float32 and e.arr.shape == (4000,) and set(np.unique(e.arr)) == {-1.0, 1.0}
    assert abs(float(e.arr.mean())) <= 5 / np.sqrt(4000)
    e2 = draw_eps(cnf.construct(cnf.FFJORD, _nn(4), 2, 2, rng=5, epsdist=cnf.Rademacher()), _Buf(np.zeros(8, np.float32), 2, 4), 1000)
    assert np.array_equal(e.arr, e2.arr)
    # HIPRNG: the host bookkeeping of `rademacher` is `normal`'s
    g = cnf.HIPRNG(9)
    assert g.take(12) == 0 and g.offset == 12 and hasattr(g, "rademacher")


def test_float64_replays_are_pinned_by_central_finite_differences():
    """The gradient expectations of the GPU tests: the oracle's discrete adjoint with the base log-density and terminal
    cotangent of tests/basedist_ref.py, against central differences of its own loss on three parameter directions."""
    from oracle import cnf_grad_oracle as G
    from oracle import cnf_oracle as O
    rng = np.random.default_rng(0)
    cfg = O.Cfg(O.Net((4, 7, 4), (O.ACT_TANH,) * 2), 3, 1, 0.01, 0.01, 0.01)
    flat = O.glorot_params(cfg.net, rng, np.float64, 0.1)
    xs, eps = rng.standard_normal((3, 5)), rng.standard_normal((4, 5))
    g = R.Gauss(rng.standard_normal(4), R.random_cov(rng, 4, "full"))
    dts, h = [0.25] * 4, 1e-6
    with R.oracle_with(g):
        train = lambda p: G.loss_and_grad(cfg, p, xs, eps, dts=dts)[:2]
        v0, _ = train(flat)
        for f in (train, lambda p: R.loss_and_grad_test(g, cfg, p, xs, dts)[:2]):
            _, grad = f(flat)
            for _ in range(3):
                d = rng.standard_normal(flat.size)
                fd = (f(flat + h * d)[0] - f(flat - h * d)[0]) / (2 * h)
                assert abs(fd - grad @ d) <= 1e-7 * max(1.0, abs(fd)), (fd, grad @ d)
    assert O.inference_sol.__module__ == "oracle.cnf_oracle" and G.final_cotangent.__module__ == "oracle.cnf_grad_oracle"
    # the base enters the value: the N(0, I) oracle gives another loss
    assert abs(G.loss_and_grad(cfg, flat, xs, eps, dts=dts)[0] - v0) > 1e-3
