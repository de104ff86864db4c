"""The gradient w.r.t. a learnable base distribution on the device (cnf_base_logpdf_pullback / cnf_base_sample_pullback,
``LearnableNormal``, ``with_base=True`` and the autograd routes) against the float64 reference of tests/base_grad_ref.py.

Cases: ``base_grad_ref.CASES`` -- n_in in {3 (nvars 2 + 1 augmented), 16, 17, 33} and the headline network 32-128-128-32 at
B = 33, B in {1, 17, 300}, the diagonal and the dense kind, TrainMode (VJP, one JVP handle, one conditional model) and TestMode.
Every case takes fixed steps, so every route takes the steps of the reference (asserted).

Bar (base_grad_ref.assert_base): per block err <= rtol scale, rtol = max(1e-4, 8 floor) <= 1e-3, floor = the float32 run of the
same reference against its float64 run (tests/test_base_grad_ref_host.py holds every case's floor under the cap); the scale of
g_scale is at least the max-abs of each of its two summands, the quadratic term and the diag(1 / L) term.
"""
import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from tests import base_grad_ref as BG
from tests import gen_vjp_ref as R
from tests import helpers

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _mode(train):
    return cnf.TrainMode() if train else cnf.TestMode()


def _base(mean, scale, dense, requires_grad=False, device="cpu"):
    m = torch.tensor(mean, dtype=torch.float32, device=device, requires_grad=requires_grad)
    s = torch.tensor(scale, dtype=torch.float32, device=device, requires_grad=requires_grad)
    return cnf.LearnableNormal(m, scale_tril=s) if dense else cnf.LearnableNormal(m, std=s)


def _model(case, base, rng=0):
    net = case.net
    layers = [cnf.Dense(a, b, helpers.ACT_NAME[k]) for a, b, k in zip(net.dims[:-1], net.dims[1:], net.acts)]
    cm = cnf.HIPJacVecMatrixMode(case.kernel) if case.jvp else cnf.HIPVecJacMatrixMode(case.kernel)
    return cnf.construct(cnf.CondRNODE if case.n_cond else cnf.FFJORD, cnf.Chain(*layers), case.nvars, case.naugs, compute_mode=cm,
                         tspan=case.tspan, lambda1=BG.LAM[0], lambda2=BG.LAM[1], lambda3=1.0 if case.naugs else 0.0,
                         sol_kwargs=case.sol_kw, rng=rng, basedist=base)


def _args(flat, ys):
    return (_dev(ys), flat, {}) if ys is not None else (flat, {})


def _steps_are_the_reference(case, icnf, sign=1.0):
    dts = R.fixed_dts(case)
    assert [float(d) for d in icnf.last_steps] == [sign * d for d in dts], (case.name, icnf.last_steps)
    return dts


def _assert_base(got, r64, r32, summands, what):
    """base_grad_ref.assert_base, with the measured errors filed in the notes of parity_report.json."""
    recs = BG.assert_base(got, r64, r32, summands, what)
    helpers.note(f"base-grad {what}: " + "; ".join(f"{n} err/scale {e:.2e} (float32 floor {f:.2e}, rtol {r:.1e})" for n, e, f, r, _, _ in recs))


def _same(a, b):
    return all(np.array_equal(_np(x), _np(y)) for x, y in zip(a, b))


# ---- 1, 5, 6: the density direction ----
@pytest.mark.parametrize("name", list(BG.CASES))
def test_density_direction(name):
    """Three cotangents of logpx from one record against the reference; the gradients w.r.t. ps, xs (and ys) are the same bits
    with and without ``with_base``; two identical calls give the same bits."""
    case, dense, train, cfg, (flat, xs, eps, ys), mean, scale, _, rng = BG.case_setup(name)
    cond = ys is not None
    ws = BG.cotangents_w(rng, case.B)
    icnf = _model(case, _base(mean, scale, dense))
    try:
        cnf.inference_record(icnf, _mode(train), _dev(xs), *_args(flat, ys), eps=_dev(eps) if train else None)
        st = dict(icnf.last_stats)
        dts = _steps_are_the_reference(case, icnf)
        got, plain = [], []
        for w in ws:
            cot = (_dev(w), None)
            plain.append(cnf.inference_pullback(icnf, cot, with_x=True, with_ys=cond))
            got.append(cnf.inference_pullback(icnf, cot, with_x=True, with_ys=cond, with_base=True))
        again = cnf.inference_pullback(icnf, (_dev(ws[0]), None), with_x=True, with_ys=cond, with_base=True)
        first = cnf.base_logpdf_pullback(icnf, _dev(ws[1]))                 # (on its own, after the parameter pullbacks)
    finally:
        icnf.close()
    if name.startswith("headline"):                                       # the record of k_solve3b<RECORD>
        assert st["kernel_used"] == _lib.KERNEL_MFMA, st
    z64 = BG.final_state(cfg, flat, xs, eps, dts, ys, train, np.float64)
    z32 = BG.final_state(cfg, flat, xs, eps, dts, ys, train, np.float32)
    for i, w in enumerate(ws):
        g = got[i]
        assert len(g) == (4 if cond else 3) and _same(g[:-1], plain[i]), f"{name} cot {i}: with_base changed another gradient"
        gm, gs = g[-1]
        assert gm.shape == mean.shape and gs.shape == scale.shape
        if dense:
            assert not np.triu(_np(gs), 1).any()
        r64 = BG.logpdf_grads(z64, w, mean, scale, dense, np.float64)
        r32 = BG.logpdf_grads(z32, w, mean, scale, dense, np.float32)
        _assert_base((_np(gm), _np(gs)), r64, r32, BG.summands_of(r64[1], np.sum(w, dtype=np.float64), scale, dense),
                       f"density {name} cot {i}")
    assert _same(again[-1], got[0][-1]) and _same(again[:-1], got[0][:-1]), f"{name}: two identical calls differ"
    assert _same(first, got[1][-1])


# ---- 2, 5, 6, 7: the sampling direction at a given z0; a smaller batch after a larger one ----
@pytest.mark.parametrize("name", ["n3-dense-B300", "n16-dense-cond-B17", "n17-diag-B1", "n17-dense-B300", "n33-diag-B300-test",
                                  "headline-dense-B33"])
def test_sampling_direction_with_given_z0(name):
    """The fixed-z0 partial against the reference; grad, grad_z0 (and grad_ys) bit-identical with and without ``with_base``; a
    one-hot cotangent gives exactly the one sample's term: the bits of a record of that sample alone, taken afterwards on the
    same handle (a smaller batch after a larger one)."""
    case, dense, train, cfg, (flat, _, eps, ys), mean, scale, nrm, rng = BG.case_setup(name)
    cond = ys is not None
    B = case.B
    z0 = BG.drawn_z0(nrm, mean, scale, dense, np.float32)
    cz, cl = R.cotangents(rng, cfg.n_in, case.nvars, B)["both"]
    j = B // 2
    hot = np.zeros(B, np.float32)
    hot[j] = 0.75
    rec = lambda icnf, cols: cnf.generate_record(icnf, _mode(train), flat, {}, len(cols), ys=_dev(ys[:, cols]) if cond else None,
                                                 z0=_dev(z0[:, cols]), eps=_dev(eps[:, cols]) if train else None)
    icnf = _model(case, _base(mean, scale, dense))
    try:
        rec(icnf, list(range(B)))
        _steps_are_the_reference(case, icnf, -1.0)
        plain = cnf.generate_pullback(icnf, (_dev(cz), _dev(cl)), with_z0=True, with_ys=cond)
        got = cnf.generate_pullback(icnf, (_dev(cz), _dev(cl)), with_z0=True, with_ys=cond, with_base=True)
        again = cnf.generate_pullback(icnf, (_dev(cz), _dev(cl)), with_z0=True, with_ys=cond, with_base=True)
        none = cnf.generate_pullback(icnf, (_dev(cz), None), with_base=True)[-1]          # no cotangent on logq: zeros
        one_of_B = cnf.base_logpdf_pullback(icnf, _dev(hot))
        rec(icnf, [j])
        alone = cnf.base_logpdf_pullback(icnf, _dev(hot[j:j + 1]))
    finally:
        icnf.close()
    assert _same(got[:-1], plain) and _same(again[:-1], got[:-1]) and _same(again[-1], got[-1])
    assert not _np(none[0]).any() and not _np(none[1]).any()
    r64 = BG.logpdf_grads(z0, cl, mean, scale, dense, np.float64)
    r32 = BG.logpdf_grads(z0, cl, mean, scale, dense, np.float32)
    _assert_base(tuple(_np(g) for g in got[-1]), r64, r32, BG.summands_of(r64[1], np.sum(cl, dtype=np.float64), scale, dense),
                   f"fixed z0 {name}")
    assert _np(one_of_B[0]).any() and _same(one_of_B, alone), f"{name}: a one-hot weight is not the one sample's term"


# ---- 3: the sampling direction with z0 drawn from the base: the autograd route ----
@pytest.mark.parametrize("name,device", [("n3-dense-B300", "cpu"), ("n16-dense-cond-B17", "cuda"), ("n17-diag-B1", "cpu"),
                                         ("n33-dense-B17-test", "cuda"), ("headline-dense-B33", "cpu")])
def test_sampling_direction_with_drawn_z0(name, device):
    """``differentiable_generate`` draws z0 = mean + L n itself: the gradient that reaches ``mean`` and the scale is the total
    derivative -- the fixed-z0 partial plus the pullback of the draw."""
    case, dense, train, cfg, (flat, _, eps, ys), mean, scale, _, rng = BG.case_setup(name)
    B, n_in = case.B, cfg.n_in
    seed = 123
    nrm = np.random.default_rng(seed).standard_normal((B, n_in)).astype(np.float32).T       # what the model's rng will draw
    cz, cl = R.cotangents(rng, n_in, case.nvars, B)["both"]
    base = _base(mean, scale, dense, requires_grad=True, device=device)
    icnf = _model(case, base, rng=seed)
    try:
        ps = _dev(flat).requires_grad_(True)
        xs, logq = cnf.differentiable_generate(icnf, _mode(train), ps, {}, B, ys=_dev(ys) if ys is not None else None,
                                               eps=_dev(eps) if train else None)
        dts = _steps_are_the_reference(case, icnf, -1.0)
        z0_dev = _np(icnf._record["zb"].view())
        out = (_dev(cz) * xs).sum() + (_dev(cl) * logq).sum()
        gp, gm, gs = torch.autograd.grad(out, (ps, base.mean_t, base.scale_t))
    finally:
        icnf.close()
    assert gm.device.type == device and gm.shape == base.mean_t.shape and gs.shape == base.scale_t.shape
    helpers.assert_parity(z0_dev, BG.drawn_z0(nrm, mean, scale, dense), f"{name}: the draw against mean + L n")
    a = (cfg, flat, nrm, eps if train else None, cz, cl, dts, mean, scale, dense, ys, train)
    r64, r32 = BG.sampling_drawn(*a, dtype=np.float64), BG.sampling_drawn(*a, dtype=np.float32)
    _assert_base((_np(gm), _np(gs)), r64[:2], r32[:2], BG.summands_of(r64[1], np.sum(cl, dtype=np.float64), scale, dense),
                   f"drawn z0 {name}")
    assert np.isfinite(_np(gp)).all() and _np(gp).any()


# ---- 4: the pullback of the draw alone ----
@pytest.mark.parametrize("dense", [False, True], ids=["diag", "dense"])
@pytest.mark.parametrize("n_in", [3, 16, 17, 33])
def test_sample_pullback_against_einsum(n_in, dense):
    """cnf_base_sample_pullback at B in {1, 17, 300} (and 5000: 64 chunks of more than 64 samples) on one handle, the batches
    growing and shrinking, against torch.einsum in float64; twice, the same bits."""
    nvars = 2 if n_in == 3 else n_in
    mean, scale = BG.base_of(n_in, dense, 40 + n_in)
    nn = cnf.Chain(cnf.Dense(n_in, 8, "tanh"), cnf.Dense(8, n_in, "tanh"))
    icnf = cnf.construct(cnf.FFJORD, nn, nvars, n_in - nvars, basedist=_base(mean, scale, dense))
    rng = np.random.default_rng(n_in)
    try:
        for B in (17, 5000, 300, 1):
            nrm, g = rng.standard_normal((n_in, B)).astype(np.float32), rng.standard_normal((n_in, B)).astype(np.float32)
            got = cnf.base_sample_pullback(icnf, _dev(nrm), _dev(g))
            again = cnf.base_sample_pullback(icnf, _dev(nrm), _dev(g))
            assert _same(got, again)
            refs = []
            for t in (torch.float64, torch.float32):
                tn, tg = torch.from_numpy(nrm).to(t), torch.from_numpy(g).to(t)
                M = torch.einsum("ib,jb->ij", tg, tn)
                refs.append((tg.sum(1).double().numpy(), (torch.tril(M) if dense else torch.diagonal(M)).double().numpy()))
            _assert_base(tuple(_np(x) for x in got), refs[0], refs[1], None, f"sample pullback n_in={n_in} B={B}")
            if dense:
                assert not np.triu(_np(got[1]), 1).any()
    finally:
        icnf.close()


def test_kind_change_on_a_live_handle():
    """n_in = 176 (11 row blocks: 66 dense tiles, more than the 64 words a diagonal plan's tickets are rounded to): a diagonal
    base at a large batch, then a dense one at a small batch on the same handle -- the buffer does not grow, so the dense
    call's tickets must not be where the diagonal call left results -- and back."""
    n_in = 176
    nn = cnf.Chain(cnf.Dense(n_in, 8, "tanh"), cnf.Dense(8, n_in, "tanh"))
    bases = {dense: _base(*BG.base_of(n_in, dense, 60 + dense), dense) for dense in (False, True)}
    icnf = cnf.construct(cnf.FFJORD, nn, n_in, 0, basedist=bases[False])
    rng = np.random.default_rng(3)
    try:
        for dense, B in ((False, 5000), (True, 17), (False, 300), (True, 40)):
            icnf.basedist = bases[dense]
            icnf.set_basedist()
            nrm, g = rng.standard_normal((n_in, B)).astype(np.float32), rng.standard_normal((n_in, B)).astype(np.float32)
            got = cnf.base_sample_pullback(icnf, _dev(nrm), _dev(g))
            refs = []
            for t in (torch.float64, torch.float32):
                tn, tg = torch.from_numpy(nrm).to(t), torch.from_numpy(g).to(t)
                M = torch.einsum("ib,jb->ij", tg, tn)
                refs.append((tg.sum(1).double().numpy(), (torch.tril(M) if dense else torch.diagonal(M)).double().numpy()))
            _assert_base(tuple(_np(x) for x in got), refs[0], refs[1], None, f"kind change n_in={n_in} dense={dense} B={B}")
    finally:
        icnf.close()


# ---- the built-in loss ----
@pytest.mark.parametrize("name", ["n3-diag-B17", "n17-dense-B300", "n33-dense-B17-test", "headline-dense-B33"])
def test_loss_and_grad_with_base(name):
    """``loss_and_grad(with_base=True)``: the density direction with the cotangent -1/B; loss and the other gradients are the
    bits of the call without it."""
    case, dense, train, cfg, (flat, xs, eps, ys), mean, scale, _, _ = BG.case_setup(name)
    icnf = _model(case, _base(mean, scale, dense))
    kw = dict(eps=_dev(eps)) if train else {}
    try:
        v0, g0, x0 = cnf.loss_and_grad(icnf, _mode(train), _dev(xs), *_args(flat, ys), with_x=True, **kw)
        v, g, x, (gm, gs) = cnf.loss_and_grad(icnf, _mode(train), _dev(xs), *_args(flat, ys), with_x=True, with_base=True, **kw)
        dts = _steps_are_the_reference(case, icnf)
    finally:
        icnf.close()
    assert v == v0 and _same((g, x), (g0, x0))
    w = np.full(case.B, -1.0 / case.B)
    r64 = BG.density(cfg, flat, xs, eps, w, dts, mean, scale, dense, ys, train, np.float64)
    r32 = BG.density(cfg, flat, xs, eps, w, dts, mean, scale, dense, ys, train, np.float32)
    _assert_base((_np(gm), _np(gs)), r64, r32, BG.summands_of(r64[1], -1.0, scale, dense), f"loss_and_grad {name}")


def test_autograd_through_inference_reaches_the_base():
    """``differentiable_inference`` and ``icnf(xs, ps, st)`` back-propagate into mean and std = log_std.exp(); an in-place
    update of the mean is uploaded before the next solve (the rule of ``set_cond``)."""
    name = "n17-dense-B300"
    case, dense, train, cfg, (flat, xs, eps, ys), mean, scale, _, rng = BG.case_setup(name)
    w = BG.cotangents_w(rng, case.B)[0]
    mean_t = torch.tensor(mean, requires_grad=True)
    raw = torch.tensor(scale, device="cuda", requires_grad=True)
    base = cnf.LearnableNormal(mean_t, scale_tril=raw * 1.0)          # (a non-leaf scale: the gradient flows on to `raw`)
    icnf = _model(case, base)
    try:
        logpx, _ = cnf.differentiable_inference(icnf, cnf.TrainMode(), _dev(xs), flat, {}, eps=_dev(eps))
        dts = _steps_are_the_reference(case, icnf)
        gm, gs = torch.autograd.grad((_dev(w) * logpx).sum(), (mean_t, raw))
        l1 = _np(icnf(_dev(xs), flat, {}, eps=_dev(eps))[0])              # the Lux form takes the same route
        assert np.array_equal(l1, _np(logpx))
        with torch.no_grad():
            mean_t.add_(0.25)
        l2 = _np(cnf.inference(icnf, cnf.TrainMode(), _dev(xs), flat, {}, eps=_dev(eps))[0])
    finally:
        icnf.close()
    z64 = BG.final_state(cfg, flat, xs, eps, dts, None, True, np.float64)
    z32 = BG.final_state(cfg, flat, xs, eps, dts, None, True, np.float32)
    r64, r32 = BG.logpdf_grads(z64, w, mean, scale, dense, np.float64), BG.logpdf_grads(z32, w, mean, scale, dense, np.float32)
    _assert_base((_np(gm), _np(gs)), r64, r32, BG.summands_of(r64[1], np.sum(w, dtype=np.float64), scale, dense), "autograd inference")
    moved = BG.gauss(mean + np.float32(0.25), scale, dense).logpdf(z64) - BG.gauss(mean, scale, dense).logpdf(z64)
    # (a difference of two float32 log-densities: held to 1e-4 of their own size, against a shift of O(1))
    err = np.abs(f64(l2) - f64(l1) - moved).max()
    assert np.abs(moved).max() > 0.1 and err <= 1e-4 * np.abs(l1).max(), (err, np.abs(moved).max(), np.abs(l1).max())


# ---- 8, 9: reverse KL on the identity flow ----
def _identity_flow(base, seed):
    nn = cnf.Chain(cnf.Dense(3, 8, "tanh"), cnf.Dense(8, 3, "identity"))
    icnf = cnf.construct(cnf.FFJORD, nn, 3, 0, tspan=(0.0, 1.0), sol_kwargs=dict(adaptive=False, dt=0.5), rng=seed, basedist=base)
    ps = 0.3 * np.random.default_rng(1).standard_normal(nn.n_params_internal).astype(np.float32)
    ps[3 * 8 + 8:] = 0.0                                    # the last layer: W_2 = 0, b_2 = 0
    return icnf, _dev(ps)


def test_reverse_kl_on_the_identity_flow_is_the_closed_form():
    """With a zero last layer xs = z0 = mu + sigma n and dlogp = 0: ``loss.backward()`` through ``reverse_kl`` to N(m, s^2)
    gives mean_b (mu + sigma n_b - m) / s^2 and mean_b (-1 / sigma + n_b (mu + sigma n_b - m) / s^2)."""
    B, seed = 300, 77
    rng = np.random.default_rng(5)
    mu, sig = rng.standard_normal(3).astype(np.float32), rng.uniform(0.5, 1.5, 3).astype(np.float32)
    m, s = rng.standard_normal(3), rng.uniform(0.5, 2.0, 3)
    nrm = np.random.default_rng(seed).standard_normal((B, 3)).astype(np.float32).T
    md, sd = _dev(m)[:, None], _dev(s)[:, None]
    target = lambda x: -0.5 * (((x - md) / sd) ** 2).sum(0)
    mean_t, std_t = torch.tensor(mu, requires_grad=True), torch.tensor(sig, requires_grad=True)
    icnf, ps = _identity_flow(cnf.LearnableNormal(mean_t, std=std_t), seed)
    try:
        loss = cnf.reverse_kl(icnf, cnf.TrainMode(), ps, {}, B, target)
        loss.backward()
    finally:
        icnf.close()
    r = (f64(mu)[:, None] + f64(sig)[:, None] * f64(nrm) - m[:, None]) / s[:, None] ** 2
    rm, rs = r.mean(1), (-1.0 / f64(sig)[:, None] + f64(nrm) * r).mean(1)
    quad, logdet = (f64(nrm) * r).mean(1), -1.0 / f64(sig)
    for what, g, ref, sc in (("mean", mean_t.grad, rm, BG.V.scale(rm)),
                             ("std", std_t.grad, rs, max(BG.V.scale(rs), np.abs(quad).max(), np.abs(logdet).max()))):
        err = np.abs(f64(_np(g)) - ref).max() / sc
        print(f"identity-flow reverse KL d/d{what}: {err:.2e} of its scale")
        assert err <= 1e-4, (what, err)


def test_adam_on_the_base_lowers_the_reverse_kl():
    """Forty Adam steps on (mean, log_std) of the base under an identity flow, towards N(m, s^2) shifted and scaled away from
    N(0, I): the KL divergence (known in closed form for two diagonal Gaussians) falls to under a fifth of where it began."""
    B = 256
    m, s = np.array([1.5, -1.0, 0.5]), np.array([0.5, 2.0, 1.25])
    md, sd = _dev(m)[:, None], _dev(s)[:, None]
    target = lambda x: -0.5 * (((x - md) / sd) ** 2).sum(0) - torch.log(sd).sum()
    mean_t = torch.zeros(3, requires_grad=True)
    log_std = torch.zeros(3, requires_grad=True)
    kl = lambda: float((np.log(s) - f64(_np(log_std)) + (np.exp(2 * f64(_np(log_std))) + (f64(_np(mean_t)) - m) ** 2) / (2 * s * s) - 0.5).sum())
    base = cnf.LearnableNormal(mean_t, std=log_std.exp())
    icnf, ps = _identity_flow(base, 9)
    opt = torch.optim.Adam([mean_t, log_std], lr=0.1)
    kl0 = kl()
    try:
        for _ in range(40):
            opt.zero_grad()
            base.update(mean_t, std=log_std.exp())
            loss = cnf.reverse_kl(icnf, cnf.TrainMode(), ps, {}, B, target)
            loss.backward()
            opt.step()
    finally:
        icnf.close()
    print(f"reverse KL of the base: {kl0:.4f} -> {kl():.4f}")
    helpers.note(f"base-grad Adam on (mean, log_std), identity flow, 40 steps, B = {B}: KL {kl0:.4f} -> {kl():.4f}")
    assert kl() < 0.2 * kl0, (kl0, kl())


# ---- the protocol ----
def test_protocol_errors():
    case, dense, train, cfg, (flat, xs, eps, _), mean, scale, nrm, _ = BG.case_setup("n3-diag-B17")
    B = case.B
    w = _dev(np.full(B, 1.0 / B, np.float32))

    def refused(fn, *a, **kw):
        with pytest.raises(cnf.CNFError) as e:
            fn(*a, **kw)
        assert e.value.status == _lib.ERR_BAD_ARG, e.value

    icnf = _model(case, _base(mean, scale, dense))
    plain = _model(case, None)
    try:
        refused(cnf.base_logpdf_pullback, icnf, w)                                  # no record
        cnf.inference_record(icnf, cnf.TrainMode(), _dev(xs), flat, {}, eps=_dev(eps))
        g0 = cnf.base_logpdf_pullback(icnf, w)
        refused(cnf.base_logpdf_pullback, icnf, w[:B - 1])                          # another B
        assert _same(cnf.base_logpdf_pullback(icnf, w), g0)                         # (the record survives refused calls)
        cnf.inference(icnf, cnf.TrainMode(), _dev(xs), flat, {}, eps=_dev(eps))
        refused(cnf.base_logpdf_pullback, icnf, w)                                  # displaced by another solve
        l, h = _lib.lib(), icnf.handle()
        out = torch.empty(8, dtype=torch.float32, device="cuda")
        assert l.cnf_base_logpdf_pullback(h, None, B, out.data_ptr(), out.data_ptr(), None) == _lib.ERR_BAD_ARG      # NULL
        assert l.cnf_base_sample_pullback(h, w.data_ptr(), None, B, out.data_ptr(), out.data_ptr(), None) == _lib.ERR_BAD_ARG
        # the default base has no mean and no chol
        cnf.inference_record(plain, cnf.TrainMode(), _dev(xs), flat, {}, eps=_dev(eps))
        hp = plain.handle()
        big = torch.empty(3 * B, dtype=torch.float32, device="cuda")
        assert l.cnf_base_logpdf_pullback(hp, w.data_ptr(), B, out.data_ptr(), out.data_ptr(), None) == _lib.ERR_BAD_ARG
        assert l.cnf_base_sample_pullback(hp, big.data_ptr(), big.data_ptr(), B, out.data_ptr(), out.data_ptr(), None) == _lib.ERR_BAD_ARG
    finally:
        icnf.close()
        plain.close()
