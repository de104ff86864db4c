"""The gradient w.r.t. the conditioning inputs ``ys`` on the device (cnf_set_grad_ys / cnf_grad_ys, ``with_ys=True``) against the
float64 reference of tests/cond_grad_ref.py, on every pullback route a conditional model can take.

Cases: the four conditional cases of ``grad_terms.GPU_CASES`` (all fixed-dt: the reference takes the same steps and the device
must have taken as many), lam = (1, 1, 1) ((1, 1, 0) without augmented rows) so that every output row exists.

Bar (tests/vjp_ref.py's, unchanged, on the one block grad_ys):  max|got - ref64| <= rtol (max|ref64| + rms ref64),
rtol = max(1e-4, 8 floor) <= 1e-3, floor = the float32 run of the same reference against its float64 run.
"""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from continuousnf.jl_amd.base_icnf import _as_colmajor, _solve_opts
from oracle import cnf_oracle as O
from tests import cond_grad_ref as R
from tests import grad_terms as GT
from tests import vjp_ref as V
from tests.test_gpu_grad_terms import _forced_split, _model
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TRAIN, TEST = cnf.TrainMode(), cnf.TestMode()
f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
WAVE, ADJ3, VJP, JVP = R.COND_CASES
GENERIC = dataclasses.replace(GT.GPU_CASES[VJP], name="generic-12x64x48-cond", route="generic", kernel="generic")
CASES = dict({n: GT.GPU_CASES[n] for n in R.COND_CASES}, **{GENERIC.name: GENERIC})


def _lam(case):
    return (1.0, 1.0, 1.0 if case.naugs else 0.0)


def _np(t):
    return t.detach().cpu().numpy()


def _args(inputs):
    flat, xs, eps, ys = inputs
    return (_dev(ys), flat, {})


def _ref(case, cot, tag, train=True):
    """(ref64, ref32) of grad_ys and the reference's (grad, grad_x) in float64."""
    cfg, r64, r32 = R.case_reference(case, cot, train, _lam(case), tag=tag)
    return r64, r32


def _steps_ok(case, icnf):
    assert len(icnf.last_steps) == len(R.case_dts(case)), (case.name, icnf.last_steps)


def _block_bar(got, ref, net, what, rtol):
    for n, sl in GT.param_blocks(net).items():
        s = V.scale(ref[sl])
        err = float(np.abs(f64(got[sl]) - f64(ref[sl])).max())
        print(f"{what} {n}: {err / max(s, 1e-300):.3e} of its scale")
        assert np.isfinite(err) and err <= rtol * s, f"{what} {n}: off by {err / max(s, 1e-300):.3g} of its scale (rtol {rtol:g})"


def _loss_leg(case, icnf, inputs, what):
    """loss_and_grad with and without with_ys: the same gradient (1e-4 per block), gy against the reference."""
    flat, xs, eps, ys = inputs
    v0, g0 = cnf.loss_and_grad(icnf, TRAIN, _dev(xs), *_args(inputs), eps=_dev(eps))
    v, g, gx, gy = cnf.loss_and_grad(icnf, TRAIN, _dev(xs), *_args(inputs), eps=_dev(eps), with_x=True, with_ys=True)
    st = dict(icnf.last_stats)
    _steps_ok(case, icnf)
    assert gy.shape == ys.shape and gx.shape == xs.shape
    assert abs(v - v0) <= 1e-5 * max(1.0, abs(v0)), (what, v, v0)
    _block_bar(_np(g), _np(g0), case.net, f"{what}: grad with / without with_ys", 1e-4)
    cot = V.loss_cotangent(case.cfg(_lam(case)), case.B)
    r64, r32 = _ref(case, cot, "loss")
    R.assert_ys(_np(gy), r64[3], r32[3], f"{what} cot=loss")
    return st


def _pull(icnf, cot):
    g, gx, gy = cnf.inference_pullback(icnf, _dev(np.asarray(cot, np.float32)), with_x=True, with_ys=True)
    return _np(g), _np(gx), _np(gy)


def _record(icnf, inputs, mode=TRAIN):
    flat, xs, eps, ys = inputs
    cnf.inference_record(icnf, mode, _dev(xs), *_args(inputs), eps=_dev(eps) if mode is TRAIN else None)


def _rows_leg(case, icnf, inputs, what):
    """One record: each output row alone and all together, a one-hot-sample cotangent, and the first cotangent again."""
    B = case.B
    _record(icnf, inputs)
    _steps_ok(case, icnf)
    rows = (0, 1, 2, 3) if case.naugs else (0, 1, 2)
    cots = V.row_cotangents(np.random.default_rng(case.seed + 7), B, rows)
    got = {k: _pull(icnf, c) for k, c in cots.items()}
    full_scale = None
    for k, c in cots.items():
        r64, r32 = _ref(case, c, f"row-{k}")
        R.assert_ys(got[k][2], r64[3], r32[3], f"{what} cot={k}")
        V.assert_vjp(got[k][0], got[k][1], (r64[1], r64[2]), (r32[1], r32[2]), case.net, f"{what} cot={k} (with_ys on)")
        if k == "all":
            full_scale = V.scale(r64[3])
    # accumulator hygiene: the first cotangent again after four others -- nothing of them may be left (bit for bit)
    first = next(iter(cots))
    again = _pull(icnf, cots[first])
    assert np.array_equal(again[2], got[first][2]) and np.array_equal(again[0], got[first][0]), f"{what}: a later pullback contains an earlier one"
    # one sample only
    j = min(5, B - 1)
    hot = np.zeros((4, B), np.float32)
    hot[:, j] = [0.3, -0.2, 0.1, 0.05 if case.naugs else 0.0]
    gy = _pull(icnf, hot)[2]
    r64, r32 = _ref(case, hot, "one-hot")
    R.assert_ys(gy, r64[3], r32[3], f"{what} cot=one-hot")
    others = np.abs(np.delete(gy, j, axis=1)).max() if B > 1 else 0.0
    print(f"{what}: one-hot sample {j}: largest entry of the other columns {others:.3e} (expected exactly 0)")
    assert others <= 1e-4 * full_scale, (what, others, full_scale)


ROUTES = [(ADJ3, None), (VJP, 0), (VJP, 1), (JVP, 0), (JVP, 1), (GENERIC.name, None), (WAVE, None)]


@pytest.mark.parametrize("name,split", ROUTES, ids=[n if s is None else f"{n}-split{s}" for n, s in ROUTES])
def test_routes(name, split):
    """k_adj3, k_adj_mfma VJP / JVP in both launch forms, the generic adjoint, and the small network on the recorded route."""
    case = CASES[name]
    inputs = case.inputs()
    what = name if split is None else f"{name} split={split}"
    with _forced_split(split):
        icnf = _model(case, _lam(case))
        try:
            st = _loss_leg(case, icnf, inputs, what)
            if case.route == "wave":            # the gradient did not run in the launch of the solve (<= 2 launches there)
                assert st["launches"] > 2, (what, st)
            elif case.route == "generic":
                assert st["kernel_used"] == _lib.KERNEL_GENERIC, (what, st)
            else:
                assert st["kernel_used"] == _lib.KERNEL_MFMA, (what, st)
            _rows_leg(case, icnf, inputs, what)
        finally:
            icnf.close()


@pytest.mark.parametrize("name", [WAVE, VJP])
def test_testmode(name):
    """k_adj_test: the TestMode loss, a per-sample cotangent of logpx from a record, and one sample alone."""
    case = CASES[name]
    inputs = case.inputs()
    flat, xs, eps, ys = inputs
    B = case.B
    icnf = _model(case, _lam(case))
    try:
        v0, g0 = cnf.loss_and_grad(icnf, TEST, _dev(xs), *_args(inputs))
        v, g, gx, gy = cnf.loss_and_grad(icnf, TEST, _dev(xs), *_args(inputs), with_x=True, with_ys=True)
        assert icnf.last_stats["launches"] > 2, icnf.last_stats
        _steps_ok(case, icnf)
        assert abs(v - v0) <= 1e-5 * max(1.0, abs(v0))
        _block_bar(_np(g), _np(g0), case.net, f"TestMode {name}: grad with / without with_ys", 1e-4)
        r64, r32 = _ref(case, V.loss_cotangent(case.cfg(_lam(case)), B, train=False), "loss", train=False)
        R.assert_ys(_np(gy), r64[3], r32[3], f"TestMode {name} cot=loss")
        _record(icnf, inputs, TEST)
        cot = np.zeros((4, B), np.float32)
        cot[0] = (np.random.default_rng(case.seed + 9).standard_normal(B) / B).astype(np.float32)
        got = _pull(icnf, cot)
        hot = np.zeros((4, B), np.float32)
        hot[0, 5] = 0.3
        ghot = _pull(icnf, hot)[2]
        again = _pull(icnf, cot)
    finally:
        icnf.close()
    r64, r32 = _ref(case, cot, "row-logpx", train=False)
    R.assert_ys(got[2], r64[3], r32[3], f"TestMode {name} cot=logpx")
    V.assert_vjp(got[0], got[1], (r64[1], r64[2]), (r32[1], r32[2]), case.net, f"TestMode {name} cot=logpx (with_ys on)")
    full_scale = V.scale(r64[3])
    r64, r32 = _ref(case, hot, "one-hot", train=False)
    R.assert_ys(ghot, r64[3], r32[3], f"TestMode {name} cot=one-hot")
    others = np.abs(np.delete(ghot, 5, axis=1)).max()
    print(f"TestMode {name}: one-hot sample: largest entry of the other columns {others:.3e} (expected exactly 0)")
    assert others <= 1e-4 * full_scale
    assert np.array_equal(again[2], got[2]), "a later pullback contains an earlier one"


def test_cond_planar():
    """CondPlanar at the sizes of test/call_tests.jl (nvars = 2, 4 samples, 2 conditioning rows): its internal network
    (n_in + n_cond) -> 1 -> n_in has ys in the first fan-in like any other."""
    nvars, B, n_cond = 2, 4, 2
    rng = np.random.default_rng(2024)
    chain = cnf.Chain(cnf.PlanarLayer(nvars, "tanh", n_cond=n_cond))
    flat = cnf.setup(7, chain)[0]
    flat[-1] = 0.2                                            # (a bias away from its zero initialisation)
    xs = rng.standard_normal((nvars, B)).astype(np.float32)
    ys = rng.standard_normal((n_cond, B)).astype(np.float32)
    eps = rng.standard_normal((nvars, B)).astype(np.float32)
    kw = dict(adaptive=False, dt=0.125)
    icnf = cnf.construct(cnf.CondPlanar, chain, nvars, 0, tspan=(0.0, 1.0), sol_kwargs=kw)
    try:
        v, g, gy = cnf.loss_and_grad(icnf, TRAIN, _dev(xs), _dev(ys), flat, {}, eps=_dev(eps), with_ys=True)
        steps = [abs(float(d)) for d in icnf.last_steps]
        vt, gt, gyt = cnf.loss_and_grad(icnf, TEST, _dev(xs), _dev(ys), flat, {}, with_ys=True)
        net = O.Net(tuple(icnf.nn.dims), tuple(icnf.nn.acts))
        internal = np.asarray(icnf.nn.to_internal(flat), np.float32)
    finally:
        icnf.close()
    assert len(steps) == 8 and net.dims == (nvars + n_cond, 1, nvars)
    cfg = O.Cfg(net, nvars, 0, tspan=(0.0, 1.0))
    for train, got, e in ((True, gy, eps), (False, gyt, None)):
        cot = V.loss_cotangent(cfg, B, train)
        r64 = R.vjp_ys64(cfg, internal, xs, e, cot, steps, ys, train)
        r32 = R.vjp_ys32(cfg, internal, xs, e, cot, steps, ys, train)
        R.assert_ys(_np(got), r64[3], r32[3], f"CondPlanar train={train}")


def _resized(case, B, tag):
    return dataclasses.replace(case, B=B, name=f"{case.name}-{tag}-B{B}")


def test_single_sample():
    """B = 1 on the MFMA route: one row per slot."""
    case = _resized(GT.GPU_CASES[VJP], 1, "single")
    inputs = case.inputs()
    icnf = _model(case, _lam(case))
    try:
        _loss_leg(case, icnf, inputs, case.name)
    finally:
        icnf.close()


def test_smaller_batch_after_a_larger_one_on_the_same_handle():
    """B = 120 and then B = 17 on one handle: the row sums of the larger call lie where the smaller one's result goes, and the
    slot stride of the factor rows changes with B."""
    big, small = _resized(GT.GPU_CASES[VJP], 120, "after"), _resized(GT.GPU_CASES[VJP], 17, "after")
    icnf = _model(big, _lam(big))
    try:
        for case in (big, small):
            _loss_leg(case, icnf, case.inputs(), case.name)
    finally:
        icnf.close()


def test_runs_of_steps_add_up_in_a_child_process():
    """CNF_GRAD_FSTEPS=3 (read once per process) on the 8-step case: runs of 3, 3 and 2 steps -- the first stores the row sums,
    the later ones add.  One fresh child process, under its own time limit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CNF_GRAD_FSTEPS="3", CNF_NO_PARITY_REPORT="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_routes and wave"], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    assert "1 passed" in r.stdout and "failed" not in r.stdout, r.stdout[-500:]
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("grad_ys |")))


def test_autograd_trains_an_encoder_through_the_flow():
    """ys = W_enc @ ctx: torch.autograd.grad of weighted_loss w.r.t. W_enc is gy_ref @ ctx'; with a ys that asks for no
    gradient the switch is never set."""
    case = GT.GPU_CASES[VJP]
    flat, xs, eps, ys = case.inputs()
    lam = (0.01, 0.02, 0.03)
    B, n_cond, n_ctx = case.B, case.n_cond, 5
    rng = np.random.default_rng(31)
    ctx = rng.standard_normal((n_ctx, B)).astype(np.float32)
    W = np.linalg.lstsq(ctx.T, ys.T, rcond=None)[0].T.astype(np.float32)      # (some encoder; ys = W ctx is what the flow sees)
    w = rng.uniform(0.0, 2.0, B)
    fn = cnf.weighted_loss(w.astype(np.float32))
    icnf = _model(case, lam)
    try:
        l, h = _lib.lib(), icnf.handle()
        probe = torch.empty(B * n_cond, device="cuda")
        # no gradient asked of ys: the switch stays off, and cnf_grad_ys has nothing to hand out
        out = fn(icnf, TRAIN, _dev(xs), _dev(ys), _dev(flat).requires_grad_(True), {})
        out.backward()
        assert l.cnf_grad_ys(h, probe.data_ptr(), B, None) == _lib.ERR_BAD_ARG
        W_enc = _dev(W).requires_grad_(True)
        ys_t = W_enc @ _dev(ctx)
        ps = _dev(flat).requires_grad_(True)
        out = fn(icnf, TRAIN, _dev(xs), ys_t, ps, {})
        eps_used = _np(icnf._record["eb"].view())
        steps = [abs(float(d)) for d in icnf.last_steps]
        gW, gps, gys = torch.autograd.grad(out, (W_enc, ps, ys_t))
        assert gys is not None and gys.shape == ys_t.shape
        gyd = _np(gys)
        assert l.cnf_grad_ys(h, probe.data_ptr(), B, None) == _lib.OK
        ys_used = _np(ys_t)
    finally:
        icnf.close()
    cfg = case.cfg(lam)
    lv = np.array(lam)
    cot = np.concatenate([[-w / w.sum()], np.outer(lv, w / w.sum())])
    r64 = R.vjp_ys64(cfg, flat, xs, eps_used, cot, steps, ys_used)
    r32 = R.vjp_ys32(cfg, flat, xs, eps_used, cot, steps, ys_used)
    R.assert_ys(gyd, r64[3], r32[3], "autograd ys.grad")
    R.assert_ys(_np(gW), r64[3] @ f64(ctx).T, f64(r32[3]) @ f64(ctx).T, "autograd d loss / d W_enc")
    V.assert_vjp(_np(gps), None, (r64[1], r64[2]), (r32[1], r32[2]), case.net, "autograd d loss / d ps beside ys")


def test_default_path_is_untouched():
    """Switch off: the small network's gradient runs in the launch of the solve, bit for bit what it gave before any
    with_ys call on the handle; submitted gradients work; the switch on refuses them at once; an unconditional handle has no
    switch."""
    case = GT.GPU_CASES[WAVE]
    inputs = case.inputs()
    flat, xs, eps, ys = inputs
    B = case.B
    icnf = _model(case, _lam(case))
    try:
        dx, dy, de, dp = _dev(xs), _dev(ys), _dev(eps), _dev(flat)
        l, h = _lib.lib(), icnf.handle()
        probe = torch.empty(B * case.n_cond, device="cuda")
        assert l.cnf_grad_ys(h, probe.data_ptr(), B, None) == _lib.ERR_BAD_ARG            # no gradient has run
        v0, g0 = cnf.loss_and_grad(icnf, TRAIN, dx, dy, dp, {}, eps=de)
        assert icnf.last_stats["launches"] <= 2, icnf.last_stats
        assert l.cnf_grad_ys(h, probe.data_ptr(), B, None) == _lib.ERR_BAD_ARG            # the switch was off during it
        g0 = g0.clone()
        cnf.loss_and_grad(icnf, TRAIN, dx, dy, dp, {}, eps=de, with_ys=True)
        assert icnf.last_stats["launches"] > 2, icnf.last_stats
        assert l.cnf_grad_ys(h, probe.data_ptr(), B - 1, None) == _lib.ERR_BAD_ARG        # another B
        assert l.cnf_grad_ys(h, probe.data_ptr(), B, None) == _lib.OK
        v1, g1 = cnf.loss_and_grad(icnf, TRAIN, dx, dy, dp, {}, eps=de)
        assert icnf.last_stats["launches"] <= 2, icnf.last_stats
        assert v1 == v0 and torch.equal(g1, g0)
        assert l.cnf_grad_ys(h, probe.data_ptr(), B, None) == _lib.ERR_BAD_ARG
        lossd, gs = cnf.loss_and_grad_submit(icnf, TRAIN, dx, dy, dp, {}, eps=de)
        cnf.loss_and_grad_collect(icnf)
        torch.cuda.synchronize()
        assert float(lossd[0]) == np.float32(v0) and torch.equal(gs, g0)
        # the switch on: a submitted gradient is refused at once, nothing is enqueued
        assert l.cnf_set_grad_ys(h, 1) == _lib.OK
        out = torch.empty(flat.size + 1, device="cuda")
        opts = _solve_opts(icnf, icnf.tspan)
        cx, ce = _as_colmajor(dx, icnf.nvars), _as_colmajor(de, case.nvars + case.naugs)
        rc = l.cnf_loss_grad_submit(h, _lib.MODE_TRAIN, cx.ptr, ce.ptr, B, C.byref(opts), out[-1:].data_ptr(), out.data_ptr(), None)
        assert rc == _lib.ERR_UNSUPPORTED and l.cnf_inference_pending(h) == 0
        assert l.cnf_set_grad_ys(h, 0) == _lib.OK
    finally:
        icnf.close()
    plain = GT.GPU_CASES["generic-cfg2"]
    icnf = _model(plain, _lam(plain))
    try:
        assert _lib.lib().cnf_set_grad_ys(icnf.handle(), 1) == _lib.ERR_BAD_ARG
        assert _lib.lib().cnf_set_grad_ys(icnf.handle(), 0) == _lib.ERR_BAD_ARG
        pf, px, pe, _ = plain.inputs()
        with pytest.raises(ValueError):
            cnf.loss_and_grad(icnf, TRAIN, _dev(px), pf, {}, eps=_dev(pe), with_ys=True)
    finally:
        icnf.close()
