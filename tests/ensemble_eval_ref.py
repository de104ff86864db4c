"""What tests/test_ensemble_eval_host.py and tests/test_gpu_ensemble_eval.py share: the cases of ensemble inference and sampling,
their inputs, and the oracle replays (float64 for the reference, float32 for the floor) on a given list of signed steps.

Every GPU case is listed here so that the host test can hold each to the float32 floor: the float32 oracle on the case's inputs
and fixed steps against its float64 run passes the parity bar of tests/helpers.py with at least 4x to spare, i.e. no device case
sits at its bar for reasons of float32 alone.  For an adaptive case the fixed steps are the ones the float64 oracle's own
controller takes at the case's tolerances (the device takes its own, of the same sizes)."""
from __future__ import annotations

import numpy as np

from oracle import cnf_oracle as O
from tests import gen_vjp_ref as GR

TANH2 = (O.ACT_TANH,) * 2
ID2 = (O.ACT_TANH, O.ACT_IDENTITY)
README = O.Cfg(O.Net((2, 6, 2), TANH2), 1, 1, 1e-2, 1e-2, 1e-2)
REGR = O.Cfg(O.Net((16, 48, 16), TANH2), 8, 8, 1e-2, 1e-2, 1e-2)
WIDE = O.Cfg(O.Net((16, 64, 16), TANH2), 10, 6, 0.0, 1e-2, 5e-2)
REV = O.Cfg(O.Net((7, 13, 7), TANH2), 4, 3, 1e-2, 1e-2, 1e-2)
REV0 = O.Cfg(O.Net((7, 13, 7), TANH2), 7, 0, 1e-2, 1e-2, 0.0)
ONE = O.Cfg(O.Net((6, 1, 6), ID2), 6, 0, 1e-2, 1e-2, 0.0)

DEFAULT_TOL = dict(abstol=1e-6, reltol=1e-3)             # (OrdinaryDiffEq's, and _solve_opts')

# (network, tspan, M, B, train, jvp, sol_kwargs): the networks of tests/test_gpu_ensemble.py, M in {1, 2, 5}, B in {1, 16, 17, 33,
# 80}, the three modes, fixed and adaptive steps; tspan (0, 13) once; a reversed span; lambda3 with augmentation and without
INFERENCE_CASES = [
    (README, (0.0, 13.0), 5, 33, True, False, dict()),
    (README, None, 1, 80, True, True, dict()),
    (README, None, 2, 16, False, False, dict(adaptive=False, dt=1 / 5)),
    (REGR, None, 2, 17, True, False, dict()),
    (REGR, None, 2, 16, True, True, dict(adaptive=False, dt=1 / 6)),
    (REGR, None, 2, 33, False, False, dict()),
    (WIDE, None, 5, 1, True, False, dict(adaptive=False, dt=1 / 5)),
    (WIDE, None, 2, 80, False, False, dict(adaptive=False, dt=1 / 5)),
    (REV, (1.0, 0.0), 2, 17, True, False, dict(adaptive=False, dt=1 / 4)),
    (REV0, (1.0, 0.0), 1, 16, False, False, dict()),
    (ONE, None, 5, 33, True, False, dict(adaptive=False, dt=1 / 5)),
    (ONE, None, 2, 17, True, True, dict()),
    (ONE, None, 1, 16, False, False, dict(adaptive=False, dt=1 / 5)),
]
# sampling: (network, tspan, M, n, train, jvp, sol_kwargs); the user's span is what the model is built with, the solve runs over
# its reverse
GENERATE_CASES = [
    (README, None, 2, 80, True, False, dict()),
    (README, None, 5, 16, False, False, dict(adaptive=False, dt=1 / 5)),
    (REGR, None, 2, 33, True, True, dict(adaptive=False, dt=1 / 6)),
    (REGR, None, 1, 17, False, False, dict()),
    (REV, (1.0, 0.0), 2, 17, True, False, dict(adaptive=False, dt=1 / 4)),
    (ONE, None, 2, 33, False, False, dict(adaptive=False, dt=1 / 5)),
]
# the one-off inputs of the other GPU tests, (name, network, tspan, train, seed, M, B, scales, sol_kwargs), listed for the floor
OTHER_CASES = [
    ("stiff member", REGR, (0.0, 6.0), True, 926, 3, 40, (3.0, 1.0, 1.0), dict(dt=3.0, reltol=1e-4, abstol=1e-6)),
    ("offsets", REGR, None, True, 77, 3, 17, None, dict()),
    ("single call", REGR, None, True, 78, 2, 80, None, dict(adaptive=False, dt=1 / 6)),
    ("single call, one workgroup", README, None, True, 90, 2, 33, None, dict(adaptive=False, dt=1 / 5)),
    ("handle afterwards", REGR, None, True, 84, 3, 33, None, dict()),
]
OTHER = {c[0]: c for c in OTHER_CASES}
FIXED4 = dict(adaptive=False, dt=1 / 4)
# ... with per-member end times: (name, network, seed, M, B, sol_kwargs, t1 per member or None), TrainMode
END_TIME_CASES = [
    ("end times, fixed", README, 79, 3, 17, FIXED4, (0.6, 1.0, 1.7)),
    ("end times, adaptive", README, 79, 3, 17, dict(), (0.6, 1.0, 1.7)),
    ("rerun", REGR, 82, 2, 33, FIXED4, None),
]
END_TIME = {c[0]: c for c in END_TIME_CASES}
# ... and of sampling: (name, network, seed, M, n, train, sol_kwargs, start time per member or None); "re-scoring" is held to
# the solver tolerance RESCORE_RTOL on the device (two solves with their own step sequences), and so is its floor
RESCORE_RTOL = 5e-3
RESCORE_TOL = dict(reltol=1e-5, abstol=1e-7)
START_TIME_CASES = [
    ("rerun", REGR, 82, 2, 33, True, FIXED4, None),
    ("start times", README, 96, 3, 17, True, dict(), (0.7, 1.0, 1.4)),
    ("re-scoring 7-13-7", REV0, 95, 3, 33, False, RESCORE_TOL, None),
    ("re-scoring 6-1-6", ONE, 95, 3, 33, False, RESCORE_TOL, None),
]
START_TIME = {c[0]: c for c in START_TIME_CASES}
# (the remaining device tests compare the device with itself, bit for bit or against a twin's single call: no float64 reference)


def cfg_of(cfg, tspan=None, jvp=False):
    return O.Cfg(cfg.net, cfg.nvars, cfg.naugs, cfg.lam1, cfg.lam2, cfg.lam3, use_jvp=jvp, tspan=tspan or cfg.tspan)


def members(cfg, M, B, seed, scale=0.5, scales=None):
    """Different parameters, data and probes per member (float32): ps (M, n_params), xs (M, nvars, B), eps (M, n_in, B);
    ``scales``: a factor on each member's parameters."""
    rng = np.random.default_rng(seed)
    ps = np.stack([O.glorot_params(cfg.net, rng, np.float32, scale) for i in range(M)])
    if scales is not None:
        ps = (ps * np.asarray(scales, dtype=np.float32)[:, None]).astype(np.float32)
    xs = rng.standard_normal((M, cfg.nvars, B)).astype(np.float32)
    eps = rng.standard_normal((M, cfg.n_in, B)).astype(np.float32)
    return ps, xs, eps


def steered_model(cnf, seed):
    """The README network with steer_rate = 0.1 on a host generator, fixed steps (the last one clipped to the drawn time)."""
    layers = [cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh")]
    return cnf.construct(cnf.RNODE, cnf.Chain(*layers), 1, 1, compute_mode=cnf.HIPVecJacMatrixMode("mfma"), tspan=(0.0, 1.0),
                         sol_kwargs=dict(FIXED4), steer_rate=0.1, lambda1=1e-2, lambda2=1e-2, lambda3=1e-2, rng=seed)


def base_draws(cfg, M, n, seed):
    return np.random.default_rng(seed + 11).standard_normal((M, cfg.n_in, n)).astype(np.float32)


def replay_inference(cfg, train, ps, xs, eps, hs, dtype=np.float64):
    """One member's inference through the signed steps ``hs`` in ``dtype``: the (4, B) matrix (logpx; E; n; A) -- row 0 is the
    row derived from dlogp: helpers' ``trace_row`` -- and the loss."""
    c = lambda a: None if a is None else np.asarray(a).astype(dtype)
    f = cfg.rhs(c(ps), c(eps) if train else None, train)
    u = O.inference_u0(cfg, c(xs), train)
    k1 = f(u)
    for h in hs:
        u, k1, _ = O.tsit5_step(f, u, k1, dtype(h))
    logpx, regs = O.inference_sol(cfg, u, train)
    zero = np.zeros_like(logpx)
    rows = np.stack([logpx, regs[0] if train else zero, regs[1] if train else zero, regs[2]])
    return rows, O.loss(cfg, logpx, regs, train)


def replay_generate(cfg, train, ps, z0, eps, hs, dtype=np.float64):
    """One member's samples (nvars, n) and logq (n) through the steps ``hs`` (GR.forward: reverse(cfg.tspan), absolute sizes)."""
    c = lambda a: None if a is None else np.asarray(a).astype(dtype)
    z, logq, _, _ = GR.forward(cfg, c(ps), c(z0), c(eps) if train else None, hs, None, train)
    return z[: cfg.nvars], logq


def oracle_steps(cfg, train, ps, xs_or_z0, eps, sol_kw, generate=False):
    """The signed steps of a case on the host: the fixed ones, or the ones the float64 controller takes at the case's tolerances."""
    t0, t1 = (cfg.tspan[1], cfg.tspan[0]) if generate else cfg.tspan
    sgn = 1.0 if t1 >= t0 else -1.0
    if not sol_kw.get("adaptive", True):
        dt, span = float(sol_kw["dt"]), abs(t1 - t0)
        n = int(np.ceil(span / dt - 1e-9))
        return [sgn * min(dt, span - i * dt) for i in range(n)]
    f64 = lambda a: None if a is None else a.astype(np.float64)
    f = cfg.rhs(f64(ps), f64(eps) if train else None, train)
    if generate:
        z0 = f64(xs_or_z0)
        u0 = np.vstack([z0, np.zeros((cfg.D(train) - cfg.n_in, z0.shape[1]))])
    else:
        u0 = O.inference_u0(cfg, f64(xs_or_z0), train)
    kw = dict(DEFAULT_TOL)
    kw.update({k: v for k, v in sol_kw.items() if k in ("abstol", "reltol", "dt")})
    _, st = O.tsit5_solve(f, u0, t0, t1, **kw)
    return [sgn * d for d in st.dts]


def replay_attempts(cfg, train, ps, xs, eps, attempts, tol, t0=None, t1=None, u0=None):
    """The loop of tests/test_gpu_parity.py::test_adaptive_solves_on_their_own_step_sequence for one member: the float64 oracle
    replays the device's attempts (rows t, signed h, EEst, accepted); every decision that its own estimate puts clear of 1 by
    10 % is the device's, and the estimates agree to 15 % where both are above 1e-2.  tol None: fixed steps, nothing to decide.
    Returns the final float64 state."""
    f64 = lambda a: None if a is None else np.asarray(a).astype(np.float64)
    f = cfg.rhs(f64(ps), f64(eps) if train else None, train)
    u = O.inference_u0(cfg, f64(xs), train) if u0 is None else f64(u0)
    k1 = f(u)
    t = float(cfg.tspan[0] if t0 is None else t0)
    end = float(cfg.tspan[1] if t1 is None else t1)
    for (tg, hg, eg, ag) in np.asarray(attempts, dtype=np.float64):
        assert abs(tg - t) <= 1e-5 * max(1.0, abs(t)), (tg, t)
        un, k7, err = O.tsit5_step(f, u, k1, hg)
        if tol is not None:
            sc = tol["abstol"] + tol["reltol"] * np.maximum(np.abs(u), np.abs(un))
            eo = O._rms(err / sc)
            if eo > 1e-2 and eg > 1e-2:
                assert abs(eg / eo - 1.0) <= 0.15, (tg, hg, eg, eo)
            if abs(eo - 1.0) > 0.1:
                assert (ag > 0) == (eo <= 1.0), (tg, hg, eg, eo, ag)
        if ag > 0:
            u, k1, t = un, k7, t + hg
    assert abs(t - end) <= 1e-5 * max(1.0, abs(end)), (t, end)
    return u


def rows_of_state(cfg, u, train):
    logpx, regs = O.inference_sol(cfg, u, train)
    zero = np.zeros_like(logpx)
    return np.stack([logpx, regs[0] if train else zero, regs[1] if train else zero, regs[2]]), O.loss(cfg, logpx, regs, train)
