"""Cases and references of differentiable ensemble sampling (``generate_vjp_many``; helper module, no GPU needed).

The case list is modelled on tests/ensemble_vjp_ref.py's -- the same networks, modes, spans and step settings, M = 3 -- with the
members' own START times of the reversed span where that list has end times.  The references of one member are
tests/gen_vjp_ref.py (``vjp64``, ``vjp32``, ``cotangents``) applied member by member, held with ``vjp_ref.assert_vjp``; nothing
is restated.  tests/test_ensemble_gen_vjp_host.py checks on the CPU that the float32 floor of every case leaves the bar where
the device tests need it; tests/test_gpu_ensemble_gen_vjp.py takes its inputs from here and replays the steps each member
accepted on the device.
"""
from __future__ import annotations

import numpy as np

from oracle import cnf_oracle as O
from tests import ensemble_vjp_ref as E
from tests import gen_vjp_ref as GR
from tests import vjp_ref as V

TANH2 = E.TANH2
M = E.M
Case = E.Case                      # (its ``t1``: the members' own start times of the reversed span, generate_vjp_many's ``t0``)

# The smallest shapes at which the kernel can still go wrong.  B in {1, 17, 33}: one live column in the last tile, and three tiles
# that must meet.  Sampling integrates over reverse(tspan): from tspan[1] (or the member's own start time) to tspan[0].
CASES = [
    Case("gen-readme-vjp-B33", O.Cfg(O.Net((2, 6, 2), TANH2), 1, 1, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)), 33, seed=21, t1=(0.6, 1.0, 1.7)),
    # member 0 is stiff for a first step of half the span: it rejects attempts (the device test asserts that it does)
    Case("gen-regr-vjp-B17-rejects", O.Cfg(O.Net((16, 48, 16), TANH2), 8, 8, 1e-2, 1e-2, 1e-2, tspan=(0.0, 2.0)), 17, seed=22,
         sol_kw=dict(dt=1.0, reltol=1e-4, abstol=1e-6), wscale=(2.0, 1.0, 1.0)),
    Case("gen-regr-jvp-B33", O.Cfg(O.Net((16, 48, 16), TANH2), 8, 8, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)), 33, jvp=True, seed=23),
    Case("gen-regr-test-B17", O.Cfg(O.Net((16, 48, 16), TANH2), 8, 8, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)), 17, train=False, seed=24),
    Case("gen-noaug-vjp-B1", O.Cfg(O.Net((7, 13, 7), TANH2), 7, 0, 1e-2, 1e-2, 0.0, tspan=(1.0, 0.0)), 1, seed=25),
    Case("gen-id2-vjp-B17", O.Cfg(O.Net((6, 9, 6), (O.ACT_TANH, O.ACT_IDENTITY)), 6, 0, 1e-2, 1e-2, 0.0, tspan=(0.0, 1.0)), 17, seed=26),
    Case("gen-readme-test-B1", O.Cfg(O.Net((2, 6, 2), TANH2), 1, 1, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)), 1, train=False, seed=27),
]
IDS = [c.name for c in CASES]

member_cfg = E.member_cfg          # (the member's span: (tspan[0], its own start time); gen_vjp_ref integrates it in reverse)


def inputs(case: Case):
    """``(ps (M, n_params), z0 (M, n_in, B), eps (M, n_in, B))`` float32."""
    cfg = case.cfg
    rng = np.random.default_rng(9500 + case.seed)
    ps = np.stack([np.float32(w) * O.glorot_params(cfg.net, rng, np.float32, s) for s, w in zip(case.scales, case.wscale)])
    z0 = rng.standard_normal((M, cfg.n_in, case.B)).astype(np.float32)
    eps = rng.standard_normal((M, cfg.n_in, case.B)).astype(np.float32)
    return ps, z0, eps


def cotangents(case: Case, m: int):
    """Member m's cotangent sets: ``gen_vjp_ref.cotangents(..., aug_rows=True)`` -- ``x``, ``logq``, ``both`` and ``z-all-rows``.
    name -> (cot_z (nvars or n_in, B) or None, cot_logq (B,) or None), float32."""
    cfg = case.cfg
    return GR.cotangents(np.random.default_rng(7500 + 10 * case.seed + m), cfg.n_in, cfg.nvars, case.B, aug_rows=True)


def stack_cot(case: Case, cots, name):
    """The members' cotangent set ``name`` -> ``(g_x (M, rows, B) or None, g_logq (M, B) or None)``."""
    gx = None if cots[0][name][0] is None else np.stack([c[name][0] for c in cots])
    gl = None if cots[0][name][1] is None else np.stack([c[name][1] for c in cots])
    return gx, gl


def host_steps(case: Case, m: int, ps, z0, eps):
    """The steps the float64 oracle's own adaptive solve of member m's SAMPLING problem accepts (what the CPU test measures the
    floor on; the device tests replay the device's), and its statistics."""
    cfg = member_cfg(case, m)
    f64 = lambda a: np.asarray(a, np.float64)
    D = cfg.D(case.train)
    u0 = np.vstack([f64(z0[m]), np.zeros((D - cfg.n_in, case.B))])
    f = cfg.rhs(f64(ps[m]), f64(eps[m]) if case.train else None, case.train)
    _, st = O.tsit5_solve(f, u0, cfg.tspan[1], cfg.tspan[0], **dict(case.sol_kw))
    return st.dts, st


def reference(case: Case, m: int, ps, z0, eps, cot, dts):
    """``((z64 (n_in, B), logq64 (B,)), (grad64, gz0_64), (grad32, gz0_32))`` of member m for ``cot = (cot_z, cot_logq)`` through
    the steps ``dts`` (absolute sizes or signed ones)."""
    cfg = member_cfg(case, m)
    e = eps[m] if case.train else None
    z, q, g64, z64, _ = GR.vjp64(cfg, ps[m], z0[m], e, cot[0], cot[1], dts, train=case.train)
    _, _, g32, z32, _ = GR.vjp32(cfg, ps[m], z0[m], e, cot[0], cot[1], dts, train=case.train)
    return (z, q), (g64, z64), (g32, z32)


def floors(case: Case, m: int, ps, z0, eps, cot, dts):
    """(name, floor, rtol) per parameter block and for grad_z0: ``vjp_ref.report`` of the float64 reference against itself."""
    _, r64, r32 = reference(case, m, ps, z0, eps, cot, dts)
    return [(n, f, r) for n, _, f, r, _, _ in V.report(r64[0], r64[1], r64, r32, case.cfg.net)]
