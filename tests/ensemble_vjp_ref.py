"""Cases and references of the differentiable ensemble (``inference_vjp_many``; helper module, no GPU needed).

The case list -- networks, modes, spans, per-member end times, step settings --, the members' inputs and cotangents, and the
float64 / float32 references of one member: tests/vjp_ref.py (``vjp64``, ``vjp32``, ``row_cotangents``, ``loss_cotangent``,
``assert_vjp``) applied member by member, nothing restated.  tests/test_ensemble_vjp_host.py checks on the CPU that the float32
floor of every case leaves the bar where the device tests need it; tests/test_gpu_ensemble_vjp.py takes its inputs from here
and replays the steps each member accepted on the device.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import cnf_oracle as O
from tests import vjp_ref as V

TANH2 = (O.ACT_TANH,) * 2
M = 3


@dataclass
class Case:
    name: str
    cfg: O.Cfg                     # (its tspan is the case's; a member with its own end time gets a copy: member_cfg)
    B: int
    train: bool = True
    jvp: bool = False
    sol_kw: dict = field(default_factory=dict)       # adaptive steps everywhere (the controller's own settings where given)
    t1: tuple | None = None        # per-member end times
    scales: tuple = (0.5, 0.5, 0.5)                  # bias scale of each member's Glorot draw
    wscale: tuple = (1.0, 1.0, 1.0)                  # ... and a factor on its whole parameter vector (a stiff member)
    shared_xs: bool = False        # one data set (nvars, B) scored by every member
    seed: int = 0


# The networks of tests/test_gpu_ensemble.py: 2-6-2 and 16-48-16 (one hidden tile and three), 7-13-7 without augmentation, the
# tanh / identity pair.  B in {1, 17, 33}: one live column in the last tile, and three tiles that must meet.
CASES = [
    Case("readme-vjp-B33", O.Cfg(O.Net((2, 6, 2), TANH2), 1, 1, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)), 33, seed=11, t1=(0.6, 1.0, 1.7)),
    # member 0 is stiff for a first step of half the span: it rejects attempts (the device test asserts that it does)
    Case("regr-vjp-B17-rejects", O.Cfg(O.Net((16, 48, 16), TANH2), 8, 8, 1e-2, 1e-2, 1e-2, tspan=(0.0, 2.0)), 17, seed=12,
         sol_kw=dict(dt=1.0, reltol=1e-4, abstol=1e-6), wscale=(2.0, 1.0, 1.0)),
    Case("regr-jvp-B33", O.Cfg(O.Net((16, 48, 16), TANH2), 8, 8, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)), 33, jvp=True, seed=13),
    Case("regr-test-B17", O.Cfg(O.Net((16, 48, 16), TANH2), 8, 8, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)), 17, train=False, seed=14,
         shared_xs=True),
    Case("noaug-vjp-B1", O.Cfg(O.Net((7, 13, 7), TANH2), 7, 0, 1e-2, 1e-2, 0.0, tspan=(1.0, 0.0)), 1, seed=15),
    Case("id2-vjp-B17", O.Cfg(O.Net((6, 9, 6), (O.ACT_TANH, O.ACT_IDENTITY)), 6, 0, 1e-2, 1e-2, 0.0, tspan=(0.0, 1.0)), 17, seed=16),
    Case("readme-test-B1", O.Cfg(O.Net((2, 6, 2), TANH2), 1, 1, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)), 1, train=False, seed=17),
]
IDS = [c.name for c in CASES]


def member_cfg(case: Case, m: int) -> O.Cfg:
    c = case.cfg
    t1 = c.tspan[1] if case.t1 is None else float(case.t1[m])
    return O.Cfg(c.net, c.nvars, c.naugs, c.lam1, c.lam2, c.lam3, use_jvp=case.jvp, tspan=(c.tspan[0], t1))


def inputs(case: Case):
    """``(ps (M, n_params), xs (M, nvars, B), eps (M, n_in, B))`` float32; with ``shared_xs`` every member's xs is the same."""
    cfg = case.cfg
    rng = np.random.default_rng(9000 + case.seed)
    ps = np.stack([np.float32(w) * O.glorot_params(cfg.net, rng, np.float32, s) for s, w in zip(case.scales, case.wscale)])
    xs = rng.standard_normal((M, cfg.nvars, case.B)).astype(np.float32)
    if case.shared_xs:
        xs[:] = xs[0]
    eps = rng.standard_normal((M, cfg.n_in, case.B)).astype(np.float32)
    return ps, xs, eps


def rows(case: Case):
    """The output rows the case's model integrates (the others ignore their cotangent)."""
    c = case.cfg
    if not case.train:
        return (0,)
    return (0,) + tuple(r for r, on in ((1, c.lam1 != 0), (2, c.lam2 != 0), (3, c.lam3 != 0 and c.naugs > 0)) if on)


def cotangents(case: Case, m: int):
    """Member m's cotangents: ``vjp_ref.row_cotangents`` -- each row alone, then all together.  name -> 4 x B float32."""
    return V.row_cotangents(np.random.default_rng(7000 + 10 * case.seed + m), case.B, rows(case))


def host_steps(case: Case, m: int, ps, xs, eps):
    """The steps the float64 oracle's own adaptive solve accepts for member m (what the CPU test measures the floor on; the
    device tests replay the device's)."""
    f64 = lambda a: np.asarray(a, np.float64)
    kw = dict(case.sol_kw)
    _, _, _, st = O.inference(member_cfg(case, m), f64(ps[m]), f64(xs[m]), f64(eps[m]) if case.train else None, case.train, **kw)
    return st.dts, st


def reference(case: Case, m: int, ps, xs, eps, cot, dts):
    """``(out64 (4, B), (grad64, gx64), (grad32, gx32))`` of member m for the cotangent ``cot`` (4, B) through ``dts``."""
    cfg = member_cfg(case, m)
    e = eps[m] if case.train else None
    out, g64, x64 = V.vjp64(cfg, ps[m], xs[m], e, cot, dts, train=case.train)
    _, g32, x32 = V.vjp32(cfg, ps[m], xs[m], e, cot, dts, train=case.train)
    return out, (g64, x64), (g32, x32)


def floors(case: Case, m: int, ps, xs, eps, cot, dts):
    """(name, floor, rtol) per parameter block and for grad_x: ``vjp_ref.report`` of the float64 reference against itself."""
    _, r64, r32 = reference(case, m, ps, xs, eps, cot, dts)
    return [(n, f, r) for n, _, f, r, _, _ in V.report(r64[0], r64[1], r64, r32, case.cfg.net)]
