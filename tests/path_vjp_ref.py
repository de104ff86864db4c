"""Reference of differentiable flow paths (``inference_path_vjp`` / ``generate_path_vjp``; helper module, no GPU needed): the
discrete adjoint of the accepted steps with the cotangents of the path's slices injected at the save times, in numpy, in the
dtype it is given.

Built from the pieces the other references are built from -- ``G.rhs_vjp`` / ``G.rhs_vjp_test`` (per-column cotangents),
``vjp_ref._stages``, ``path_ref.dense_b`` / ``path_ref.tsit5_step_all``, the Tsit5 tables -- and the bracketing rule of
include/cnfhip_path.h as ``path_ref.replay`` states it.  The step sequence ``(t_n, h_n)`` is frozen, hence ``theta`` is a constant.
With ``pbar_j`` the cotangent of slice j (all D rows):

    tau_j == t_start           the slice is u0:        pbar_j joins d / d u(t_start) at the very end
    the end of its step        the slice is u_{n+1}:   lambda += pbar_j before step n is pulled back
    interior                   u_n + h sum_i b_i(theta_j) k_i:  s_i = sum_j b_i(theta_j) pbar_j, e = sum_j pbar_j;
                               k_7 = f(u_{n+1}) first: w_7, g = rhs_vjp(u_{n+1}; h s_7), lambda_z += w_7; then the stages
                               i = 6..1 with kbar_i = h (b_i lambda + s_i + sum_{m > i} a_{m,i} w_m); lambda_z += sum w_i;
                               lambda += e

(no FSAL fold here: k_7 is pulled back where it is used).  tests/test_path_vjp_ref_host.py pins it by central differences.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import cnf_grad_oracle as G
from oracle import cnf_oracle as O
from tests import ensemble_vjp_ref as E
from tests import path_ref as P
from tests import vjp_ref as V

START, END, INTERIOR = "start", "end", "interior"


def brackets(tspan, steps_t, steps_h, saveat):
    """Which step serves which save time, and how: a list of ``(kind, n, theta)`` per save time -- the rule of
    ``path_ref.replay``, decided in float32 as the device decides it (``theta`` itself is returned in float64 from the float32
    times)."""
    t0, t1 = np.float32(tspan[0]), np.float32(tspan[1])
    sv = np.asarray(saveat, dtype=np.float32)
    d = np.float32(1.0 if t1 >= t0 else -1.0)
    out, cur = [], 0
    while cur < sv.size and sv[cur] == t0:
        out.append((START, -1, 0.0))
        cur += 1
    N = len(steps_t)
    for n in range(N):
        tn, hn = np.float32(steps_t[n]), np.float32(steps_h[n])
        last = n == N - 1
        t_end = t1 if last else np.float32(steps_t[n + 1])
        while cur < sv.size:
            tau = sv[cur]
            if not last and d * (tau - t_end) > 0:
                break
            th32 = (tau - tn) / hn
            theta = (float(tau) - float(tn)) / float(hn)
            out.append((END, n, 1.0) if (tau == t_end or not th32 < 1) else (INTERIOR, n, theta))
            cur += 1
    assert cur == sv.size, "save times left unserved"
    return out


def adjoint(cfg, flat, u0, eps, tspan, steps_t, steps_h, saveat, lam_end_of, path_cot, train):
    """The core, on the augmented state.  ``u0`` D x B; ``(steps_t, steps_h)`` the accepted steps (signed sizes); ``lam_end_of``:
    final state -> its cotangent (D x B); ``path_cot`` K x D x B or None.  Returns ``(path K x D x B, u_final, grad, lam0 D x B)``
    in the dtype of ``u0``."""
    u0 = np.asarray(u0)
    T = u0.dtype.type
    flat = np.asarray(flat).astype(u0.dtype)
    eps = None if eps is None else np.asarray(eps).astype(u0.dtype)
    n_in = cfg.n_in
    f = cfg.rhs(flat, eps if train else None, train)
    br = brackets(tspan, steps_t, steps_h, saveat)
    K, N = len(br), len(steps_t)
    path = np.zeros((K,) + u0.shape, dtype=u0.dtype)
    pc = np.zeros_like(path) if path_cot is None else np.asarray(path_cot).astype(u0.dtype)
    us, kss = [u0.copy()], []
    u, k1 = u0, f(u0)
    for n in range(N):
        u, ks = P.tsit5_step_all(f, u, k1, T(steps_h[n]))
        k1 = ks[6]
        us.append(u)
        kss.append(ks)
    for j, (kind, n, theta) in enumerate(br):
        path[j] = u0 if kind == START else us[n + 1] if kind == END else P.interpolate(us[n], kss[n], np.float32(steps_h[n]), theta)
    A, Bc = O.TSIT5_A, O.TSIT5_B
    nz, nj = cfg.lam1 != 0, cfg.lam2 != 0
    lam = np.asarray(lam_end_of(us[-1])).astype(u0.dtype).copy()
    grad = np.zeros(flat.size, dtype=u0.dtype)

    def pull(z, h, kbar, c_l=None):
        """rhs_vjp at z for the cotangent h kbar (D x B) of the stage's k: (w n_in x B, grad).  TestMode: ``c_l`` is the dlogp
        row's part, already multiplied by h (in the order tests/vjp_ref.py multiplies it: the two agree bit for bit without a
        path cotangent)."""
        if train:
            return G.rhs_vjp(cfg.net, flat, z, eps, h * kbar, nz, nj, cfg.use_jvp)
        return G.rhs_vjp_test(cfg.net, flat, z, h * kbar[:n_in], c_l)

    for n in reversed(range(N)):
        h = T(steps_h[n])
        mine = [(j, kind, theta) for j, (kind, nn, theta) in enumerate(br) if nn == n]
        for j, kind, _ in mine:
            if kind == END:
                lam = lam + pc[j]
        inner = [(j, P.dense_b(theta, u0.dtype)) for j, kind, theta in mine if kind == INTERIOR]
        seeds = [sum((b[i] * pc[j] for j, b in inner), np.zeros_like(lam)) for i in range(7)]
        if inner:
            w7, g = pull(us[n + 1][:n_in], h, seeds[6], h * seeds[6][n_in][None, :])
            lam = lam.copy()
            lam[:n_in] += w7
            grad += g
        Us = V._stages(f, us[n], h, T)
        ws = [None] * 6
        for i in reversed(range(6)):
            kbar = T(Bc[i]) * lam + seeds[i]
            for m in range(i + 1, 6):
                kbar[:n_in] += T(A[m][i]) * ws[m]
            ws[i], g = pull(Us[i][:n_in], h, kbar, h * T(Bc[i]) * lam[n_in][None, :] + h * seeds[i][n_in][None, :])
            grad += g
        lam = lam.copy()
        if train:
            for i in range(6):
                lam[:n_in] += ws[i]
        else:                                              # (the order tests/vjp_ref.py adds them in)
            lam[:n_in] = lam[:n_in] + sum(ws)
        for j, _ in inner:
            lam = lam + pc[j]
    for j, (kind, _, _) in enumerate(br):
        if kind == START:
            lam = lam + pc[j]
    return path, us[-1], grad, lam


def _pack(cfg, train, B, K, rows, dtype):
    """A dict of row cotangents (``z`` K x n_in x B, scalars K x B by state row index) -> K x D x B, or None."""
    if not rows:
        return None
    pc = np.zeros((K, cfg.D(train), B), dtype=dtype)
    for key, v in rows.items():
        if v is None:
            continue
        if key == "z":
            pc[:, :cfg.n_in] = v
        else:
            pc[:, key] = v
    return pc


def inference(cfg, flat, xs, eps, cot, path_cot, steps_t, steps_h, saveat, train=True, dtype=np.float64):
    """``(out 4 x B, path K x D x B, grad, grad_x nvars x B)``: ``cot`` 4 x B (rows logpx, E, n, A) or None; ``path_cot`` a dict
    with any of ``z``, ``dlogp``, ``E``, ``n``."""
    c = lambda a: None if a is None else np.asarray(a).astype(dtype)
    xs = c(xs)
    B, K = xs.shape[1], len(saveat)
    n_in = cfg.n_in
    cot = np.zeros((4, B), dtype) if cot is None else c(cot)
    names = {"z": "z", "dlogp": n_in, "E": n_in + 1, "n": n_in + 2}
    pc = _pack(cfg, train, B, K, {names[k]: c(v) for k, v in (path_cot or {}).items()}, dtype)
    u0 = O.inference_u0(cfg, xs, train)

    def lam_end(fsol):
        z = fsol[:n_in]
        lam = np.zeros_like(fsol)
        lam[:n_in] = -cot[0] * z
        lam[n_in] = -cot[0]
        if train:
            if cfg.lam3 != 0 and cfg.naugs > 0:
                lam[cfg.nvars:n_in] += cot[3] * G._unit(z[cfg.nvars:])
            lam[n_in + 1] = cot[1]
            lam[n_in + 2] = cot[2]
        return lam

    path, fsol, grad, lam0 = adjoint(cfg, c(flat), u0, c(eps), cfg.tspan, steps_t, steps_h, saveat, lam_end, pc, train)
    logpx, (En, nn, An) = O.inference_sol(cfg, fsol, train)
    zero = np.zeros_like(logpx)
    out = np.stack([logpx] + [np.broadcast_to(np.asarray(r, dtype=logpx.dtype), logpx.shape) if train else zero for r in (En, nn, An)])
    return out, path, grad, lam0[:cfg.nvars].copy()


def generate(cfg, flat, z0, eps, cot_z, cot_logq, path_cot, steps_t, steps_h, saveat, train=True, dtype=np.float64):
    """``(z n_in x B, logq B, path K x D x B, logq_path K x B, grad, grad_z0 n_in x B)`` over reverse(cfg.tspan); ``path_cot`` a dict
    with any of ``z``, ``logq`` (the cotangent of ``logq_path = logpdf(N(0, I), z0) + dlogp(tau_k)``)."""
    c = lambda a: None if a is None else np.asarray(a).astype(dtype)
    z0 = c(z0)
    n_in, B, K = cfg.n_in, z0.shape[1], len(saveat)
    cz = np.zeros((n_in, B), dtype)
    if cot_z is not None:
        cz[:np.asarray(cot_z).shape[0]] = c(cot_z)
    cl = np.zeros(B, dtype) if cot_logq is None else c(cot_logq).reshape(B)
    pcd = path_cot or {}
    pc = _pack(cfg, train, B, K, {"z": c(pcd.get("z")), n_in: c(pcd.get("logq"))} if pcd else {}, dtype)
    u0 = np.vstack([z0, np.zeros((cfg.D(train) - n_in, B), dtype=dtype)])

    def lam_end(fsol):
        lam = np.zeros_like(fsol)
        lam[:n_in] = cz
        lam[n_in] = cl
        return lam

    span = (cfg.tspan[1], cfg.tspan[0])
    path, fsol, grad, lam0 = adjoint(cfg, c(flat), u0, c(eps), span, steps_t, steps_h, saveat, lam_end, pc, train)
    lp0 = -0.5 * (n_in * np.log(2.0 * np.pi) + np.sum(z0 * z0, axis=0))
    tail = cl + (c(pcd["logq"]).sum(axis=0) if pcd.get("logq") is not None else 0.0)
    gz0 = lam0[:n_in] - tail[None, :] * z0
    return fsol[:n_in].copy(), (lp0 + fsol[n_in]).astype(dtype), path, (lp0[None, :] + path[:, n_in]).astype(dtype), grad, gz0


# ---------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    cfg: O.Cfg
    B: int
    train: bool = True
    jvp: bool = False
    sol_kw: dict = field(default_factory=dict)
    wscale: float = 1.0
    seed: int = 0
    fixed_saveat: tuple | None = None       # save times given as times (the fixed-step case), not as fractions of steps


def _from(e: E.Case) -> Case:
    """Member 0 of a case of tests/ensemble_vjp_ref.py (its own end time where the members have one)."""
    return Case("path-" + e.name, E.member_cfg(e, 0), e.B, e.train, e.jvp, dict(e.sol_kw), e.wscale[0], e.seed)


_BY = {c.name: c for c in E.CASES}
CASES = [_from(_BY[n]) for n in ("readme-vjp-B33", "regr-vjp-B17-rejects", "regr-jvp-B33", "regr-test-B17", "noaug-vjp-B1",
                                 "id2-vjp-B17", "readme-test-B1")]
# fixed steps of 0.25 over (0, 1): the save time 0.5 is exactly the end of the second step
CASES.append(Case("path-fixed-B17", O.Cfg(O.Net((2, 6, 2), E.TANH2), 1, 1, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)), 17, seed=31,
                  sol_kw=dict(adaptive=False, dt=0.25), fixed_saveat=(0.0, 0.1, 0.3, 0.35, 0.5, 0.5, 0.9, 1.0)))
IDS = [c.name for c in CASES]


def inputs(case: Case):
    """``(flat, xs (nvars, B), z0 (n_in, B), eps (n_in, B))`` float32."""
    cfg = case.cfg
    rng = np.random.default_rng(9700 + case.seed)
    flat = np.float32(case.wscale) * O.glorot_params(cfg.net, rng, np.float32, 0.5)
    xs = rng.standard_normal((cfg.nvars, case.B)).astype(np.float32)
    z0 = rng.standard_normal((cfg.n_in, case.B)).astype(np.float32)
    eps = rng.standard_normal((cfg.n_in, case.B)).astype(np.float32)
    return flat, xs, z0, eps


def save_times(case: Case, steps_t, steps_h, tspan, which="mixed"):
    """The save-time sets, as fractions of the steps a first call reported, turned into float32 times.  ``mixed``: t_start, the
    middle of the first step, two in one interior step, a duplicate time, the middle of the last step, t_end;  ``k40``: 40 times
    spread over the span (more saves than steps);  ``end``: t_end alone."""
    t_start, t_end = np.float32(tspan[0]), np.float32(tspan[1])
    if which == "end":
        return np.array([t_end], np.float32)
    if which == "k40":
        return (t_start + (t_end - t_start) * np.linspace(0.0, 1.0, 40, dtype=np.float64)).astype(np.float32)
    if case.fixed_saveat is not None:
        sv = np.asarray(case.fixed_saveat, np.float32)
        return sv if t_end >= t_start else (t_start + t_end - sv).astype(np.float32)      # (mirrored: it runs along the span)
    ts, hs = np.asarray(steps_t, np.float64), np.asarray(steps_h, np.float64)
    N = len(ts)
    at = lambda n, fr: np.float32(ts[n] + fr * hs[n])
    mid = N // 2
    sv = [t_start, at(0, 0.5), at(mid, 0.3), at(mid, 0.7), at(mid, 0.7), at(N - 1, 0.5), t_end]
    d = 1.0 if t_end >= t_start else -1.0
    sv = np.asarray(sv, np.float32)
    assert np.all(d * np.diff(sv) >= 0), "the steps of this case are too few to place the save times in order"
    return sv


def path_cotangents(case: Case, K, sampling, which):
    """The cotangent sets of the device tests: ``terminal`` (none on the path), each path row alone, ``all`` together.  Returns
    ``(cot, path_cot)``: inference ``cot`` 4 x B and a dict of ``z, dlogp[, E, n]``; sampling ``cot = (cot_z, cot_logq)`` and a dict
    of ``z, logq``.  Entries N(0, 1) / B."""
    cfg, B = case.cfg, case.B
    rng = np.random.default_rng(7700 + 10 * case.seed + (1 if sampling else 0))
    d = lambda *s: (rng.standard_normal(s) / B).astype(np.float32)
    rows = E.rows(E.Case(case.name, cfg, B, case.train, case.jvp))
    term = np.zeros((4, B), np.float32)
    for r in rows:
        term[r] = d(B)
    term_s = (d(cfg.n_in, B), d(B))
    full = {"z": d(K, cfg.n_in, B), ("logq" if sampling else "dlogp"): d(K, B)}
    if not sampling and case.train:
        if cfg.lam1 != 0:
            full["E"] = d(K, B)
        if cfg.lam2 != 0:
            full["n"] = d(K, B)
    terminal = term_s if sampling else term
    if which == "terminal":
        return terminal, None
    if which == "all":
        return terminal, full
    if which == "path-only":
        return None, full
    return None, {which: full[which]}


def cot_sets(case: Case, sampling):
    names = ["terminal", "z", "logq" if sampling else "dlogp"]
    if not sampling and case.train:
        names += [k for k, on in (("E", case.cfg.lam1 != 0), ("n", case.cfg.lam2 != 0)) if on]
    return names + ["all"]


def host_steps(case: Case, flat, xs, z0, eps, sampling, dtype=np.float64):
    """The accepted steps ``(t_n, signed h_n)`` and statistics of the oracle's own solve of the case in ``dtype`` (what the CPU
    tests replay; the device tests replay the device's)."""
    cfg = case.cfg
    c = lambda a: np.asarray(a).astype(dtype)
    D = cfg.D(case.train)
    u0 = np.vstack([c(z0), np.zeros((D - cfg.n_in, case.B), dtype)]) if sampling else O.inference_u0(cfg, c(xs), case.train)
    f = cfg.rhs(c(flat), c(eps) if case.train else None, case.train)
    a, b = (cfg.tspan[1], cfg.tspan[0]) if sampling else cfg.tspan
    _, st = O.tsit5_solve(f, u0, a, b, **dict(case.sol_kw))
    d = 1.0 if b >= a else -1.0
    hs = np.asarray([d * h for h in st.dts], np.float32)
    ts = np.float32(a) + np.concatenate([[0.0], np.cumsum(hs[:-1].astype(np.float64))]).astype(np.float32)
    return ts.astype(np.float32), hs, st
