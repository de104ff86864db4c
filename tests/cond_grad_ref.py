"""Float64 / float32 reference of the gradient of ``inference`` w.r.t. the conditioning inputs ``ys`` of a conditional model,
for an arbitrary cotangent of the four outputs (helper module; no GPU needed).

``tests/vjp_ref.vjp`` with one more result.  The first layer of a conditional model reads ``[z; ys]``
(src/layers/cond_layer.jl:7-9), so every stage pullback already forms the cotangent of that whole input,
``hbar_0 = W_1' abar_1``: its first n_in rows are zbar (what the oracle's ``rhs_vjp`` / ``rhs_vjp_test`` return), the
remaining n_cond rows are this stage's share of d / d ys.  ``ys`` is constant over the solve, so

    gy = sum over steps, sum over stages  hbar_0[n_in:]          (n_cond x B)

The two pullbacks are restated here from oracle/cnf_grad_oracle.py so that they return the whole ``hbar_0``; nothing under
oracle/ is changed.  tests/test_cond_grad_host.py pins the restatement: gradient and grad_x identical to ``vjp_ref``'s,
central differences in float64 w.r.t. single entries of ``ys``, and the independence of the samples.
"""
from __future__ import annotations

import numpy as np

from oracle import cnf_grad_oracle as G
from oracle import cnf_oracle as O
from tests import vjp_ref as V
from tests.vjp_ref import RTOL, FLOOR_FACTOR, RTOL_CAP, scale  # noqa: F401  (the bar, taken over unchanged)


def rhs_vjp_full(net, flat, z, eps, cot, norm_z, norm_j, use_jvp=False, ys=None):
    """``G.rhs_vjp`` returning (hbar_0 [(n_in + n_cond) x B], grad): the cotangent of the whole first-layer input."""
    n_in = z.shape[0]
    Ws, bs = O.unflatten_params(net, flat)
    x0 = z if ys is None else np.vstack([z, ys])
    hs, as_ = [x0], []
    h = x0
    for W, b in zip(Ws, bs):
        a = W @ h + b[:, None]
        as_.append(a)
        h = O.act_apply(net.acts[len(as_) - 1], a)[0]
        hs.append(h)
    d1 = [O.act_apply(k, a)[1] for k, a in zip(net.acts, as_)]
    d2 = [G.act_d2(k, a) for k, a in zip(net.acts, as_)]
    zdot = hs[-1]
    a_z, c_l, c_E, c_n = cot[:n_in], cot[n_in:n_in + 1], cot[n_in + 1:n_in + 2], cot[n_in + 2:n_in + 3]
    ahat = a_z + (c_E * G._unit(zdot) if norm_z else 0)
    if use_jvp:
        _, Je = O.mlp_jvp(net, flat, z, eps, ys)
        omega = -c_l * eps + (c_n * G._unit(Je) if norm_j else 0)
        tau = eps
    else:
        _, eJ = O.mlp_vjp(net, flat, z, eps, ys)
        omega = eps
        tau = -c_l * eps + (c_n * G._unit(eJ) if norm_j else 0)
    t = tau if ys is None else np.vstack([tau, np.zeros_like(ys)])
    ts, ps = [t], []
    for W, d in zip(Ws, d1):
        p = W @ t
        ps.append(p)
        t = d * p
        ts.append(t)
    hbar, tbar = ahat, omega
    gWs, gbs = [None] * len(Ws), [None] * len(Ws)
    for l in reversed(range(len(Ws))):
        abar = hbar * d1[l] + tbar * d2[l] * ps[l]
        pbar = tbar * d1[l]
        gWs[l] = abar @ hs[l].T + pbar @ ts[l].T
        gbs[l] = abar.sum(axis=1)
        hbar = Ws[l].T @ abar
        tbar = Ws[l].T @ pbar
    return hbar, G.flatten_grads(net, gWs, gbs)


def rhs_vjp_test_full(net, flat, z, kbar_z, c, ys=None):
    """``G.rhs_vjp_test`` returning (hbar_0 [(n_in + n_cond) x B], grad)."""
    n_in, B = z.shape
    Ws, bs = O.unflatten_params(net, flat)
    L = len(Ws)
    x0 = z if ys is None else np.vstack([z, ys])
    hs, d1, d2 = [x0], [], []
    h = x0
    for l, (W, b) in enumerate(zip(Ws, bs)):
        a = W @ h + b[:, None]
        h, d = O.act_apply(net.acts[l], a)
        hs.append(h); d1.append(d); d2.append(G.act_d2(net.acts[l], a))
    Ms = [d1[l].T[:, :, None] * Ws[l][None, :, :] for l in range(L)]
    P = [None] * L
    P[0] = np.broadcast_to(np.eye(x0.shape[0], n_in, dtype=z.dtype), (B, x0.shape[0], n_in))
    for l in range(1, L):
        P[l] = Ms[l - 1] @ P[l - 1]
    Q = [None] * L
    Q[L - 1] = np.broadcast_to(np.eye(n_in, dtype=z.dtype), (B, n_in, n_in))
    for l in range(L - 2, -1, -1):
        Q[l] = Q[l + 1] @ Ms[l + 1]
    cc = np.broadcast_to(np.asarray(c, dtype=z.dtype).reshape(1, -1), (1, B))[0]
    hbar = kbar_z
    gWs, gbs = [None] * L, [None] * L
    for l in reversed(range(L)):
        Gm = np.transpose(P[l] @ Q[l], (0, 2, 1))
        u = np.einsum("jk,bjk->jb", Ws[l], Gm)
        abar = hbar * d1[l] + cc[None, :] * (-1.0) * d2[l] * u
        gWs[l] = abar @ hs[l].T - np.einsum("b,jb,bjk->jk", cc, d1[l], Gm)
        gbs[l] = abar.sum(axis=1)
        hbar = Ws[l].T @ abar
    return hbar, G.flatten_grads(net, gWs, gbs)


def vjp_ys(cfg, flat, xs, eps, cot, dts, ys, train=True):
    """(out, grad, grad_x, grad_ys): the first three as ``vjp_ref.vjp`` gives them, grad_ys = sum_b sum_r cot[r][b]
    d out_r[b] / d ys (n_cond x B; column b depends on sample b alone), through the fixed steps ``dts``, in the dtype of
    ``flat``.  ``cot``: 4 x B, rows (logpx, E, n, A)."""
    if ys is None:
        raise ValueError("the gradient w.r.t. ys needs a conditional model")
    flat = np.asarray(flat)
    dts = [abs(float(d)) for d in dts]
    out, us, f = V.outputs(cfg, flat, xs, eps, dts, ys, train)
    fsol = us[-1]
    T = fsol.dtype.type
    cot = np.asarray(cot).astype(fsol.dtype)
    n_in = cfg.n_in
    z = fsol[:n_in]
    lam = np.zeros_like(fsol)
    lam[:n_in] = -cot[0] * z
    lam[n_in] = -cot[0]
    if train:
        if cfg.lam3 != 0 and cfg.naugs > 0:
            lam[cfg.nvars:n_in] += cot[3] * G._unit(z[cfg.nvars:])
        lam[n_in + 1] = cot[1]
        lam[n_in + 2] = cot[2]
    grad = np.zeros(flat.size, dtype=flat.dtype)
    gy = np.zeros_like(np.asarray(ys), dtype=fsol.dtype)
    A, Bc = O.TSIT5_A, O.TSIT5_B
    nz, nj = cfg.lam1 != 0, cfg.lam2 != 0
    tdir = 1.0 if cfg.tspan[1] >= cfg.tspan[0] else -1.0
    wl = lam[n_in][None, :]
    lz = lam[:n_in].copy()
    for n in reversed(range(len(dts))):
        h = T(tdir * dts[n])
        Us = V._stages(f, us[n], h, T)
        ws = [None] * 6
        for i in reversed(range(6)):
            if train:
                kbar = T(Bc[i]) * lam
                for m in range(i + 1, 6):
                    kbar[:n_in] += T(A[m][i]) * ws[m]
                hbar, g = rhs_vjp_full(cfg.net, flat, Us[i][:n_in], eps, h * kbar, nz, nj, cfg.use_jvp, ys)
            else:
                kb = T(Bc[i]) * lz
                for m in range(i + 1, 6):
                    kb = kb + T(A[m][i]) * ws[m]
                hbar, g = rhs_vjp_test_full(cfg.net, flat, Us[i][:n_in], h * kb, h * T(Bc[i]) * wl, ys)
            ws[i] = hbar[:n_in]
            gy += hbar[n_in:]
            grad += g
        if train:
            lam = lam.copy()
            for i in range(6):
                lam[:n_in] += ws[i]
        else:
            lz = lz + sum(ws)
    gx = (lam if train else lz)[:cfg.nvars].copy()
    return out, grad, gx, gy


def vjp_ys64(cfg, flat, xs, eps, cot, dts, ys, train=True):
    c = lambda a: V._cast(a, np.float64)
    return vjp_ys(cfg, c(flat), c(xs), c(eps), c(cot), dts, c(ys), train)


def vjp_ys32(cfg, flat, xs, eps, cot, dts, ys, train=True):
    c = lambda a: V._cast(a, np.float32)
    return vjp_ys(cfg, c(flat), c(xs), c(eps), c(cot), dts, c(ys), train)


def report_ys(got, ref64, ref32):
    """(err / scale, float32 floor, rtol, scale, ok) on the one block grad_ys, at the bar of ``vjp_ref.report``:
    max|got - ref64| <= rtol (max|ref64| + rms ref64), rtol = max(1e-4, 8 floor) <= 1e-3, floor = the float32 run of this
    reference against its float64 run (never a device number)."""
    r64 = np.asarray(ref64, np.float64)
    s = scale(r64)
    floor = float(np.abs(np.asarray(ref32, np.float64) - r64).max()) / s if s > 0 else np.inf
    got = np.asarray(got, np.float64)
    assert got.shape == r64.shape, (got.shape, r64.shape)
    err = float(np.abs(got - r64).max()) / s if s > 0 else np.inf
    rtol = max(RTOL, FLOOR_FACTOR * floor)
    return err, floor, rtol, s, bool(np.isfinite(err) and err <= rtol and rtol <= RTOL_CAP)


def assert_ys(got, ref64, ref32, what):
    err, floor, rtol, s, ok = report_ys(got, ref64, ref32)
    print(f"grad_ys | {what} | err/scale {err:.2e} floor {floor:.2e} rtol {rtol:.1e} scale {s:.2e}")
    assert s > 0, f"{what}: the reference grad_ys is zero (nothing to compare against)"
    assert rtol <= RTOL_CAP, f"{what}: the float32 reference's own error {floor:.3g} asks for rtol {rtol:.3g} > the cap {RTOL_CAP:g}"
    assert ok, f"{what}: grad_ys off by {err:.3g} of its scale {s:.3g} (rtol {rtol:.3g}, float32 floor {floor:.3g})"
    return err, floor, rtol, s


# the conditional cases of tests/grad_terms.py, by name, and the fixed steps they take
COND_CASES = ("wave-6x18-B40-cond", "adj3-28x128x128-cond", "mfma-12x64x48-cond-vjp", "mfma-12x64x48-cond-jvp")


def case_dts(case):
    assert case.steps[0] == "fixed", case.name
    return [case.steps[1]] * int(round(abs(case.tspan[1] - case.tspan[0]) / case.steps[1]))


_MEMO = {}


def case_reference(case, cot, train=True, lam=(0.01, 0.02, 0.03), tag=""):
    """(cfg, ref64, ref32) of ``vjp_ys`` on a case of tests/grad_terms.py, memoised per (case, mode, tag): each a tuple
    (out, grad, grad_x, grad_ys).  ``tag`` names the cotangent."""
    key = (case.name, train, tuple(lam), tag)
    if key not in _MEMO:
        cfg = case.cfg(lam)
        flat, xs, eps, ys = case.inputs()
        dts = case_dts(case)
        e = eps if train else None
        _MEMO[key] = (cfg, vjp_ys64(cfg, flat, xs, e, cot, dts, ys, train), vjp_ys32(cfg, flat, xs, e, cot, dts, ys, train))
    return _MEMO[key]
