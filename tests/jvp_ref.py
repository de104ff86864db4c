"""Reference of the forward-mode derivative (tangent) of ``inference`` and of sampling (helper module; no GPU needed).

ANALYTIC, in numpy, in the dtype it is handed: the product rule through every line of ``oracle.cnf_oracle`` that
``vjp_ref.outputs`` / ``gen_vjp_ref.forward`` run -- the MLP, its VJP / JVP / exact-trace sweep, the norms, Tsit5's stage sums
over the given step sizes ``dts`` (constants of the derivative: the discrete map through the accepted steps) and the
post-processing.  Along a direction ``(dflat, dx)``:

    da_l = W_l dh_{l-1} + dW_l h_{l-1} + db_l,   dh_l = s'(a_l) da_l,   ds'_l = s''(a_l) da_l
    VJP sweep   g <- W_l' (g s'_l):   dg <- W_l' (dg s'_l + g ds'_l) + dW_l' (g s'_l)
    JVP sweep   t <- s'_l (W_l t):    dt <- ds'_l (W_l t) + s'_l (dW_l t + W_l dt)
    trace       the JVP sweep on the n_in unit columns at once
    dldot = -eps . d(eps'J);   dE = zdot . dzdot / |zdot|;   dn = v . dv / |v| (v = eps'J or J eps);   0 where the norm is 0
    dlogpx = -z(t1) . dz(t1) - d dlogp;   dA = z_aug . dz_aug / |z_aug|;   sampling: dlogq = -z0 . dz0 + d dlogp

tests/test_jvp_ref_host.py pins it by central differences of ``vjp_ref.outputs`` and by the dot identity with ``vjp_ref.vjp64``
(and ``gen_vjp_ref.vjp64``).  Nothing under oracle/ is changed.
"""
from __future__ import annotations

import numpy as np

from oracle import cnf_oracle as O
from tests import gen_vjp_ref as GR
from tests import vjp_ref as V


def _act3(kind, a):
    """(s, s', s'') of the activations the tangent kernels take."""
    one = a.dtype.type(1)
    if kind == O.ACT_IDENTITY:
        return a, np.ones_like(a), np.zeros_like(a)
    if kind == O.ACT_TANH:
        h = np.tanh(a)
        d = one - h * h
        return h, d, a.dtype.type(-2) * h * d
    raise ValueError(f"no second derivative restated for activation {kind}")


def _unit_dot(v, dv):
    """d |v| per column = v . dv / |v|, 0 where |v| = 0."""
    n = np.sqrt(np.sum(v * v, axis=0))
    num = np.sum(v * dv, axis=0)
    return np.where(n > 0, num / np.where(n > 0, n, 1), 0).astype(v.dtype)


def rhs_tangent(cfg, flat, dflat, eps, train):
    """f(u, du) -> (f(u), df): ``cfg.rhs`` and its tangent along ``dflat`` (and the state tangent ``du``)."""
    net = cfg.net
    Ws, bs = O.unflatten_params(net, flat)
    dWs, dbs = O.unflatten_params(net, dflat)
    n_in = cfg.n_in

    def f(u, du):
        z, dz = u[:n_in], du[:n_in]
        hs, ds, dds, dhs, das = [z], [], [], [dz], []
        for W, b, dW, db, k in zip(Ws, bs, dWs, dbs, net.acts):
            a = W @ hs[-1] + b[:, None]
            da = W @ dhs[-1] + dW @ hs[-1] + db[:, None]
            h, d, dd = _act3(k, a)
            hs.append(h); ds.append(d); dds.append(dd); das.append(da); dhs.append(d * da)
        zdot, dzdot = hs[-1], dhs[-1]
        dsl = [dd * da for dd, da in zip(dds, das)]          # d s'_l
        if train:
            if cfg.use_jvp:
                t, dt = eps, np.zeros_like(eps)
                for W, dW, d, dd in zip(Ws, dWs, ds, dsl):
                    wt = W @ t
                    t, dt = d * wt, dd * wt + d * (dW @ t + W @ dt)
                v, dv = t, dt
            else:
                g, dg = eps, np.zeros_like(eps)
                for W, dW, d, dd in zip(reversed(Ws), reversed(dWs), reversed(ds), reversed(dsl)):
                    p = g * d
                    dp = dg * d + g * dd
                    g, dg = W.T @ p, W.T @ dp + dW.T @ p
                v, dv = g, dg
            ldot = -np.sum(v * eps, axis=0, keepdims=True)
            dldot = -np.sum(dv * eps, axis=0, keepdims=True)
            zero = np.zeros_like(ldot)
            E = O._colnorm(zdot)[None, :] if cfg.lam1 != 0 else zero
            dE = _unit_dot(zdot, dzdot)[None, :] if cfg.lam1 != 0 else zero
            n = O._colnorm(v)[None, :] if cfg.lam2 != 0 else zero
            dn = _unit_dot(v, dv)[None, :] if cfg.lam2 != 0 else zero
            return np.vstack([zdot, ldot, E, n]), np.vstack([dzdot, dldot, dE, dn])
        # exact trace: the JVP sweep on all unit columns, T[i, j, b] = d h_i / d z_j
        B = z.shape[1]
        T = np.broadcast_to(np.eye(n_in, dtype=z.dtype)[:, :, None], (n_in, n_in, B)).copy()
        dT = np.zeros_like(T)
        for W, dW, d, dd in zip(Ws, dWs, ds, dsl):
            wt = np.einsum("oi,ijb->ojb", W, T)
            dwt = np.einsum("oi,ijb->ojb", dW, T) + np.einsum("oi,ijb->ojb", W, dT)
            T, dT = d[:, None, :] * wt, dd[:, None, :] * wt + d[:, None, :] * dwt
        ldot = -np.trace(T, axis1=0, axis2=1)[None, :]
        dldot = -np.trace(dT, axis1=0, axis2=1)[None, :]
        return np.vstack([zdot, ldot]), np.vstack([dzdot, dldot])

    return f


def _replay(f, u0, du0, t0, t1, dts):
    """(u_N, du_N) through the steps ``dts`` (absolute sizes) of Tsit5, FSAL as ``G.forward_record`` takes them."""
    T = u0.dtype.type
    tdir = T(1) if t1 >= t0 else T(-1)
    A = O.TSIT5_A
    u, du = u0, du0
    k1, dk1 = f(u, du)
    for hh in dts:
        h = tdir * T(abs(float(hh)))
        ks, dks = [k1], [dk1]
        us = dus = None
        for s in range(1, 7):
            acc, dacc = T(A[s][0]) * ks[0], T(A[s][0]) * dks[0]
            for j in range(1, s):
                acc = acc + T(A[s][j]) * ks[j]
                dacc = dacc + T(A[s][j]) * dks[j]
            us, dus = u + h * acc, du + h * dacc
            k, dk = f(us, dus)
            ks.append(k); dks.append(dk)
        u, du, k1, dk1 = us, dus, ks[6], dks[6]
    return u, du


def _dflat(cfg, flat, dflat):
    return np.zeros_like(flat) if dflat is None else np.asarray(dflat).astype(flat.dtype)


def inference_jvp(cfg, flat, xs, eps, dflat, dxs, dts, train=True):
    """(out, dout): ``vjp_ref.outputs`` (4 x B, rows logpx, E, n, A) and its tangent along (dflat | None, dxs | None)."""
    flat = np.asarray(flat)
    xs = np.asarray(xs)
    dfl = _dflat(cfg, flat, dflat)
    dxs = np.zeros_like(xs) if dxs is None else np.asarray(dxs).astype(xs.dtype)
    u0 = O.inference_u0(cfg, xs, train)
    du0 = O.inference_u0(cfg, dxs, train)
    f = rhs_tangent(cfg, flat, dfl, eps, train)
    u, du = _replay(f, u0, du0, cfg.tspan[0], cfg.tspan[1], dts)
    n_in = cfg.n_in
    z, dz = u[:n_in], du[:n_in]
    logpx, (E, n, A) = O.inference_sol(cfg, u, train)
    zero = np.zeros_like(logpx)
    dlogpx = (-np.sum(z * dz, axis=0) - du[n_in]).astype(u.dtype)
    if train:
        dA = _unit_dot(z[cfg.nvars:], dz[cfg.nvars:]) if (cfg.lam3 != 0 and cfg.naugs > 0) else zero
        out = np.stack([logpx, E, n, np.broadcast_to(np.asarray(A, dtype=u.dtype), logpx.shape)])
        return out, np.stack([dlogpx, du[n_in + 1], du[n_in + 2], dA])
    return np.stack([logpx, zero, zero, zero]), np.stack([dlogpx, zero, zero, zero])


def generate_jvp(cfg, flat, z0, eps, dflat, dz0, dts, train=True):
    """((z, logq), (dz, dlogq)): ``gen_vjp_ref.forward`` and its tangent along (dflat | None, dz0 | None); z is n_in x B."""
    flat = np.asarray(flat)
    z0 = np.asarray(z0)
    dfl = _dflat(cfg, flat, dflat)
    dz0 = np.zeros_like(z0) if dz0 is None else np.asarray(dz0).astype(z0.dtype)
    D, n_in = cfg.D(train), cfg.n_in
    pad = np.zeros((D - n_in, z0.shape[1]), dtype=z0.dtype)
    f = rhs_tangent(cfg, flat, dfl, eps, train)
    t0, t1 = GR._span(cfg)
    u, du = _replay(f, np.vstack([z0, pad]), np.vstack([dz0, pad]), t0, t1, dts)
    logq = (GR.base_logpdf(z0) + u[n_in]).astype(u.dtype)
    dlogq = (-np.sum(z0 * dz0, axis=0) + du[n_in]).astype(u.dtype)
    return (u[:n_in].copy(), logq), (du[:n_in].copy(), dlogq)


def _c(a, dtype):
    return None if a is None else np.asarray(a).astype(dtype)


def inference_jvp64(cfg, flat, xs, eps, dflat, dxs, dts, train=True):
    c = lambda a: _c(a, np.float64)
    return inference_jvp(cfg, c(flat), c(xs), c(eps), c(dflat), c(dxs), dts, train)


def inference_jvp32(cfg, flat, xs, eps, dflat, dxs, dts, train=True):
    c = lambda a: _c(a, np.float32)
    return inference_jvp(cfg, c(flat), c(xs), c(eps), c(dflat), c(dxs), dts, train)


def generate_jvp64(cfg, flat, z0, eps, dflat, dz0, dts, train=True):
    c = lambda a: _c(a, np.float64)
    return generate_jvp(cfg, c(flat), c(z0), c(eps), c(dflat), c(dz0), dts, train)


def generate_jvp32(cfg, flat, z0, eps, dflat, dz0, dts, train=True):
    c = lambda a: _c(a, np.float32)
    return generate_jvp(cfg, c(flat), c(z0), c(eps), c(dflat), c(dz0), dts, train)


# ---- the bar: tests/envelope.py:10-16 and vjp_ref.py:143-149, unchanged ----
def bar(ref64, ref32):
    """(scale, floor, rtol) of one tangent array: scale = max|ref64| + rms ref64, floor = max|ref32 - ref64| / scale (the float32
    run of THIS reference, never the device), rtol = max(1e-4, 8 floor)."""
    s = V.scale(ref64)
    floor = float(np.abs(np.asarray(ref32, np.float64) - np.asarray(ref64, np.float64)).max()) / s if s > 0 else 0.0
    return s, floor, max(V.RTOL, V.FLOOR_FACTOR * floor)


FLOOR_CAP = V.RTOL_CAP / V.FLOOR_FACTOR                  # 1.25e-4: above it the bar would pass the cap of 1e-3


def assert_tangent(got, ref64, ref32, what):
    """max|got - ref64| <= rtol (max|ref64| + rms ref64), rtol = max(1e-4, 8 floor) <= 1e-3; an all-zero reference wants zeros."""
    s, floor, rtol = bar(ref64, ref32)
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref64, np.float64)).max())
    print(f"jvp | {what} | err/scale {err / s if s > 0 else err:.2e} floor {floor:.2e} rtol {rtol:.1e} scale {s:.3g}")
    assert rtol <= V.RTOL_CAP, f"{what}: the float32 reference's own error {floor:.3g} asks for rtol {rtol:.3g} > the cap"
    if s == 0:
        assert err == 0, f"{what}: the reference is zero, the device is not ({err:.3g})"
        return
    assert np.isfinite(err) and err <= rtol * s, f"{what}: off by {err / s:.3g} of its scale {s:.3g} (rtol {rtol:.3g}, floor {floor:.3g})"


# ---- the cases of the device tests (tests/test_gpu_jvp.py); tests/test_jvp_ref_host.py holds their floors under the cap ----
TANH2 = (O.ACT_TANH,) * 2
NETS = {
    "2-6-2": O.Cfg(O.Net((2, 6, 2), TANH2), 1, 1, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)),
    "16-48-16": O.Cfg(O.Net((16, 48, 16), TANH2), 8, 8, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)),
    "16-16": O.Cfg(O.Net((16, 16), (O.ACT_TANH,)), 16, 0, 1e-2, 1e-2, 0.0, tspan=(0.0, 1.0)),
}
# the other instantiations of the kernel: two hidden tiles, FOUR (64 hidden units: the most registers, every mode), and a real
# second layer with the identity activation (it has a direction of its own, unlike the appended one of "16-16")
NETS.update({
    "2-24-2": O.Cfg(O.Net((2, 24, 2), TANH2), 1, 1, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)),
    "2-64-2": O.Cfg(O.Net((2, 64, 2), TANH2), 1, 1, 1e-2, 1e-2, 1e-2, tspan=(0.0, 1.0)),
    "6-9-6-id": O.Cfg(O.Net((6, 9, 6), (O.ACT_TANH, O.ACT_IDENTITY)), 6, 0, 1e-2, 1e-2, 0.0, tspan=(0.0, 1.0)),
})
MAIN_NETS = ("2-6-2", "16-48-16", "16-16")               # every mode, every set of directions
MODES = ("vjp", "jvp", "test")
EXTRA_CASES = (("2-24-2", "vjp"), ("2-64-2", "vjp"), ("2-64-2", "jvp"), ("2-64-2", "test"), ("6-9-6-id", "vjp"), ("6-9-6-id", "test"))
R = 3


def case_cfg(net, mode):
    c = NETS[net]
    return O.Cfg(c.net, c.nvars, c.naugs, c.lam1, c.lam2, c.lam3, use_jvp=mode == "jvp", tspan=c.tspan)


def case_inputs(net, mode, B, seed=0, wscale=1.0):
    """(flat, xs, z0, eps, d_ps (R, n_params), d_xs (R, nvars, B), d_z0 (R, n_in, B)) float32; the third direction of each kind
    is v_1 + 2 v_2 (test 4 of the device suite)."""
    cfg = case_cfg(net, mode)
    rng = np.random.default_rng(4200 + 97 * seed + 13 * list(NETS).index(net) + MODES.index(mode))
    flat = np.float32(wscale) * O.glorot_params(cfg.net, rng, np.float32, 0.5)
    xs = rng.standard_normal((cfg.nvars, B)).astype(np.float32)
    z0 = rng.standard_normal((cfg.n_in, B)).astype(np.float32)
    eps = rng.standard_normal((cfg.n_in, B)).astype(np.float32)

    def dirs(*shape):
        d = rng.standard_normal((R,) + shape).astype(np.float32)
        d[2] = d[0] + np.float32(2) * d[1]
        return d
    return flat, xs, z0, eps, dirs(flat.size), dirs(cfg.nvars, B), dirs(cfg.n_in, B)


def host_steps(cfg, flat, xs, eps, train, sampling=False, **kw):
    """The steps the float64 oracle's own adaptive solve accepts (what the CPU test measures the floors on)."""
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    if sampling:
        D = cfg.D(train)
        u0 = np.vstack([f64(xs), np.zeros((D - cfg.n_in, xs.shape[1]))])
        t0, t1 = GR._span(cfg)
        _, st = O.tsit5_solve(cfg.rhs(f64(flat), f64(eps) if train else None, train), u0, t0, t1, **kw)
        return st.dts
    _, _, _, st = O.inference(cfg, f64(flat), f64(xs), f64(eps) if train else None, train, **kw)
    return st.dts
