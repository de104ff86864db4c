"""Reference for flow paths (cnf_solve_path): Tsit5's dense output in numpy, in the dtype it is given.

* ``tsit5_step_all``: one Tsit5 step that returns all seven ``k`` (the tableau of oracle/cnf_oracle.py);
* ``dense_b`` / ``interpolate``: the interpolant ``u_n + h sum_i b_i(theta) k_i``, ``b_i(theta) = theta (r_i1 + theta (r_i2 +
  theta (r_i3 + theta r_i4)))`` (Tsitouras 2011, as OrdinaryDiffEq's Tsit5 uses it; third party in the reference, restated);
* ``replay``: the device's own accepted steps (cnf_path_steps) taken again, and the slices at ``saveat`` by the bracketing rule of
  include/cnfhip_path.h: ``tau`` is served by the step with ``t_n < tau <= t_n + h`` along the direction, the last step takes
  everything left, ``tau == t_start`` is ``u0`` and the end of a step is the accepted state itself.
"""
import numpy as np

from oracle import cnf_oracle as O

R = np.array([
    [1.0, -2.763706197274826, 2.9132554618219126, -1.0530884977290216],
    [0.0, 0.13169999999999998, -0.2234, 0.1017],
    [0.0, 3.9302962368947516, -5.941033872131505, 2.490627285651253],
    [0.0, -12.411077166933676, 30.33818863028232, -16.548102889244902],
    [0.0, 37.50931341651104, -88.1789048947664, 47.37952196281928],
    [0.0, -27.896526289197286, 65.09189467479366, -34.87065786149661],
    [0.0, 1.5, -4.0, 2.5]])


def dense_b(theta, dtype=np.float64):
    """The seven ``b_i(theta)`` in ``dtype`` (Horner)."""
    T = np.dtype(dtype).type
    th = T(theta)
    r = R.astype(dtype)
    return [th * (r[i, 0] + th * (r[i, 1] + th * (r[i, 2] + th * r[i, 3]))) for i in range(7)]


def tsit5_step_all(f, u, k1, dt):
    """One Tsit5 step from ``(u, k1 = f(u))``: ``(u_new, [k_1 .. k_7])`` in ``u``'s dtype."""
    T = u.dtype.type
    ks = [k1]
    for s in range(1, 7):
        acc = T(O.TSIT5_A[s][0]) * ks[0]
        for j in range(1, s):
            acc = acc + T(O.TSIT5_A[s][j]) * ks[j]
        us = u + T(dt) * acc
        ks.append(f(us))
    return us, ks


def interpolate(u, ks, h, theta):
    """``u + h sum_i b_i(theta) k_i`` in ``u``'s dtype."""
    T = u.dtype.type
    b = dense_b(theta, u.dtype)
    acc = b[0] * ks[0]
    for j in range(1, 7):
        acc = acc + b[j] * ks[j]
    return u + T(h) * acc


def replay(f, u0, tspan, steps_t, steps_h, saveat, dtype=np.float64):
    """The slices ``[K, D, B]`` at ``saveat`` and the final state, from the accepted steps ``(steps_t[n], steps_h[n])`` the
    device took (float32 values, used as they are) with the arithmetic in ``dtype``."""
    T = np.dtype(dtype).type
    t0, t1 = np.float32(tspan[0]), np.float32(tspan[1])
    sv = np.asarray(saveat, dtype=np.float32)
    d = 1.0 if t1 >= t0 else -1.0
    u = np.asarray(u0).astype(dtype)
    out = np.full((sv.size,) + u.shape, np.nan, dtype=dtype)
    cur = 0
    while cur < sv.size and sv[cur] == t0:
        out[cur] = u
        cur += 1
    k1 = f(u)
    N = len(steps_t)
    for n in range(N):
        tn, hn = np.float32(steps_t[n]), np.float32(steps_h[n])
        last = n == N - 1
        t_end = t1 if last else np.float32(steps_t[n + 1])
        u_new, ks = tsit5_step_all(f, u, k1, T(hn))
        while cur < sv.size:
            tau = sv[cur]
            if not last and d * (float(tau) - float(t_end)) > 0:
                break
            theta = (T(tau) - T(tn)) / T(hn)
            out[cur] = u_new if (tau == t_end or not theta < 1) else interpolate(u, ks, hn, theta)
            cur += 1
        u, k1 = u_new, ks[6]
    assert cur == sv.size, "save times left unserved"
    return out, u
