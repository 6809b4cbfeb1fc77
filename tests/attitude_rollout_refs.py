"""Plain numpy restatement of hjb_rollout_run_attitude (include/hjbdp.h, csrc/kernels_rollout_attitude.h), the checker of
tests/test_gpu_rollout_attitude.py, vectorised over trajectories, one IEEE float64 operation at a time:
  atan2c / asinc: fdlibm's atan2 / asin in the kernel's form (+ - * /, sqrt, comparisons, selects; sign of zero by signbit);
  angles: quat_to_yaw_pitch_roll([X7 X6 X5 X4]) with them, no renormalisation first;
  lookup: the dense values u_table[labels[:, p] - base, j] through the oracle's C twin (oracle.c_oracle.lookup), as
          tests/rollout_refs.py does;
  cost += ((q1*(X1*X1) + q2*(X2*X2)) + ... + q7*(X7*X7)) + r1*(u1*u1) + r2*(u2*u2) + r3*(u3*u3);
  step: taylor X + h f(X) or RK4 with u held (hjbdp/rollout.py::next_stage_states), then X4..X7 / sqrt(((X4^2 + X5^2) + X6^2) + X7^2).
"""
from __future__ import annotations

import numpy as np

PI, PI_LO, PIO2_HI, PIO2_LO, PIO4_HI = (3.1415926535897931160e+00, 1.2246467991473531772e-16, 1.57079632679489655800e+00,
                                         6.12323399573676603587e-17, 7.85398163397448278999e-01)
ATAN_HI = np.array([4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00])
ATAN_LO = np.array([2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17])


def _atan_nonneg(x):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        conds = [x < 0.4375, x < 0.6875, x < 1.1875, x < 2.4375]
        idx = np.select(conds, [-1, 0, 1, 2], 3)
        r = np.select(conds, [x, (2.0 * x - 1.0) / (2.0 + x), (x - 1.0) / (x + 1.0), (x - 1.5) / (1.0 + 1.5 * x)], -1.0 / x)
        z = r * r
        w = z * z
        s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
                  w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))))
        s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
                  w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))))
        k = np.maximum(idx, 0)
        return np.where(idx < 0, r - r * (s1 + s2), ATAN_HI[k] - ((r * (s1 + s2) - ATAN_LO[k]) - r))


def atan2c(y, x):
    y, x = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64))
    ax, ay = np.abs(x), np.abs(y)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = _atan_nonneg(ay / ax)
    xneg = np.signbit(x)
    a = np.where(xneg, PI - (z - PI_LO), z)
    a = np.where(ax == 0.0, np.where(ay == 0.0, np.where(xneg, PI, 0.0), PIO2_HI), a)
    return np.where(np.signbit(y), -a, a)


def _pq(t):
    p = t * (1.66666666666666657415e-01 + t * (-3.25565818622400915405e-01 + t * (2.01212532134862925881e-01 +
             t * (-4.00555345006794114027e-02 + t * (7.91534994289814532176e-04 + t * 3.47933107596021167570e-05)))))
    q = 1.0 + t * (-2.40339491173441421878e+00 + t * (2.02094576023350569471e+00 + t * (-6.88283971605453293030e-01 +
                   t * 7.70381505559019352791e-02)))
    return p, q


def asinc(x):
    x = np.asarray(x, dtype=np.float64)
    ax = np.abs(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = ax * ax
        p, q = _pq(t)
        small = ax + ax * (p / q)
        t = (1.0 - ax) * 0.5
        p, q = _pq(t)
        s = np.sqrt(t)
        big = PIO2_HI - (2.0 * (s + s * (p / q)) - PIO2_LO)
        cs = s * 134217729.0
        sh = cs - (cs - s)
        c = (t - sh * sh) / (s + sh)
        pp = 2.0 * s * (p / q) - (PIO2_LO - 2.0 * c)
        qq = PIO4_HI - 2.0 * sh
        mid = PIO4_HI - (pp - qq)
    v = np.where(ax < 0.5, small, np.where(ax >= 0.975, big, mid))
    return np.where(np.signbit(x), -v, v)


def angles(X):
    """(yaw, pitch, roll) of the quaternion rows X[3:7] of X [7, n]."""
    x4, x5, x6, x7 = X[3], X[4], X[5], X[6]
    yaw = atan2c(2.0 * (x6 * x5 + x7 * x4), ((x7 * x7 + x6 * x6) - x5 * x5) - x4 * x4)
    s = -2.0 * (x6 * x4 - x7 * x5)
    s = np.where(s > 1.0, 1.0, np.where(s < -1.0, -1.0, s))
    pitch = asinc(s)
    roll = atan2c(2.0 * (x5 * x4 + x7 * x6), ((x7 * x7 - x6 * x6) - x5 * x5) + x4 * x4)
    return yaw, pitch, roll


def rates(X, U, J):
    """spacecraft_dynamics_list (Solver_attitude.m:600-620) with c1..c3 formed once, X [7, n], U [3, n]."""
    J1, J2, J3 = (float(v) for v in J)
    c1, c2, c3 = (J2 - J3) / J1, (J3 - J1) / J2, (J1 - J2) / J3
    x1, x2, x3, x4, x5, x6, x7 = X
    return np.stack([((c1 * x2) * x3) + U[0] / J1, ((c2 * x3) * x1) + U[1] / J2, ((c3 * x1) * x2) + U[2] / J3,
                     0.5 * (((x3 * x5) - (x2 * x6)) + (x1 * x7)), 0.5 * (((-x3 * x4) + (x1 * x6)) + (x2 * x7)),
                     0.5 * (((x2 * x4) - (x1 * x5)) + (x3 * x7)), 0.5 * (((-x1 * x4) - (x2 * x5)) - (x3 * x6))])


def step(X, U, J, h, integrator="taylor"):
    """One step and the renormalisation (next_stage_states, Solver_attitude.m:670-696)."""
    X = np.asarray(X, dtype=np.float64)
    k1 = rates(X, U, J)
    if integrator == "taylor":
        Xn = X + h * k1
    else:
        k2 = rates(X + (k1 * h) / 2.0, U, J)
        k3 = rates(X + (k2 * h) / 2.0, U, J)
        k4 = rates(X + k3 * h, U, J)
        Xn = X + (h * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)) / 6.0
    n = np.sqrt(((Xn[3] * Xn[3] + Xn[4] * Xn[4]) + Xn[5] * Xn[5]) + Xn[6] * Xn[6])
    Xn[3:7] = Xn[3:7] / n
    return Xn


def rollout(knots, labels, u_table, index_base, inertia, h, integrator, X0, plane_of_step, method="nearest", q=None, r=None):
    """knots: the 6 grid vectors (w1, w2, w3, yaw, pitch, roll); labels nS x n_planes (column-major, any shape); u_table [n_labels, 3];
    X0 [7, n].  Returns X_final [7, n], cost [n], X_path [n, 7, K+1], U_path [n, 3, K], A_path [n, 3, K]."""
    from hjbdp import _abi
    from oracle import c_oracle
    ks = [np.asarray(k, dtype=np.float64) for k in knots]
    nS = int(np.prod([len(k) for k in ks]))
    lab = np.asarray(labels).reshape(-1, order="F").reshape((nS, -1), order="F").astype(np.int64)
    ut = np.asarray(u_table, dtype=np.float64).reshape(-1, 3)
    q = np.zeros(7) if q is None else np.asarray(q, dtype=np.float64).reshape(7)
    r = np.zeros(3) if r is None else np.asarray(r, dtype=np.float64).reshape(3)
    x = np.array(np.asarray(X0, dtype=np.float64).reshape(7, -1))
    n = x.shape[1]
    planes = np.asarray(plane_of_step, dtype=np.int64).reshape(-1)
    K = planes.size
    X_path = np.zeros((n, 7, K + 1))
    U_path = np.zeros((n, 3, K))
    A_path = np.zeros((n, 3, K))
    cost = np.zeros(n)
    X_path[:, :, 0] = x.T
    for k, p in enumerate(planes):
        yaw, pitch, roll = angles(x)
        pts = np.ascontiguousarray(np.stack([x[0], x[1], x[2], yaw, pitch, roll], axis=1))
        u = np.empty((3, n))
        for j in range(3):
            u[j] = c_oracle.lookup(_abi, ks, ut[lab[:, p] - index_base, j], pts, method)
        g = q[0] * (x[0] * x[0])
        for a in range(1, 7):
            g = g + q[a] * (x[a] * x[a])
        for j in range(3):
            g = g + r[j] * (u[j] * u[j])
        cost = cost + g
        x = step(x, u, inertia, h, integrator)
        A_path[:, :, k] = np.stack([yaw, pitch, roll], axis=1)
        U_path[:, :, k] = u.T
        X_path[:, :, k + 1] = x.T
    return x, cost, X_path, U_path, A_path
