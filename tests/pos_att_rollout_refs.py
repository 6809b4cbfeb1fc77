"""Plain numpy restatement of hjb_rollout_run_pos_att (include/hjbdp.h, csrc/kernels_rollout_pos_att.h), the checker of
tests/test_gpu_rollout_pos_att.py, vectorised over trajectories, one IEEE float64 operation at a time:
  t_i = 2 * asinc(clamp(X[6+i], -1, 1)) with attitude_rollout_refs.asinc;
  M = ECI2body(q) * RSW, xb = M x, vb = M v;
  per channel the 'nearest' lookup of the label through the oracle's C twin (oracle.c_oracle.lookup, as tests/rollout_refs.py
  does: the labels of plane p as dense double values), then its row of the thruster table;
  U_M, a = RSWinv (inv3(ECI2body(q)) a_body), inv3 the adjugate over the determinant;
  S classical RK4 sub-steps of h / S with a and U_M held, the orbit scalars from the table's nodes 2 (S k + s) + {0, 1, 1, 2}.
Nothing here comes from the package's kernel path (hjbdp._abi only names the oracle's library).
"""
from __future__ import annotations

import numpy as np

from attitude_rollout_refs import asinc

SLOTS = ((0, 1, 6, 7), (2, 3, 8, 9), (4, 5, 10, 11))      # thrusters of channel x, y, z
AXIS = (1, 2, 0)                                           # channel x looks up at the angle / rate about y, y about z, z about x


def inv3(m):
    """m [9, ...] row-major -> its inverse [9, ...]: adjugate over determinant, the library's order (pa_inv3)."""
    with np.errstate(all="ignore"):
        c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4]
        c10, c11, c12 = m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5]
        c20, c21, c22 = m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]
        det = (m[0] * c00 + m[1] * c10) + m[2] * c20
        return np.stack([c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det])


def mul3(m, v0, v1, v2):
    return [(m[3 * r] * v0 + m[3 * r + 1] * v1) + m[3 * r + 2] * v2 for r in range(3)]


def eci2body(q1, q2, q3, q4):
    return [1.0 - 2.0 * (q2 * q2 + q3 * q3), 2.0 * (q1 * q2 + q3 * q4), 2.0 * (q1 * q3 - q2 * q4),
            2.0 * (q2 * q1 - q3 * q4), 1.0 - 2.0 * (q1 * q1 + q3 * q3), 2.0 * (q2 * q3 + q1 * q4),
            2.0 * (q3 * q1 + q2 * q4), 2.0 * (q3 * q2 - q1 * q4), 1.0 - 2.0 * (q1 * q1 + q2 * q2)]


def rates(J, Ji, c, a, um, y):
    c0, c1, c2, c3, c4 = (float(v) for v in c)
    q1, q2, q3, q4, w1, w2, w3 = y[6:13]
    jw = mul3(J, w1, w2, w3)
    t = [um[0] - (w2 * jw[2] - w3 * jw[1]), um[1] - (w3 * jw[0] - w1 * jw[2]), um[2] - (w1 * jw[1] - w2 * jw[0])]
    return np.stack([y[3], y[4], y[5],
                     ((c0 * y[0] - c1 * y[1]) + c2 * y[4]) + a[0],
                     ((c1 * y[0] - c3 * y[1]) - c2 * y[3]) + a[1],
                     a[2] - c4 * y[2],
                     0.5 * (((w3 * q2) - (w2 * q3)) + (w1 * q4)),
                     0.5 * (((w1 * q3) - (w3 * q1)) + (w2 * q4)),
                     0.5 * (((w2 * q1) - (w1 * q2)) + (w3 * q4)),
                     0.5 * (((-(w1 * q1)) - (w2 * q2)) - (w3 * q3))] + mul3(Ji, t[0], t[1], t[2]))


def prepare_channels(channels):
    """(knots, labels, u_table, index_base) per channel -> (knots, labels [nS, n_planes], u_table [n_labels, 4], index_base, a cache
    of the planes as dense double values)."""
    chans = []
    for knots, labels, ut, base in channels:
        ks = [np.asarray(k, dtype=np.float64) for k in knots]
        nS = int(np.prod([len(k) for k in ks]))
        lab = np.asarray(labels).reshape(-1, order="F").reshape((nS, -1), order="F")
        chans.append((ks, lab, np.asarray(ut, dtype=np.float64).reshape(-1, 4), int(base), {}))
    return chans


def moments_and_acceleration(f, E, RSWi, mass, t_dist):
    """Thruster levels f [12, n] at attitude E = eci2body(q) -> (U_M [3], a [3]): the body moments and the acceleration in RSW."""
    um = [(((f[4] - f[5]) + f[10]) - f[11]) * t_dist, (((f[0] - f[1]) + f[6]) - f[7]) * t_dist,
          (((f[2] - f[3]) + f[8]) - f[9]) * t_dist]
    ab = [(((f[0] + f[1]) + f[6]) + f[7]) / mass, (((f[2] + f[3]) + f[8]) + f[9]) / mass, (((f[4] + f[5]) + f[10]) + f[11]) / mass]
    Ei = inv3(np.stack(E))
    ae = mul3(Ei, ab[0], ab[1], ab[2])
    return um, mul3(RSWi, ae[0], ae[1], ae[2])


def rk4_stage(J, Ji, coef, k, S, hs, a, um, x):
    """Stage k: S classical RK4 sub-steps of hs with a and um held, the orbit scalars from nodes 2 (S k + s) + {0, 1, 1, 2}."""
    for sub in range(S):
        j = 2 * (S * k + sub)
        r = rates(J, Ji, coef[j], a, um, x)
        acc = r
        xt = x + (r * hs) / 2.0
        r = rates(J, Ji, coef[j + 1], a, um, xt)
        acc = acc + 2.0 * r
        xt = x + (r * hs) / 2.0
        r = rates(J, Ji, coef[j + 1], a, um, xt)
        acc = acc + 2.0 * r
        xt = x + r * hs
        r = rates(J, Ji, coef[j + 2], a, um, xt)
        x = x + (hs * (acc + r)) / 6.0
    return x


def rollout(channels, inertia, mass, t_dist, h, substeps, rsw2eci, coef, X0, plane_of_step):
    """channels: for x, y, z (knots [4 grid vectors], labels nS x n_planes (column-major, any shape), u_table [n_labels, 4],
    index_base); inertia, rsw2eci [3, 3]; coef [n_nodes, 5]; X0 [13, n].
    Returns X_final [13, n], X_path [n, 13, K+1], F_path [n, 12, K], FM_path [n, 6, K]."""
    from hjbdp import _abi
    from oracle import c_oracle
    chans = prepare_channels(channels)
    J = [float(v) for v in np.asarray(inertia, dtype=np.float64).reshape(9)]
    Ji = [float(v) for v in inv3(np.array(J))]
    RSW = [float(v) for v in np.asarray(rsw2eci, dtype=np.float64).reshape(9)]
    RSWi = [float(v) for v in inv3(np.array(RSW))]
    S = int(substeps)
    hs = float(h) / S
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 5)
    x = np.array(np.asarray(X0, dtype=np.float64).reshape(13, -1))
    n = x.shape[1]
    planes = np.asarray(plane_of_step, dtype=np.int64).reshape(-1)
    K = planes.size
    X_path = np.zeros((n, 13, K + 1))
    F_path = np.zeros((n, 12, K))
    FM_path = np.zeros((n, 6, K))
    X_path[:, :, 0] = x.T
    with np.errstate(all="ignore"):
        for k, p in enumerate(planes):
            s = x[6:9]
            s = np.where(s > 1.0, 1.0, np.where(s < -1.0, -1.0, s))
            th = 2.0 * asinc(s)
            E = eci2body(x[6], x[7], x[8], x[9])
            M = [(E[3 * r] * RSW[c] + E[3 * r + 1] * RSW[3 + c]) + E[3 * r + 2] * RSW[6 + c] for r in range(3) for c in range(3)]
            xb, vb = mul3(M, x[0], x[1], x[2]), mul3(M, x[3], x[4], x[5])
            f = np.zeros((12, n))
            for ch, (ks, lab, ut, base, dense) in enumerate(chans):
                if p not in dense:
                    dense[p] = lab[:, p].astype(np.float64)
                pts = np.ascontiguousarray(np.stack([xb[ch], vb[ch], th[AXIS[ch]], x[10 + AXIS[ch]]], axis=1))
                L = c_oracle.lookup(_abi, ks, dense[p], pts, "nearest").astype(np.int64) - base
                for j, slot in enumerate(SLOTS[ch]):
                    f[slot] = ut[L, j]
            um, a = moments_and_acceleration(f, E, RSWi, mass, t_dist)
            F_path[:, :, k] = f.T
            FM_path[:, :, k] = np.stack(a + um, axis=1)
            x = rk4_stage(J, Ji, coef, k, S, hs, a, um, x)
            X_path[:, :, k + 1] = x.T
    return x, X_path, F_path, FM_path
