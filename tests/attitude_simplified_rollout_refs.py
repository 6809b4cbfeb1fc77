"""Plain numpy restatement of hjb_rollout_run_attitude_simplified (include/hjbdp.h, csrc/kernels_rollout_attitude_simplified.h),
the checker of tests/test_gpu_rollout_attitude_simplified.py, vectorised over trajectories, one IEEE float64 operation at a time:
  t_i = 2 * asinc(clamp(X[3+i], -1, 1)) with attitude_rollout_refs.asinc;
  u_i: per channel the 'nearest' lookup of the label through the oracle's C twin (oracle.c_oracle.lookup, as
       tests/pos_att_rollout_refs.py does: the labels of plane p as dense double values), then its entry of the torque table;
  cost += (g_0 + g_1) + g_2, g_i = (qw_i * (w_i * w_i) + qt_i * (t_i * t_i)) + r_i * (u_i * u_i);
  'full': S classical RK4 sub-steps of h / S with u held, w_dot = inv3(J) (u - w x (J w)) (inv3, mul3 of pos_att_rollout_refs),
          the quaternion rates in the pos-att loop's order, no renormalisation;
  'diagonal': attitude_rollout_refs.step(., 'RK4') at diag(J): one RK4 step, then q / |q|.
Nothing here comes from the package's kernel path (hjbdp._abi only names the oracle's library).
"""
from __future__ import annotations

import numpy as np

from attitude_rollout_refs import asinc, step
from pos_att_rollout_refs import inv3, mul3


def rates(J, Ji, u, y):
    w1, w2, w3, q1, q2, q3, q4 = y
    jw = mul3(J, w1, w2, w3)
    t = [u[0] - (w2 * jw[2] - w3 * jw[1]), u[1] - (w3 * jw[0] - w1 * jw[2]), u[2] - (w1 * jw[1] - w2 * jw[0])]
    return np.stack(mul3(Ji, t[0], t[1], t[2]) + [0.5 * (((w3 * q2) - (w2 * q3)) + (w1 * q4)),
                                                  0.5 * (((w1 * q3) - (w3 * q1)) + (w2 * q4)),
                                                  0.5 * (((w2 * q1) - (w1 * q2)) + (w3 * q4)),
                                                  0.5 * (((-(w1 * q1)) - (w2 * q2)) - (w3 * q3))])


def rollout(channels, inertia, h, substeps, dynamics, X0, plane_of_step, qw=None, qt=None, r=None):
    """channels: for 1, 2, 3 (knots [s_w, s_t], labels nS x n_planes (column-major, any shape), u_table [n_labels] or [n_labels, 1],
    index_base); inertia [3, 3]; dynamics 'full' or 'diagonal'; X0 [7, n].
    Returns X_final [7, n], cost [n], X_path [n, 7, K+1], U_path [n, 3, K], A_path [n, 3, K]."""
    from hjbdp import _abi
    from oracle import c_oracle
    chans = []
    for knots, labels, ut, base in channels:
        ks = [np.asarray(k, dtype=np.float64) for k in knots]
        nS = int(np.prod([len(k) for k in ks]))
        lab = np.asarray(labels).reshape(-1, order="F").reshape((nS, -1), order="F")
        chans.append((ks, lab, np.asarray(ut, dtype=np.float64).reshape(-1), int(base), {}))
    Jm = np.asarray(inertia, dtype=np.float64).reshape(3, 3)
    J = [float(v) for v in Jm.reshape(9)]
    Ji = [float(v) for v in inv3(np.array(J))]
    Jd = [J[0], J[4], J[8]]
    S = int(substeps)
    assert dynamics in ("full", "diagonal") and S >= 1 and (dynamics == "full" or S == 1)
    hs = float(h) / S
    w = lambda v: np.zeros(3) if v is None else np.asarray(v, dtype=np.float64).reshape(3)
    qw, qt, r = w(qw), w(qt), w(r)
    x = np.array(np.asarray(X0, dtype=np.float64).reshape(7, -1))
    n = x.shape[1]
    planes = np.asarray(plane_of_step, dtype=np.int64).reshape(-1)
    K = planes.size
    X_path = np.zeros((n, 7, K + 1))
    U_path = np.zeros((n, 3, K))
    A_path = np.zeros((n, 3, K))
    cost = np.zeros(n)
    X_path[:, :, 0] = x.T
    with np.errstate(all="ignore"):
        for k, p in enumerate(planes):
            s = x[3:6]
            s = np.where(s > 1.0, 1.0, np.where(s < -1.0, -1.0, s))
            th = 2.0 * asinc(s)
            u = np.zeros((3, n))
            for ch, (ks, lab, ut, base, dense) in enumerate(chans):
                if p not in dense:
                    dense[p] = lab[:, p].astype(np.float64)
                pts = np.ascontiguousarray(np.stack([x[ch], th[ch]], axis=1))
                u[ch] = ut[c_oracle.lookup(_abi, ks, dense[p], pts, "nearest").astype(np.int64) - base]
            g = [(qw[j] * (x[j] * x[j]) + qt[j] * (th[j] * th[j])) + r[j] * (u[j] * u[j]) for j in range(3)]
            cost = cost + ((g[0] + g[1]) + g[2])
            A_path[:, :, k] = th.T
            U_path[:, :, k] = u.T
            if dynamics == "full":
                for _ in range(S):
                    f = rates(J, Ji, u, x)
                    acc = f
                    xt = x + (f * hs) / 2.0
                    f = rates(J, Ji, u, xt)
                    acc = acc + 2.0 * f
                    xt = x + (f * hs) / 2.0
                    f = rates(J, Ji, u, xt)
                    acc = acc + 2.0 * f
                    xt = x + f * hs
                    f = rates(J, Ji, u, xt)
                    x = x + (hs * (acc + f)) / 6.0
            else:
                x = step(x, u, Jd, float(h), "RK4")
            X_path[:, :, k + 1] = x.T
    return x, cost, X_path, U_path, A_path
