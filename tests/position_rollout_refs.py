"""Plain numpy restatement of hjb_rollout_run_position (include/hjbdp.h, csrc/kernels_rollout_position.h), the checker of
tests/test_gpu_rollout_position.py, vectorised over trajectories, one IEEE float64 operation at a time:
  per channel i the 'nearest' lookup of the label at (y_i, y_3+i) through the oracle's C twin (oracle.c_oracle.lookup, as
  tests/rollout_refs.py does: the acceleration of plane p's labels as dense double values);
  per sub-step of the stage's table rows the six Fehlberg stage derivatives formed with h_form, the error estimate and the
  off-schedule test allowed >= 1100 * (te_max + eps) (false for NaN), the update applied over h_apply.
The tableau below is Fehlberg's 4(5), written out again: nothing here comes from the package's kernel path or its host loops
(hjbdp._abi only names the oracle's library).
"""
from __future__ import annotations

import numpy as np

B = ((),
     (1.0 / 4,),
     (3.0 / 32, 9.0 / 32),
     (1932.0 / 2197, -7200.0 / 2197, 7296.0 / 2197),
     (439.0 / 216, -8.0, 3680.0 / 513, -845.0 / 4104),
     (-8.0 / 27, 2.0, -3544.0 / 2565, 1859.0 / 4104, -11.0 / 40))
C4 = (25.0 / 216, 0.0, 1408.0 / 2565, 2197.0 / 4104, -1.0 / 5, 0.0)
C5 = (16.0 / 135, 0.0, 6656.0 / 12825, 28561.0 / 56430, -9.0 / 50, 2.0 / 55)
USED = (0, 2, 3, 4, 5)                                     # C4_1 = C5_1 = 0: no term
EPS = 2.0 ** -52
MARGIN = 1100.0


def rates(c, a, y):
    c0, c1, c2, c3, c4 = (float(v) for v in c)
    return np.stack([y[3], y[4], y[5],
                     ((c0 * y[0] - c1 * y[1]) + c2 * y[4]) + a[0],
                     ((c1 * y[0] - c3 * y[1]) - c2 * y[3]) + a[1],
                     a[2] - c4 * y[2]])


def absmax(m, v):
    """max(m, |v|) elementwise that keeps a NaN once met"""
    v = np.abs(v)
    return np.where((v > m) | (v != v), v, m)


def rollout(channels, n_sub, table, tol, X0, plane_of_step):
    """channels: for x, y, z (knots [2 grid vectors], labels nS x n_planes (column-major, any shape), u_table [n_labels] or
    [n_labels, 1], index_base); n_sub [>= K]; table [>= K, max_sub, 32]; X0 [6, n].
    Returns X_final [6, n], X_path [n, 6, K+1], A_path [n, 3, K], off_schedule [n] int32."""
    from hjbdp import _abi
    from oracle import c_oracle
    chans = []
    for knots, labels, ut, base in channels:
        ks = [np.asarray(k, dtype=np.float64) for k in knots]
        nS = int(np.prod([len(k) for k in ks]))
        lab = np.asarray(labels).reshape(-1, order="F").reshape((nS, -1), order="F").astype(np.int64)
        chans.append((ks, lab, np.asarray(ut, dtype=np.float64).reshape(-1), int(base), {}))
    table = np.asarray(table, dtype=np.float64)
    tol = float(tol)
    y = np.array(np.asarray(X0, dtype=np.float64).reshape(6, -1))
    n = y.shape[1]
    planes = np.asarray(plane_of_step, dtype=np.int64).reshape(-1)
    K = planes.size
    X_path = np.zeros((n, 6, K + 1))
    A_path = np.zeros((n, 3, K))
    off = np.full(n, -1, np.int32)
    X_path[:, :, 0] = y.T
    d = [C4[j] - C5[j] for j in range(6)]
    with np.errstate(all="ignore"):
        for k, p in enumerate(planes):
            a = []
            for ch, (ks, lab, ut, base, dense) in enumerate(chans):
                if p not in dense:
                    dense[p] = ut[lab[:, p] - base]
                pts = np.ascontiguousarray(np.stack([y[ch], y[3 + ch]], axis=1))
                a.append(c_oracle.lookup(_abi, ks, dense[p], pts, "nearest"))
            A_path[:, :, k] = np.stack(a, axis=1)
            on = np.ones(n, bool)
            for s in range(int(n_sub[k])):
                row = table[k, s]
                hf, ha = float(row[0]), float(row[1])
                f = [rates(row[2:7], a, y)]
                for st in range(1, 6):
                    yin = y
                    for j in range(st):
                        yin = yin + (hf * B[st][j]) * f[j]
                    f.append(rates(row[2 + 5 * st:7 + 5 * st], a, yin))
                e = f[0] * d[0]
                s5 = f[0] * C5[0]
                for j in USED[1:]:
                    e = e + f[j] * d[j]
                    s5 = s5 + f[j] * C5[j]
                te, ym = np.zeros(n), np.ones(n)
                for i in range(6):
                    te = absmax(te, hf * e[i])
                    ym = absmax(ym, y[i])
                on &= tol * ym >= MARGIN * (te + EPS)
                y = y + ha * s5
            off = np.where(~on & (off < 0), np.int32(k), off).astype(np.int32)
            X_path[:, :, k + 1] = y.T
    return y, X_path, A_path, off
