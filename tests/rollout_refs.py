"""Plain numpy restatement of hjb_rollout_run (include/hjbdp.h), the checker of tests/test_gpu_rollout.py.

Per step the dense control values u_table[labels[:, p] - base, j] are looked up with the oracle's C twin (oracle.c_oracle.lookup,
bit-exact with k_policy_lookup in float64); the stage cost and the affine update are formed elementwise in the library's stated
order, one IEEE operation at a time:
    g = ((q0*(x0*x0) + q1*(x1*x1)) + ...) + r0*(u0*u0) + ...;   cost += g
    x+_a = ((A[a,0]*x0 + A[a,1]*x1) + ...) + B[a,0]*u0 + ... + c_a
"""
from __future__ import annotations

import numpy as np


def rollout(knots, labels, u_table, index_base, A, B, X0, plane_of_step, method="linear", c=None, q=None, r=None):
    """knots: D grid vectors; labels: nS x n_planes (column-major, any shape); u_table [n_labels, n_u]; X0 [D, n].
    Returns X_final [D, n], cost [n], X_path [n, D, K+1], U_path [n, n_u, K]."""
    from hjbdp import _abi
    from oracle import c_oracle
    ks = [np.asarray(k, dtype=np.float64) for k in knots]
    D = len(ks)
    nS = int(np.prod([len(k) for k in ks]))
    lab = np.asarray(labels).reshape(-1, order="F").reshape((nS, -1), order="F").astype(np.int64)
    ut = np.asarray(u_table, dtype=np.float64)
    ut = ut.reshape(-1, 1) if ut.ndim == 1 else ut
    nu = ut.shape[1]
    A = np.asarray(A, dtype=np.float64).reshape(D, D)
    B = np.asarray(B, dtype=np.float64).reshape(D, nu)
    q = np.zeros(D) if q is None else np.asarray(q, dtype=np.float64).reshape(D)
    r = np.zeros(nu) if r is None else np.asarray(r, dtype=np.float64).reshape(nu)
    x = np.array(np.asarray(X0, dtype=np.float64).reshape(D, -1))
    n = x.shape[1]
    planes = np.asarray(plane_of_step, dtype=np.int64).reshape(-1)
    K = planes.size
    X_path = np.zeros((n, D, K + 1))
    U_path = np.zeros((n, nu, K))
    cost = np.zeros(n)
    X_path[:, :, 0] = x.T
    for k, p in enumerate(planes):
        u = np.empty((nu, n))
        pts = np.ascontiguousarray(x.T)
        for j in range(nu):
            dense = ut[lab[:, p] - index_base, j]
            u[j] = c_oracle.lookup(_abi, ks, dense, pts, method)
        g = q[0] * (x[0] * x[0])
        for a in range(1, D):
            g = g + q[a] * (x[a] * x[a])
        for j in range(nu):
            g = g + r[j] * (u[j] * u[j])
        cost = cost + g
        xn = np.empty_like(x)
        for a in range(D):
            acc = A[a, 0] * x[0]
            for b in range(1, D):
                acc = acc + A[a, b] * x[b]
            for j in range(nu):
                acc = acc + B[a, j] * u[j]
            if c is not None:
                acc = acc + float(np.asarray(c, dtype=np.float64).reshape(D)[a])
            xn[a] = acc
        x = xn
        U_path[:, :, k] = u.T
        X_path[:, :, k + 1] = x.T
    return x, cost, X_path, U_path
