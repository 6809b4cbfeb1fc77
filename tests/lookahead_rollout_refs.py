"""Plain numpy restatement of hjb_rollout_run_lookahead (include/hjbdp.h), the checker of tests/test_rollout_lookahead_abi.py
and tests/test_gpu_rollout_lookahead.py.  It imports nothing of hjbdp's lookahead code.

Per step the candidates are formed for all trajectories at once, label by label and node by node in the library's stated order,
one IEEE operation at a time:
    gs, as_a once;   per label: g_l, xn_a (greedy_rollout_refs' operations);
    per node w: the query is xn with  xn_a + e[a][w]  on the axes of the lookahead mask (the axes with an offset that is not +-0)
                and xn_a itself, untouched, on the others;   v_w = blend of the plane at the query
    expect: acc = p_0 * v_0, then acc = fma(p_w, v_w, acc);   worst: acc = v_0, then acc = v_w where v_w > acc
    cand_l = g_l + acc;   best = cand_0; l >= 1 replaces iff cand_l < best
    flight: x = xn_best, then  x_a = x_a + d[a][w']  on the axes of the FLIGHT mask, w' the given node of the trajectory and step
The blend is the oracle's C twin (oracle.c_oracle.lookup 'linear' in float64) on the plane widened to float64; the fma is
disturbance_refs.fma64 (error-free transformations, one rounding).
"""
from __future__ import annotations

import numpy as np

from disturbance_refs import fma64 as fma


def mask_of(offsets):
    """the axes with at least one offset that is not +-0, as a list of bools"""
    off = np.asarray(offsets, dtype=np.float64)
    return [bool(np.any(off[a] != 0.0)) for a in range(off.shape[0])]


def rollout(knots, u_table, A, B, values, X0, plane_of_step, offsets, weights=None, mode="expect", c=None, q=None, r=None,
            index_base=0, nodes=None, flight_offsets=None):
    """greedy_rollout_refs.rollout's arguments; offsets [D, W], weights [W] or None (1.0 / W each), mode 'expect' / 'worst': the
    lookahead set; nodes [n, K] ints + flight_offsets [D, W_f]: the plant's noise as given nodes (None: nominal).
    Returns X_final [D, n], cost [n], X_path [n, D, K+1], U_path [n, n_u, K], L_path [n, K] int32, V_path [n, K]."""
    from hjbdp import _abi
    from oracle import c_oracle
    ks = [np.asarray(k, dtype=np.float64) for k in knots]
    D = len(ks)
    nS = int(np.prod([len(k) for k in ks]))
    ut = np.asarray(u_table, dtype=np.float64)
    ut = ut.reshape(-1, 1) if ut.ndim == 1 else ut
    nl, nu = ut.shape
    V = None if values is None else np.asarray(values).reshape(-1, order="F").reshape((nS, -1), order="F").astype(np.float64)
    A = np.asarray(A, dtype=np.float64).reshape(D, D)
    B = np.asarray(B, dtype=np.float64).reshape(D, nu)
    q = np.zeros(D) if q is None else np.asarray(q, dtype=np.float64).reshape(D)
    r = np.zeros(nu) if r is None else np.asarray(r, dtype=np.float64).reshape(nu)
    cv = None if c is None else np.asarray(c, dtype=np.float64).reshape(D)
    E = np.asarray(offsets, dtype=np.float64).reshape(D, -1)
    W = E.shape[1]
    P = np.full(W, 1.0 / W) if weights is None else np.asarray(weights, dtype=np.float64).reshape(W)
    lmask = mask_of(E)
    F = None if flight_offsets is None else np.asarray(flight_offsets, dtype=np.float64).reshape(D, -1)
    fmask = None if F is None else mask_of(F)
    x = np.array(np.asarray(X0, dtype=np.float64).reshape(D, -1))
    n = x.shape[1]
    planes = np.asarray(plane_of_step, dtype=np.int64).reshape(-1)
    K = planes.size
    X_path = np.zeros((n, D, K + 1))
    U_path = np.zeros((n, nu, K))
    L_path = np.zeros((n, K), dtype=np.int32)
    V_path = np.zeros((n, K))
    cost = np.zeros(n)
    X_path[:, :, 0] = x.T
    cols = np.arange(n)
    for k, p in enumerate(planes):
        gs = q[0] * (x[0] * x[0])
        for a in range(1, D):
            gs = gs + q[a] * (x[a] * x[a])
        parts = []
        for a in range(D):
            acc = A[a, 0] * x[0]
            for b in range(1, D):
                acc = acc + A[a, b] * x[b]
            parts.append(acc)
        G = np.empty((nl, n))
        XN = np.empty((nl, D, n))
        best = np.empty(n)
        lab = np.zeros(n, dtype=np.int64)
        for l in range(nl):
            g = gs
            for j in range(nu):
                g = g + r[j] * (ut[l, j] * ut[l, j])
            for a in range(D):
                acc = parts[a]
                for j in range(nu):
                    acc = acc + B[a, j] * ut[l, j]
                if cv is not None:
                    acc = acc + cv[a]
                XN[l, a] = acc
            G[l] = g
            if p < 0:
                acc = np.zeros(n)
            else:
                for w in range(W):
                    Q = np.array(XN[l])
                    for a in range(D):
                        if lmask[a]:
                            Q[a] = XN[l, a] + E[a, w]
                    v = c_oracle.lookup(_abi, ks, V[:, p], np.ascontiguousarray(Q.T), "linear")
                    if mode == "worst":
                        acc = v if w == 0 else np.where(v > acc, v, acc)
                    else:
                        acc = P[0] * v if w == 0 else fma(np.broadcast_to(P[w], v.shape), v, acc)
            cand = g + acc
            if l == 0:
                best[:] = cand
            else:
                take = cand < best
                best[take] = cand[take]
                lab[take] = l
        cost = cost + G[lab, cols]
        x = np.ascontiguousarray(XN[lab, :, cols].T)
        if nodes is not None:
            wk = np.asarray(nodes)[:, k]
            for a in range(D):
                if fmask[a]:
                    x[a] = x[a] + F[a, wk]
        U_path[:, :, k] = ut[lab]
        L_path[:, k] = lab + index_base
        V_path[:, k] = best
        X_path[:, :, k + 1] = x.T
    return x, cost, X_path, U_path, L_path, V_path


def node_sets(rng, D, W, lmask_axes, with_weights=True):
    """a seeded lookahead set: offsets [D, W] non-zero on lmask_axes only (one entry an exact 0.0, one a -0.0 where there is room),
    weights [W] positive, not summing to 1 (they are used as given), or None"""
    E = np.zeros((D, W))
    for a in lmask_axes:
        E[a] = rng.uniform(-0.3, 0.3, size=W)
    if W >= 2 and lmask_axes:
        E[lmask_axes[0], 0] = 0.0
        if len(lmask_axes) > 1:
            E[lmask_axes[-1], 1] = -0.0
    P = rng.uniform(0.1, 0.6, size=W) if with_weights else None
    return E, P
