"""Plain numpy restatement of hjb_rollout_run_control_lookahead (include/hjbdp.h), the checker of
tests/test_control_lookahead_refs.py, tests/test_gpu_rollout_ctrl_lookahead.py and tests/test_gpu_rollout_ctrl_lookahead_campaign.py.
It imports nothing of hjbdp's lookahead code.

tests/lookahead_rollout_refs.py's loop with the contract's one change: node w of the candidate with 0-based label l queries
    xn_a + e[a][w][l]  on the axes of the mask (the axes with SOME (w, l) entry that is not +-0),  xn_a itself on the others,
every node for every candidate.  The flown plant is the actuator plant of tests/actuator_rollout_refs.py (its steps 1 - 4) on the
chosen label's xn and commanded u, at nodes drawn by tests/noisy_rollout_refs.py's sampler; the cost is charged on the commanded u.
The blend is the oracle's C twin on the plane widened to float64, the fma disturbance_refs.fma64.
"""
from __future__ import annotations

import numpy as np

from actuator_rollout_refs import eps_matrix
from disturbance_refs import fma64 as fma
from noisy_rollout_refs import draw, thresholds


def mask_of(offsets):
    """the axes with at least one (w, l) entry that is not +-0, as a list of bools; offsets [D, W, n_labels]"""
    off = np.asarray(offsets, dtype=np.float64)
    return [bool(np.any(off[a] != 0.0)) for a in range(off.shape[0])]


def actuator_plant(xn, u, B, eps, base, w):
    """tests/actuator_rollout_refs.py's steps 1 - 4 on the affine update xn [D, n] and the commanded u [n_u, n] at the nodes w [n]:
    eps [W] or [W, n_u], base [D, W] or None.  Returns x+ [D, n]."""
    D, nu = xn.shape[0], u.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(D, nu)
    e = eps_matrix(eps, nu)                                                     # [n_u, W]
    W = e.shape[1]
    live = [bool(np.any(e[j] != 0.0)) for j in range(nu)]
    bs = None if base is None else np.asarray(base, dtype=np.float64).reshape(D, W)
    base_axis = [bs is not None and bool(np.any(bs[a] != 0.0)) for a in range(D)]
    ue = {j: u[j] * e[j, w] for j in range(nu) if live[j]}                      # step 1
    out = np.array(xn)
    for a in range(D):
        terms = [B[a, j] * ue[j] for j in range(nu) if live[j] and B[a, j] != 0.0]      # step 2
        if base_axis[a]:
            terms.append(bs[a, w])
        if terms:                                                               # steps 3 and 4
            na = terms[0]
            for t in terms[1:]:
                na = na + t
            out[a] = xn[a] + na
    return out


def drawn_nodes(weights, W, n_traj, n_steps, seed, first_stream):
    """the nodes a flown run draws: noisy_rollout_refs' sampler, [n_traj, n_steps] int32"""
    return draw(thresholds(weights, W), seed, first_stream, n_traj, n_steps)


def rollout(knots, u_table, A, B, values, X0, plane_of_step, offsets, weights=None, mode="expect", c=None, q=None, r=None,
            index_base=0, nodes=None, eps=None, base=None):
    """lookahead_rollout_refs.rollout's arguments with offsets [D, W, n_labels]; nodes [n, K] ints + eps (+ base): the actuator
    plant at given nodes (None: nominal).  Returns X_final [D, n], cost [n], X_path [n, D, K+1], U_path [n, n_u, K] (the commanded
    u), L_path [n, K] int32, V_path [n, K]."""
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
    E = np.asarray(offsets, dtype=np.float64)
    assert E.ndim == 3 and E.shape[0] == D and E.shape[2] == nl, E.shape
    W = E.shape[1]
    P = np.full(W, 1.0 / W) if weights is None else np.asarray(weights, dtype=np.float64).reshape(W)
    lmask = mask_of(E)
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
                            Q[a] = XN[l, a] + E[a, w, l]
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
        cost = cost + G[lab, cols]                                              # on the COMMANDED u
        x = np.ascontiguousarray(XN[lab, :, cols].T)
        if nodes is not None:
            x = actuator_plant(x, np.ascontiguousarray(ut[lab].T), B, eps, base, np.asarray(nodes)[:, k])
        U_path[:, :, k] = ut[lab]
        L_path[:, k] = lab + index_base
        V_path[:, k] = best
        X_path[:, :, k + 1] = x.T
    return x, cost, X_path, U_path, L_path, V_path


PLANES = [2, 0, -1, 1, 1]                  # 5 steps: -1 inside, a plane repeated, the Philox block of k = 4 begins inside
N_TRAJ = 70                                # more than one wave, less than a block


def problem(D, dtype, salt=0):
    """The seeded problem of instantiation (D, dtype) for the GPU tests, the smallest at which the kernels can still go wrong: 4 - 5
    NON-UNIFORM knots per axis (4 at D = 6: 4^6 nodes), 3 - 7 labels, n_u cycling over 1 - 4 with zeros in B (from two inputs on), a
    per-control set of 3 nodes on a proper subset of the axes (from D = 2 on) with signed zeros and one all-zero candidate, an
    actuator set of 3 nodes with a dead input and a base, N_TRAJ starts of which a third lie outside the grid on both sides.
    Returns a dict: model (control_lookahead_host's leading arguments), E, P, mode, eps, base, Pf, X0, seed, first."""
    wide = np.dtype(dtype).itemsize == 8
    rng = np.random.default_rng(3600 + 10 * D + wide + 1000 * salt)
    nu = (D - 1 + wide + salt) % 4 + 1
    nl = 3 + (2 * D + wide + salt) % 5
    n = [4] * D if D == 6 else [int(m) for m in rng.integers(4, 6, size=D)]
    knots = [np.sort(np.concatenate(([-1.0, 1.0], rng.uniform(-0.9, 0.9, size=m - 2)))) for m in n]
    ut = rng.uniform(-1.0, 1.0, size=(nl, nu))
    ut[nl - 1] = ut[(nl - 1) // 2]                                              # an exact tie: the lower label must win it
    A = 0.8 * np.eye(D) + rng.uniform(-0.15, 0.15, size=(D, D))
    B = rng.uniform(-0.3, 0.3, size=(D, nu))
    if nu > 1:
        B[int(rng.integers(0, D)), int(rng.integers(0, nu))] = 0.0
        B[D - 1, 0] = -0.0
    c = rng.uniform(-0.05, 0.05, size=D)
    q, r = rng.uniform(0.0, 1.0, size=D), rng.uniform(0.0, 0.3, size=nu)       # a cheap control: the value planes decide the label
    V = rng.uniform(0.0, 4.0, size=(int(np.prod(n)), 3)).astype(dtype)
    mode = "expect" if (D + wide + salt) % 2 else "worst"
    axes = [0, D - 1] if D >= 3 else [D - 1]
    E, P = control_table(rng, D, 3, nl, axes, with_weights=(mode == "expect"))
    E[:, :, 1] = 0.0                                                            # the all-zero candidate
    E[axes[0], 2, 1] = -0.0
    E[:, :, nl - 1] = E[:, :, (nl - 1) // 2]                                    # ... a tie under the table too
    eps, base, Pf = actuator_set(rng, D, nu)
    lo = np.array([k[0] for k in knots])
    hi = np.array([k[-1] for k in knots])
    X0 = rng.uniform(lo[:, None], hi[:, None], size=(D, N_TRAJ))
    for i in range(N_TRAJ // 3):                                                # grid nodes, the corners first
        X0[:, i] = [k[int(rng.integers(0, len(k)))] for k in knots]
    X0[:, 0], X0[:, 1] = lo, hi
    n_out = N_TRAJ // 3
    side = rng.integers(0, 2, size=(D, n_out))
    side[:, 0], side[:, 1] = 0, 1                                               # both sides on every axis
    X0[:, N_TRAJ - n_out:] = np.where(side == 0, lo[:, None] - rng.uniform(0.0, 0.2, size=(D, n_out)),
                                      hi[:, None] + rng.uniform(0.0, 0.2, size=(D, n_out)))
    return dict(model=dict(knots=knots, u_table=ut, A=A, B=B, J=V, c=c, q=q, r=r), E=E, P=P, mode=mode, eps=eps, base=base, Pf=Pf, X0=X0,
                seed=91 + D, first=2000 + 7 * D, nl=nl, nu=nu)


def labels_stub(knots, n_labels, base):
    """labels the lookahead never reads: one plane of the last label"""
    return np.full((int(np.prod([len(k) for k in knots])), 1), base + n_labels - 1, dtype=np.int32)


def control_table(rng, D, W, nl, axes, with_weights=True):
    """a seeded per-control set: offsets [D, W, nl] non-zero on `axes` only, with signed zeros among the entries and ONE all-zero
    candidate (label nl - 1; label 0 when there is one label is left alone), weights [W] positive, not summing to 1, or None"""
    E = np.zeros((D, W, nl))
    for a in axes:
        E[a] = rng.uniform(-0.3, 0.3, size=(W, nl))
    if axes:
        E[axes[0], 0, 0] = 0.0
        E[axes[-1], W - 1, 0] = -0.0
    if nl > 1:
        E[:, :, nl - 1] = 0.0
        if axes:
            E[axes[0], 0, nl - 1] = -0.0
    P = rng.uniform(0.1, 0.6, size=W) if with_weights else None
    return E, P


def actuator_set(rng, D, nu, W=3, with_base=True):
    """a seeded actuator set: eps [W, n_u] with input 0 live and (from two inputs on) the last input dead, a base on axis D // 2
    alone (or None), weights [W]"""
    eps = rng.uniform(-0.4, 0.4, size=(W, nu))
    eps[1, 0] = 0.0
    if nu > 1:
        eps[:, nu - 1] = 0.0
        eps[0, nu - 1] = -0.0
    base = None
    if with_base:
        base = np.zeros((D, W))
        base[D // 2] = rng.uniform(-0.1, 0.1, size=W)
    return eps, base, rng.uniform(0.2, 1.0, size=W)
