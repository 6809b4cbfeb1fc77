"""Plain numpy restatement of hjb_rollout_run_greedy (include/hjbdp.h), the checker of tests/test_rollout_greedy_abi.py and
tests/test_gpu_rollout_greedy.py.  It imports nothing of hjbdp's greedy code.

Per step the candidates are formed for all trajectories at once, label by label in the library's stated order, one IEEE
operation at a time:
    gs = (q0*(x0*x0) + q1*(x1*x1)) + ...;   as_a = (A[a,0]*x0 + A[a,1]*x1) + ...          once
    g_l = gs + r0*(u0*u0) + ...;   xn_a = as_a + B[a,0]*u0 + ... (+ c_a);   v_l = blend of the plane at xn;   cand_l = g_l + v_l
    best = cand_0; l >= 1 replaces iff cand_l < best
The blend is the oracle's C twin (oracle.c_oracle.lookup 'linear' in float64: bit-exact with k_policy_lookup, cell clamped to
[0, n - 2]) on the plane widened to float64.  The chosen label's g and xn are the arrays step 3 formed, picked by index.

It also holds the two exactly posed lattice problems of the closed-loop tests.
"""
from __future__ import annotations

import numpy as np


def rollout(knots, u_table, A, B, values, X0, plane_of_step, c=None, q=None, r=None, index_base=0):
    """knots: D grid vectors; u_table [n_labels, n_u]; values: nS x n_planes (column-major, any shape; float32 or float64) or
    None; X0 [D, n]; plane_of_step: plane indices, -1 = the zero function.
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
            v = np.zeros(n) if p < 0 else c_oracle.lookup(_abi, ks, V[:, p], np.ascontiguousarray(XN[l].T), "linear")
            cand = g + v
            if l == 0:
                best[:] = cand
            else:
                take = cand < best
                best[take] = cand[take]
                lab[take] = l
        cost = cost + G[lab, cols]
        x = np.ascontiguousarray(XN[lab, :, cols].T)
        U_path[:, :, k] = ut[lab]
        L_path[:, k] = lab + index_base
        V_path[:, k] = best
        X_path[:, :, k + 1] = x.T
    return x, cost, X_path, U_path, L_path, V_path


def random_problem(rng, D, nu, n_labels, n_planes, dtype, duplicate_rows=True):
    """A seeded problem on a small grid: 3-5 knots per axis, one axis non-uniform; a contraction-like A so that flights stay near
    the grid; u_table with (from 2 labels on) one row repeated, the exact tie the lower label must win.
    Returns knots, u_table, A, B, c, q, r, values [nS, n_planes] in dtype."""
    n = rng.integers(3, 6, size=D)
    knots = [np.linspace(-1.0, 1.0, int(m)) for m in n]
    a_nu = int(rng.integers(0, D))
    knots[a_nu] = np.sort(np.concatenate(([-1.0, 1.0], rng.uniform(-0.9, 0.9, size=int(n[a_nu]) - 2))))
    ut = rng.uniform(-1.0, 1.0, size=(n_labels, nu))
    if duplicate_rows and n_labels >= 2:
        ut[n_labels - 1] = ut[(n_labels - 1) // 2]
    A = 0.8 * np.eye(D) + rng.uniform(-0.15, 0.15, size=(D, D))
    B = rng.uniform(-0.3, 0.3, size=(D, nu))
    c = rng.uniform(-0.05, 0.05, size=D)
    q = rng.uniform(0.0, 1.0, size=D)
    r = rng.uniform(0.0, 1.0, size=nu)
    nS = int(np.prod(n))
    values = rng.uniform(0.0, 2.0, size=(nS, n_planes)).astype(dtype)
    return knots, ut, A, B, c, q, r, values


def starts(rng, knots, n):
    """[D, n] starts: the first on grid nodes (the corners included), a third outside the grid by up to 0.2, the rest inside."""
    D = len(knots)
    lo = np.array([k[0] for k in knots])
    hi = np.array([k[-1] for k in knots])
    X = rng.uniform(lo[:, None], hi[:, None], size=(D, n))
    n_node = max(1, n // 3)
    for i in range(n_node):
        X[:, i] = [k[int(rng.integers(0, len(k)))] for k in knots]
    X[:, 0] = lo
    if n > 1:
        X[:, 1] = hi
    n_out = n // 3
    if n_out:
        side = rng.integers(0, 2, size=(D, n_out))
        X[:, n - n_out:] = np.where(side == 0, lo[:, None] - rng.uniform(0.0, 0.2, size=(D, n_out)),
                                    hi[:, None] + rng.uniform(0.0, 0.2, size=(D, n_out)))
    return X


# ---- the exactly posed lattice problems: every quantity an integer or a half in double --------------------------------------------
# 1-D: knots -16 .. 16, u in {-1, 0, 1}, x+ = x + u, g = x^2 + u^2 / 2, 6 stages, zero terminal, starts -4 .. 4.
LATTICE_KNOTS = np.arange(-16.0, 17.0)
LATTICE_U = np.array([-1.0, 0.0, 1.0])
LATTICE1 = dict(knots=[LATTICE_KNOTS], A=[[1.0]], B=[[1.0]], q=[1.0], r=[0.5], stages=6,
                starts=np.arange(-4.0, 5.0).reshape(1, -1))
# 2-D integer double integrator: x1+ = x1 + x2, x2+ = x2 + u, g = x1^2 + x2^2 + u^2 / 2, 4 stages, starts |x1| <= 2, |x2| <= 1.
# |x2| grows by at most 1 a step and |x1| by |x2|: every path stays within |x1| <= 12, |x2| <= 5, inside the grid.
LATTICE2 = dict(knots=[LATTICE_KNOTS, LATTICE_KNOTS], A=[[1.0, 1.0], [0.0, 1.0]], B=[[0.0], [1.0]], q=[1.0, 1.0], r=[0.5], stages=4,
                starts=np.array([[x1, x2] for x1 in range(-2, 3) for x2 in range(-1, 2)], dtype=np.float64).T)


def lattice_spec(D):
    """the hjbdp.ProblemSpec of the D-dimensional lattice problem (float64, 0-based labels), its terms in K16's order"""
    from hjbdp import ProblemSpec, Term
    k, u = LATTICE_KNOTS, LATTICE_U
    if D == 1:
        return ProblemSpec([k], [3], [[Term((0,), k), Term((1,), u)]], [Term((0,), k * k), Term((1,), 0.5 * (u * u))], dtype=np.float64,
                           index_base=0)
    return ProblemSpec([k, k], [3], [[Term((0,), k), Term((1,), k), Term((2,), 0.0 * u)], [Term((0,), 0.0 * k), Term((1,), k), Term((2,), u)]],
                       [Term((0,), k * k), Term((1,), k * k), Term((2,), 0.5 * (u * u))], dtype=np.float64, index_base=0)
