"""Plain numpy restatement of hjb_rollout_run_actuator (include/hjbdp.h), the checker of tests/test_actuator_rollout_refs.py,
tests/test_gpu_rollout_actuator.py and tests/test_gpu_rollout_actuator_campaign.py.  tests/noisy_rollout_refs.py's rollout with the
contract's steps 1 - 4 in the place of the offset add; the Philox generator, the thresholds and the draw are that file's.  It
imports nothing of hjbdp's sampler.

  live inputs   input j is live iff some eps[j][w] is not +-0;  ue_j = u_j * eps[j][w], one rounded product per step;
  terms of a    for live j ascending with B[a,j] not +-0: B[a,j] * ue_j (rounded); then base[a][w] if row a of base has an entry
                that is not +-0;
  update        no term: x+_a = acc_a (not touched);  otherwise n_a = the first term, n_a = n_a + term left to right,
                x+_a = acc_a + n_a.
"""
from __future__ import annotations

import itertools
from fractions import Fraction

import numpy as np

from noisy_rollout_refs import draw, thresholds


def eps_matrix(eps, nu):
    """eps as [n_u, W]: [W] (one error for every input) or [W, n_u], the shapes hjbdp.actuator_nodes takes"""
    e = np.asarray(eps, dtype=np.float64)
    if e.ndim == 1:
        e = np.repeat(e[:, None], nu, axis=1)
    assert e.ndim == 2 and e.shape[1] == nu
    return np.ascontiguousarray(e.T)


def rollout(knots, labels, u_table, index_base, A, B, X0, plane_of_step, eps, weights=None, base=None, seed=0, first_stream=0,
            method="linear", c=None, q=None, r=None, nodes=None):
    """tests/rollout_refs.py's rollout under the actuator node set (eps [W] or [W, n_u], weights [W] or None, base [D, W] or
    None).  nodes [n, K]: a given node sequence instead of the drawn one (enumerations).  Returns X_final [D, n], cost [n], X_path
    [n, D, K+1], U_path [n, n_u, K] (the commanded u), W_path [n, K] int32."""
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
    e = eps_matrix(eps, nu)                                                     # [n_u, W]
    W = e.shape[1]
    live = [bool(np.any(e[j] != 0.0)) for j in range(nu)]
    bs = None if base is None else np.asarray(base, dtype=np.float64).reshape(D, W)
    base_axis = [bs is not None and bool(np.any(bs[a] != 0.0)) for a in range(D)]
    x = np.array(np.asarray(X0, dtype=np.float64).reshape(D, -1))
    n = x.shape[1]
    planes = np.asarray(plane_of_step, dtype=np.int64).reshape(-1)
    K = planes.size
    if nodes is None:
        nodes = draw(thresholds(weights, W), seed, first_stream, n, K)
    nodes = np.asarray(nodes).reshape(n, K)
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
            g = g + r[j] * (u[j] * u[j])                                        # on the COMMANDED u
        cost = cost + g
        w = nodes[:, k]
        ue = {j: u[j] * e[j, w] for j in range(nu) if live[j]}                  # step 1
        xn = np.empty_like(x)
        for a in range(D):
            acc = A[a, 0] * x[0]
            for b in range(1, D):
                acc = acc + A[a, b] * x[b]
            for j in range(nu):
                acc = acc + B[a, j] * u[j]
            if c is not None:
                acc = acc + float(np.asarray(c, dtype=np.float64).reshape(D)[a])
            terms = [B[a, j] * ue[j] for j in range(nu) if live[j] and B[a, j] != 0.0]      # step 2
            if base_axis[a]:
                terms.append(bs[a, w])
            if terms:                                                           # steps 3 and 4
                na = terms[0]
                for t in terms[1:]:
                    na = na + t
                acc = acc + na
            xn[a] = acc
        x = xn
        U_path[:, :, k] = u.T
        X_path[:, :, k + 1] = x.T
    return x, cost, X_path, U_path, nodes.astype(np.int32)


# ---- the exactly posed lattice problem: promised against paid -------------------------------------------------------------------
# D = 1, knots -16 .. 16, controls {-4, -2, 0, 2, 4}, x+ = x + u (1 + eps), eps = (-1/2, 0, 1/2) with p = (1/4, 1/2, 1/4),
# g = x^2 + u^2 / 8, 6 stages, terminal cost zero, starts -4 .. 4.  u eps is an integer, so every state is a knot or an integer
# beyond the grid (unit spacing: the extrapolation weight is an integer), every cost a multiple of 1/2 and every weighted sum a
# dyadic rational far inside double: the backup's and the flight's arithmetic is exact.
LATTICE_KNOTS = np.arange(-16.0, 17.0)
LATTICE_U = np.array([-4.0, -2.0, 0.0, 2.0, 4.0])
LATTICE_EPS = np.array([-0.5, 0.0, 0.5])
LATTICE_P = np.array([0.25, 0.5, 0.25])
LATTICE_STAGES = 6
LATTICE_STARTS = np.arange(-4.0, 5.0)
LATTICE_R = 0.125


def lattice_spec(mode, nominal=False):
    """the hjbdp.ProblemSpec of the lattice problem under its actuator noise ('expect': LATTICE_P; 'worst': no weights), float64;
    nominal: the same problem with no disturbance"""
    from hjbdp import ProblemSpec, Term, actuator_nodes
    k, u = LATTICE_KNOTS, LATTICE_U
    cd = None
    if not nominal:
        off, _ = actuator_nodes([[1.0]], u, LATTICE_EPS)
        cd = (off, LATTICE_P if mode == "expect" else None, mode)
    return ProblemSpec([k], [u.size], [[Term((0,), k), Term((1,), u)]], [Term((0,), k * k), Term((1,), LATTICE_R * u * u)],
                       dtype=np.float64, index_base=0, control_disturbance=cd)


def lattice_sequences():
    """([729, 6] int32 node sequences, [729] the probability of each under LATTICE_P)"""
    seqs = np.array(list(itertools.product(range(3), repeat=LATTICE_STAGES)), dtype=np.int32)
    return seqs, np.prod(LATTICE_P[seqs], axis=1)


def lattice_enumeration(labels):
    """Every one of the 3^6 node sequences flown from every start under the policy `labels` [33, 6] (plane k = step k, 0-based)
    with the restatement: (costs [9, 729], probability [729] of each sequence under LATTICE_P, X_path [9, 729, 7])."""
    seqs, prob = lattice_sequences()
    n_seq, n_st = seqs.shape[0], LATTICE_STARTS.size
    X0 = np.repeat(LATTICE_STARTS, n_seq).reshape(1, -1)
    out = rollout([LATTICE_KNOTS], labels, LATTICE_U, 0, [[1.0]], [[1.0]], X0, np.arange(LATTICE_STAGES), LATTICE_EPS,
                  q=[1.0], r=[LATTICE_R], nodes=np.tile(seqs, (n_st, 1)))
    return out[1].reshape(n_st, n_seq), prob, out[2][:, 0, :].reshape(n_st, n_seq, LATTICE_STAGES + 1)


def lattice_exact(mode, nominal=False):
    """The lattice problem's sweep in exact rationals (fractions.Fraction), by the backup's rules: the query x + u (1 + eps_w),
    the cell clamp(upper_bound - 1, 0, n - 2) with an unclamped weight (linear extrapolation), E_w with LATTICE_P or max_w, the
    first minimum.  nominal: one node eps = 0.  -> (J [6][33] Fractions, labels [6][33]), first = the stage computed first."""
    k = [Fraction(int(v)) for v in LATTICE_KNOTS]
    us = [Fraction(int(v)) for v in LATTICE_U]
    es = [Fraction(0)] if nominal else [Fraction(-1, 2), Fraction(0), Fraction(1, 2)]
    ps = [Fraction(1)] if nominal else [Fraction(1, 4), Fraction(1, 2), Fraction(1, 4)]
    n = len(k)

    def interp(J, qx):
        i = min(max(sum(1 for v in k if v <= qx) - 1, 0), n - 2)
        t = (qx - k[i]) / (k[i + 1] - k[i])
        return J[i] + t * (J[i + 1] - J[i])

    J = [Fraction(0)] * n
    out = []
    for _ in range(LATTICE_STAGES):
        Jn, lab = [], []
        for x in k:
            best, best_l = None, 0
            for l, u in enumerate(us):
                vals = [interp(J, x + u * (1 + e)) for e in es]
                acc = sum(p * v for p, v in zip(ps, vals)) if mode == "expect" else max(vals)
                cand = x * x + Fraction(1, 8) * u * u + acc
                if best is None or cand < best:
                    best, best_l = cand, l
            Jn.append(best)
            lab.append(best_l)
        J = Jn
        out.append((Jn, lab))
    return out
