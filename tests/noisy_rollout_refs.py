"""Plain numpy restatement of hjb_rollout_run_noisy and its sampler (include/hjbdp.h), the checker of
tests/test_rollout_noisy_abi.py and tests/test_gpu_rollout_noisy.py.  It imports nothing of hjbdp's sampler.

  philox4x32_10   the generator in uint64 arithmetic (products of two 32-bit values fit 64 bits);
  thresholds      T[w] = floor(2^32 * (S_w / S_{W-1})), S_w summed left to right in double; null weights are 1.0 each;
  draw            node of (stream i, step k) = #{w in [0, W-2]: T[w] <= (double)word}, word = word k & 3 of
                  Philox((lo32 s, hi32 s, k >> 2, 0), (lo32 seed, hi32 seed)), s = first_stream + i (mod 2^64);
  rollout         tests/rollout_refs.py's loop with, after K16's update, x+_a = acc_a + d[a][w] on the axes of the offset mask
                  (those with an offset that is not +-0) and on no other axis.
"""
from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

# counter / key -> output (Random123's known-answer file, philox4x32 with 10 rounds)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit values, key: two 32-bit integers.  Returns the four output words as uint64
    arrays holding 32-bit values."""
    c = [np.asarray(x, dtype=np.uint64) & LO for x in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def words(seed, first_stream, n_traj, n_steps):
    """[n_traj, n_steps] uint64: the word step k of stream first_stream + i reads."""
    seed = int(seed) & (2 ** 64 - 1)
    s = (np.arange(n_traj, dtype=np.uint64) + np.uint64(int(first_stream) & (2 ** 64 - 1)))      # wraps mod 2^64
    out = np.zeros((n_traj, n_steps), dtype=np.uint64)
    for blk in range((n_steps + 3) // 4):
        r = philox4x32_10((s & LO, s >> S32, np.full(n_traj, blk, dtype=np.uint64), np.zeros(n_traj, dtype=np.uint64)),
                          (seed & 0xFFFFFFFF, seed >> 32))
        for j in range(4):
            if 4 * blk + j < n_steps:
                out[:, 4 * blk + j] = r[j]
    return out


def thresholds(weights, n_nodes=None):
    """[W - 1] float64.  weights None: n_nodes equal weights of 1.0."""
    p = np.ones(int(n_nodes)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    S = np.zeros(p.size)
    acc = 0.0
    for w in range(p.size):
        acc = acc + float(p[w])
        S[w] = acc
    return np.array([np.floor(4294967296.0 * (S[w] / S[-1])) for w in range(p.size - 1)], dtype=np.float64)


def nodes_of(T, word):
    """the count of thresholds <= (double)word, for an array of words"""
    x = np.asarray(word, dtype=np.uint64).astype(np.float64)
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    return (T.reshape((1,) * x.ndim + (-1,)) <= x[..., None]).sum(axis=-1).astype(np.int32)


def draw(T, seed, first_stream, n_traj, n_steps):
    """[n_traj, n_steps] int32 node indices"""
    return nodes_of(T, words(seed, first_stream, n_traj, n_steps))


def offset_mask(offsets):
    """the axes with at least one offset that is not +-0"""
    return [bool(np.any(row != 0.0)) for row in np.asarray(offsets, dtype=np.float64)]


def rollout(knots, labels, u_table, index_base, A, B, X0, plane_of_step, offsets, weights=None, seed=0, first_stream=0,
            method="linear", c=None, q=None, r=None, nodes=None):
    """tests/rollout_refs.py's rollout under the node set (offsets [D, W], weights [W] or None).  nodes [n, K]: a given node
    sequence instead of the drawn one (enumerations).  Returns X_final [D, n], cost [n], X_path [n, D, K+1], U_path [n, n_u, K],
    W_path [n, K] int32."""
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
    off = np.asarray(offsets, dtype=np.float64).reshape(D, -1)
    mask = offset_mask(off)
    x = np.array(np.asarray(X0, dtype=np.float64).reshape(D, -1))
    n = x.shape[1]
    planes = np.asarray(plane_of_step, dtype=np.int64).reshape(-1)
    K = planes.size
    if nodes is None:
        nodes = draw(thresholds(weights, off.shape[1]), seed, first_stream, n, K)
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
            if mask[a]:
                acc = acc + off[a, nodes[:, k]]
            xn[a] = acc
        x = xn
        U_path[:, :, k] = u.T
        X_path[:, :, k + 1] = x.T
    return x, cost, X_path, U_path, nodes.astype(np.int32)


# ---- the exactly posed lattice problem: promised against paid -------------------------------------------------------------------
# D = 1, knots -16 .. 16, controls {-1, 0, 1}, x+ = x + u + d, g = x^2 + 0.5 u^2, nodes d = (-1, 0, 1), 6 stages, terminal cost
# zero, starts -4 .. 4.  Every quantity is a dyadic rational and every reachable state a knot inside the grid until the terminal
# stage (|x_k| <= 4 + 2 k), so the disturbed backup's arithmetic (fma cascades on p = 1/4, 1/2, 1/4) is exact.
LATTICE_KNOTS = np.arange(-16.0, 17.0)
LATTICE_U = np.array([-1.0, 0.0, 1.0])
LATTICE_NODES = np.array([[-1.0, 0.0, 1.0]])
LATTICE_P = np.array([0.25, 0.5, 0.25])
LATTICE_STAGES = 6
LATTICE_STARTS = np.arange(-4.0, 5.0)


def lattice_spec(mode):
    """the hjbdp.ProblemSpec of the lattice problem with its disturbance ('expect': LATTICE_P; 'worst': no weights), float64"""
    from hjbdp import ProblemSpec, Term
    k, u = LATTICE_KNOTS, LATTICE_U
    return ProblemSpec([k], [3], [[Term((0,), k), Term((1,), u)]], [Term((0,), k * k), Term((1,), 0.5 * u * u)], dtype=np.float64,
                       index_base=0, disturbance=(LATTICE_NODES, LATTICE_P if mode == "expect" else None, mode))


def lattice_enumeration(labels):
    """Every one of the 3^6 node sequences flown from every start under the policy `labels` [33, 6] (plane k = step k, 0-based)
    with the restatement: (costs [9, 729], probability [729] of each sequence under LATTICE_P)."""
    import itertools
    seqs = np.array(list(itertools.product(range(3), repeat=LATTICE_STAGES)), dtype=np.int32)           # [729, 6]
    prob = np.prod(LATTICE_P[seqs], axis=1)
    n_seq, n_st = seqs.shape[0], LATTICE_STARTS.size
    X0 = np.repeat(LATTICE_STARTS, n_seq).reshape(1, -1)
    out = rollout([LATTICE_KNOTS], labels, LATTICE_U, 0, [[1.0]], [[1.0]], X0, np.arange(LATTICE_STAGES), LATTICE_NODES,
                  q=[1.0], r=[0.5], nodes=np.tile(seqs, (n_st, 1)))
    return out[1].reshape(n_st, n_seq), prob
