"""Plain numpy restatement of the noisy campaign's reduction (include/hjbdp.h, "noisy campaigns"), the checker of
tests/test_campaign_refs.py and tests/test_gpu_rollout_campaign.py.  It imports nothing of hjbdp.

  slot values   v0 = c, v1 = c * c, v2 = c, v3 = c, v7 = t ? c : +0.0; e = c > threshold[s] (strict), l = the `left` flag,
                t = |xf_a| <= tol_a on every axis; a padding slot holds v0 = v1 = v7 = +0.0, v2 = +inf, v3 = -inf, counts 0;
  blocks        G = min(64, smallest power of two >= M) consecutive samples of a start, the last block padded;
  tree          level by level on explicit slices: v = op(v[0::2], v[1::2]) - sums a + b, min b < a ? b : a, max b > a ? b : a;
  fold          acc = p_0, then acc = op(acc, p_b) in block order.
No np.sum, np.min or np.max touches a sample: every operation is one the contract names, in the order it names.
"""
from __future__ import annotations

import numpy as np

NSTAT = 8


def group(M):
    g = 1
    while g < 64 and g < M:
        g *= 2
    return g


def _add(a, b):
    return a + b


def _min(a, b):
    return np.where(b < a, b, a)


def _max(a, b):
    return np.where(b > a, b, a)


def _tree(v, op):
    """v [..., G] -> [...]: the adjacent-pair tree along the last axis"""
    while v.shape[-1] > 1:
        v = op(v[..., 0::2], v[..., 1::2])
    return v[..., 0]


def left_flags(X_path, knots):
    """[n] uint8: some visited state of X_path [n, D, K + 1] has an axis outside [first knot, last knot]; a NaN is outside"""
    X = np.asarray(X_path, dtype=np.float64)
    out = np.zeros(X.shape[0], dtype=bool)
    for a, k in enumerate(knots):
        k = np.asarray(k, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            inside = (k[0] <= X[:, a, :]) & (X[:, a, :] <= k[-1])
        out |= ~inside.all(axis=1)
    return out.astype(np.uint8)


def reduce(cost, M, X_final=None, left=None, threshold=None, tol=None):
    """cost [n_starts * M] (trajectory s * M + m is sample m of start s), X_final [D, n_starts * M], left [n_starts * M],
    threshold [n_starts], tol [D] -> stats [n_starts, 8]"""
    c = np.asarray(cost, dtype=np.float64).reshape(-1, M)
    ns = c.shape[0]
    G = group(M)
    B = -(-M // G)
    pad = B * G - M

    def blocks(x, fill):
        return np.concatenate([x, np.full((ns, pad), fill)], axis=1).reshape(ns, B, G)

    with np.errstate(invalid="ignore", over="ignore"):
        settled = np.zeros((ns, M), dtype=bool)
        if tol is not None:
            xf = np.asarray(X_final, dtype=np.float64).reshape(len(tol), ns, M)
            settled[:] = True
            for a in range(len(tol)):
                settled &= np.abs(xf[a]) <= float(tol[a])
        exceed = np.zeros((ns, M), dtype=bool) if threshold is None else c > np.asarray(threshold, dtype=np.float64).reshape(ns, 1)
        lf = np.zeros((ns, M), dtype=bool) if left is None else np.asarray(left).reshape(ns, M) != 0
        cols = [(blocks(c, 0.0), _add), (blocks(c * c, 0.0), _add), (blocks(c, np.inf), _min), (blocks(c, -np.inf), _max),
                (blocks(np.where(settled, c, 0.0), 0.0), _add)]
        out = np.empty((ns, NSTAT))
        for slot, (v, op) in zip((0, 1, 2, 3, 7), cols):
            p = _tree(v, op)                                    # [ns, B] block partials
            acc = p[:, 0]
            for b in range(1, B):
                acc = op(acc, p[:, b])
            out[:, slot] = acc
    for slot, flag in ((4, exceed), (5, lf), (6, settled)):
        out[:, slot] = np.count_nonzero(flag, axis=1)
    return out
