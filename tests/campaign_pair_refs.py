"""Plain numpy restatement of the paired campaign's difference record (include/hjbdp.h, "paired campaigns"), the checker of
tests/test_campaign_pair_refs.py and tests/test_gpu_rollout_campaign_pair.py.  Written from the contract, not from
csrc/hjbdp_campaign.h; it imports nothing of hjbdp.

  sample        d = c_B - c_A, one rounded subtraction; e = d < 0, l = d > 0 (a NaN d sets neither), t = neither flight left;
  slot values   v0 = d, v1 = d * d (rounded), v2 = d, v3 = d, v7 = t ? d : +0.0;
                a padding slot holds v0 = v1 = v7 = +0.0, v2 = +inf, v3 = -inf and counts 0;
  blocks        G = min(64, smallest power of two >= M) consecutive samples of a start, the last block padded;
  tree          at level L element i (a multiple of 2^(L+1)) becomes op(v[i], v[i + 2^L]):
                sums a + b, min b < a ? b : a, max b > a ? b : a, `a` the earlier operand;
  fold          acc = p_0, then acc = op(acc, p_b) in block order.
One scalar IEEE double operation at a time, in the order the contract names them.
"""
from __future__ import annotations

import numpy as np

NSTAT = 8
F = np.float64


def group(M):
    g = 1
    while g < 64 and g < M:
        g *= 2
    return g


def _op(a, b):
    """a the earlier operand; the five doubles (sum, sumsq, min, max, sum over both-in)"""
    return (a[0] + b[0], a[1] + b[1], b[2] if b[2] < a[2] else a[2], b[3] if b[3] > a[3] else a[3], a[4] + b[4])


def _block(v):
    """the adjacent-pair tree over the G slots of one block, level by level, in place on a list"""
    G, half = len(v), 1
    while half < G:
        for i in range(0, G, 2 * half):
            v[i] = _op(v[i], v[i + half])
        half *= 2
    return v[0]


def pair_reduce(cost_a, cost_b, M, left_a=None, left_b=None):
    """cost_a, cost_b [n_starts * M] (trajectory s * M + m is sample m of start s), left_a, left_b [n_starts * M] or None ->
    stats_d [n_starts, 8]"""
    ca = np.asarray(cost_a, dtype=F).reshape(-1, M)
    cb = np.asarray(cost_b, dtype=F).reshape(-1, M)
    ns = ca.shape[0]
    la = np.zeros((ns, M), dtype=bool) if left_a is None else np.asarray(left_a).reshape(ns, M) != 0
    lb = np.zeros((ns, M), dtype=bool) if left_b is None else np.asarray(left_b).reshape(ns, M) != 0
    G = group(M)
    pad = (F(0.0), F(0.0), F(np.inf), F(-np.inf), F(0.0))
    out = np.empty((ns, NSTAT))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(ns):
            n_b = n_a = n_in = 0
            acc = None
            for m0 in range(0, M, G):
                v = []
                for m in range(m0, m0 + G):
                    if m >= M:
                        v.append(pad)
                        continue
                    d = F(cb[s, m]) - F(ca[s, m])
                    t = not la[s, m] and not lb[s, m]
                    n_b += bool(d < 0)
                    n_a += bool(d > 0)
                    n_in += t
                    v.append((d, d * d, d, d, d if t else F(0.0)))
                p = _block(v)
                acc = p if acc is None else _op(acc, p)
            out[s] = (acc[0], acc[1], acc[2], acc[3], n_b, n_a, n_in, acc[4])
    return out


def swap_of(stats_d):
    """what the record of the swapped pair must equal AS VALUES: sums negated, min and max swapped and negated, the sign counts
    swapped, sum of squares and the both-in count kept"""
    s = np.asarray(stats_d, dtype=F)
    out = s.copy()
    out[:, 0], out[:, 7] = -s[:, 0], -s[:, 7]
    out[:, 2], out[:, 3] = -s[:, 3], -s[:, 2]
    out[:, 4], out[:, 5] = s[:, 5], s[:, 4]
    return out


def same_values(x, y):
    """equal as values (+0.0 == -0.0), NaNs in the same places"""
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    return x.shape == y.shape and bool(np.all((x == y) | (np.isnan(x) & np.isnan(y))))


def same_bits(x, y):
    """equal bit for bit; a NaN equals a NaN (IEEE 754 leaves the sign and the payload of an operation's NaN to the machine)"""
    x, y = np.ascontiguousarray(x, dtype=F), np.ascontiguousarray(y, dtype=F)
    if x.shape != y.shape:
        return False
    nx, ny = np.isnan(x), np.isnan(y)
    return bool(np.array_equal(nx, ny) and np.array_equal(x.view(np.uint64)[~nx], y.view(np.uint64)[~ny]))


def harness_inputs(s, M):
    """the inputs of start s of tests/campaign_pair_harness.cpp, exactly representable; both build the same numbers"""
    m = np.arange(M)
    ca = ((m * 37 + s * 11) % 101) / 8.0 - 3.0
    cb = ((m * 29 + s * 5) % 103) / 8.0 - 3.0
    cb = np.where(m % 5 == 0, ca, cb)                                           # exact ties
    la = (m * 5 + s) % 7 == 0
    lb = (m * 3 + s) % 11 == 0
    return ca, cb, la.astype(np.uint8), lb.astype(np.uint8)
