"""References for the fixed-label stage (hjb_evaluate*): J(x) = g(x, u(x)) + F(x_next(x, u(x))) for given labels.

evaluate_ref gathers, per state, the candidate value of the state's own label from the numpy oracle's quantities (oracle.hjb_oracle:
Problem._sum, cell_and_weight, interp_linear).  Two lerp forms:

  lerp="oracle"  interp_linear itself: v0 + t * (v1 - v0), product and sum rounded separately.  Fed hjb_oracle.backup_stage's labels
                 it reproduces that oracle's J bit for bit.
  lerp="fma"     the canonical form of the C twin and of every stage kernel: fma(t, v1 - v0, v0), ONE rounding, computed exactly
                 (float32: in float64 with the double rounding repaired from the sum's exact residual; float64: in rationals).
                 Everything else - ordered term sums, cell search, weight, corner order, the cost sum, g + v - is the oracle's
                 own.  Fed the C twin's labels it reproduces the C twin's J bit for bit (tests/test_evaluate_abi.py), which is what
                 makes it the bit-exact reference for arbitrary labels on the GPU: the two oracles differ by a few ulp exactly
                 because of this one rounding (tests/test_oracle_golden.py).

evaluate_ref forms whole-grid arrays; evaluate_ref_states is the same canonical form for a list of states, with J_next behind a
callable (grids too large for the host: tests/test_gpu_evaluate_forms.py).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from oracle import hjb_oracle


def oracle_problem(spec):
    """The numpy oracle's view of a ProblemSpec (default typings: no table_dtype / cost_dtype)."""
    assert spec.table_dtype is None and spec.cost_dtype is None and spec.model is None
    return hjb_oracle.Problem(spec.knots, spec.m, [[hjb_oracle.Term(t.dims, t.data) for t in ts] for ts in spec.next_terms],
                              [hjb_oracle.Term(t.dims, t.data) for t in spec.cost_terms], spec.dtype)


def _fma32(t, d, v0):
    """float32 fma(t, d, v0), exactly: the product of two float32 is exact in float64; the float64 sum's residual (TwoSum) decides
    the one case a second rounding could go wrong - a float64 sum that sits exactly on a float32 midpoint."""
    p = t.astype(np.float64) * d.astype(np.float64)
    c = v0.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                      # s + err == p + c exactly
    f = s.astype(np.float32)
    away = np.where(f.astype(np.float64) < s, np.float32(np.inf), np.float32(-np.inf))
    other = np.nextafter(f, away)                        # the float32 neighbour on s's side
    with np.errstate(invalid="ignore", over="ignore"):
        mid = (f.astype(np.float64) + other.astype(np.float64)) * 0.5 == s
    mid &= (f.astype(np.float64) != s) & (err != 0) & np.isfinite(s)
    up = np.maximum(f, other)
    dn = np.minimum(f, other)
    return np.where(mid, np.where(err > 0, up, dn), f).astype(np.float32)


def _fma64(t, d, v0):
    out = np.empty(t.shape, dtype=np.float64)
    tf, df, vf, of = t.reshape(-1), d.reshape(-1), v0.reshape(-1), out.reshape(-1)
    for i in range(tf.size):
        of[i] = float(Fraction(float(tf[i])) * Fraction(float(df[i])) + Fraction(float(vf[i])))      # int / int: correctly rounded
    return out


def evaluate_ref(p, J_next, labels, lerp="oracle"):
    """p: hjb_oracle.Problem; J_next: p.n values (any layout reshapeable column-major); labels: one 0-based flat control label per
    state (column-major over the control dims, first control dim fastest - what backup_stage returns), any integer dtype.
    -> J [p.n] in p.dtype."""
    dt = p.dtype
    J_next = np.asarray(J_next, dtype=dt)
    J_next = J_next.reshape(p.n, order="F") if J_next.ndim == 1 else J_next.reshape(p.n)
    lab = np.asarray(labels).astype(np.int64)
    lab = lab.reshape(p.n, order="F") if lab.ndim == 1 else lab.reshape(p.n)
    assert lab.min() >= 0 and lab.max() < p.nU
    sub = np.unravel_index(lab, p.m, order="F")                      # (i1, .., iC), control dim 0 fastest
    full = p.n + p.m
    q = [np.broadcast_to(p._sum(p.next_terms[a]), full) for a in range(p.D)]
    g = np.broadcast_to(p._sum(p.cost_terms), full)
    states = np.indices(p.n, sparse=True)
    at = tuple(np.broadcast_to(s, p.n) for s in states) + tuple(sub)
    if lerp == "oracle":
        Jf = hjb_oracle.interp_linear(p.knots, J_next, q)
        tot = (g + Jf).astype(dt, copy=False)
        return tot[at]
    assert lerp == "fma"
    fma = _fma32 if dt == np.float32 else _fma64
    cells, ts = [], []
    for a in range(p.D):
        i, t = hjb_oracle.cell_and_weight(p.knots[a], q[a][at])
        cells.append(i)
        ts.append(t)
    vals = [J_next[tuple(cells[a] + ((corner >> a) & 1) for a in range(p.D))] for corner in range(1 << p.D)]
    for a in range(p.D):                                             # axis 0 first, as interp_linear
        vals = [fma(ts[a], (vals[j + 1] - vals[j]).astype(dt, copy=False), vals[j]) for j in range(0, len(vals), 2)]
    return (g[at] + vals[0]).astype(dt, copy=False)


def evaluate_ref_states(p, states, labels_at_states, jnext_at):
    """evaluate_ref's canonical (fma) form for a LIST of states - nothing of the grid's size is formed, so it serves grids of 10^7
    .. 10^10 states.  states: flat whole-grid state indices (column-major, axis 0 fastest); labels_at_states: the 0-based flat
    control label of each listed state; jnext_at(idx): J_next, in p.dtype, at the tuple idx of D integer index arrays (an array
    lookup for a J the host holds, the ordered float32 sum of float64_refs.ordered_sum for fill_separable's terminal cost).
    -> J [len(states)] in p.dtype.  Same arithmetic as evaluate_ref(lerp="fma"): ordered term sums, cell_and_weight, the 2^D corners
    lerped axis 0 first with the exact fma, then g + v (tests/test_evaluate_abi.py holds the two equal, and this one to the C twin)."""
    dt = p.dtype
    states = np.asarray(states, dtype=np.int64)
    lab = np.asarray(labels_at_states).astype(np.int64)
    assert states.shape == lab.shape and states.ndim == 1
    assert states.min() >= 0 and states.max() < int(np.prod([int(x) for x in p.n], dtype=object))
    assert lab.min() >= 0 and lab.max() < p.nU
    at = tuple(np.unravel_index(states, p.n, order="F")) + tuple(np.unravel_index(lab, p.m, order="F"))

    def osum(terms):                                                 # Problem._sum at the listed (state, control) pairs
        acc = None
        for t in terms:
            x = np.broadcast_to(t.data[tuple(at[d] for d in t.dims)], states.shape)
            acc = x if acc is None else (acc + x).astype(dt, copy=False)
        return acc
    fma = _fma32 if dt == np.float32 else _fma64
    cells, ts = [], []
    for a in range(p.D):
        i, t = hjb_oracle.cell_and_weight(p.knots[a], osum(p.next_terms[a]))
        cells.append(i)
        ts.append(t)
    vals = [np.asarray(jnext_at(tuple(cells[a] + ((corner >> a) & 1) for a in range(p.D))), dtype=dt) for corner in range(1 << p.D)]
    for a in range(p.D):                                             # axis 0 first, as interp_linear
        vals = [fma(ts[a], (vals[j + 1] - vals[j]).astype(dt, copy=False), vals[j]) for j in range(0, len(vals), 2)]
    return (osum(p.cost_terms) + vals[0]).astype(dt, copy=False)


def separable_jnext(vecs, dtype, storage):
    """jnext_at for fill_separable's terminal cost: ((v0[i0] + v1[i1]) + ...) in `dtype`, rounded once to `storage` (what the
    device buffer holds) and widened back to `dtype` (what the kernels read)."""
    from float64_refs import ordered_sum
    vs = [np.asarray(v, dtype=dtype) for v in vecs]
    return lambda idx: ordered_sum([v[i] for v, i in zip(vs, idx)], dtype).astype(storage).astype(dtype)
