"""Lattice problems whose Bellman backup is EXACT, an exact-arithmetic reference of it, and the input conditions that make a
problem a test of the stage kernels' argmin.  The reference, the counts and the conditions are numpy only; the ONE thing taken from
the package is the pair of plain Python records hjbdp.ProblemSpec / hjbdp.Term (hjbdp/problem.py: no native call), imported
lazily by the generators because a ProblemSpec is what they must return - nothing here loads libhjbdp or the C twin.

On a grid whose knots are integers times a power of two, with next-state terms that are whole cells (or halves / eighths of one),
integer costs and an integer terminal cost, every quantity of the canonical arithmetic is a dyadic
rational with a short significand: each term sum, weight, difference v1 - v0, partial lerp, total and stored J is representable
in the type it is formed in, so NO operation rounds and the order of operations cannot matter.  tie_reference computes the sweep
in int64 fixed point (units of 2^-F) and ASSERTS that representability per operation - in the arithmetic type, the storage type
(binary16 included) and the query type - so the stage counts used are the ones that stay exact, by the reference's own check.

Small integers tie often: g_a + v_a == g_b + v_b with g_a != g_b, v read from different cells.  tie_counts / assert_ties state per
registered case which kinds of tie occur (TIE_CASES; seeds are literals found by search on the CPU, conditions are assertions:
a change to a generator cannot hollow a GPU case out unnoticed - the rule tests/problems.py's placement_case follows)."""
from __future__ import annotations

import numpy as np

F = 24                     # fixed point: values in units of 2^-F
FW = 4                     # weights (and node probabilities) in units of 2^-FW: eighths of a cell are the finest move
_FMT = {np.dtype(np.float16): (11, -24, 65504.0), np.dtype(np.float32): (24, -149, 3.4e38), np.dtype(np.float64): (53, -1074, 1.7e308)}
STEPS = (-2, -1, 0, 1, 2)


# ---- exactness ------------------------------------------------------------------------------------------------------------------
def fits(x, frac, dtype):
    """Every x * 2^-frac (x int64) is a value of `dtype`: odd part below 2^p, lowest bit not under the smallest subnormal, magnitude
    within the largest finite value."""
    p, emin, big = _FMT[np.dtype(dtype)]
    x = np.asarray(x, dtype=np.int64)
    ax = np.abs(x)
    low = np.where(ax == 0, 1, ax & -ax)
    ok = (ax // low) < (1 << p)
    if frac + emin > 0:
        ok &= (ax == 0) | (low >= (1 << (frac + emin)))
    if big < 2.0 ** (62 - frac):
        ok &= ax <= int(big * 2.0 ** frac)
    return bool(np.all(ok))


def to_fixed(x, what=""):
    """float values -> int64 in units of 2^-F; asserts that nothing is lost."""
    y = np.asarray(x, dtype=np.float64) * float(1 << F)
    r = np.rint(y)
    assert np.array_equal(r, y) and np.all(np.abs(r) < 2.0 ** 60), ("not on the 2^-%d lattice" % F, what)
    return r.astype(np.int64)


def from_fixed(x, dtype):
    assert fits(x, F, dtype), "a stored value is not representable in %s" % np.dtype(dtype).name
    return (np.asarray(x, dtype=np.int64).astype(np.float64) / float(1 << F)).astype(dtype)


def visiting_labels(m, index_base=0):
    """label[u] of visiting index u (control dim 0 SLOWEST, the last one fastest): the column-major index + index_base."""
    cj = np.unravel_index(np.arange(int(np.prod(m))), tuple(m), order="C")
    return np.ravel_multi_index(cj, tuple(m), order="F") + index_base


def _grid_shape(t, g):
    return [g[d] if d in t.dims else 1 for d in range(len(g))]


def _ordered_sum(terms, g, dtypes, what):
    """Exact sum of broadcast terms (shape: singleton where no term varies); every term and every partial sum must be a value of
    each of `dtypes`."""
    acc = None
    for k, t in enumerate(terms):
        x = to_fixed(t.data, (what, k)).reshape(_grid_shape(t, g))
        acc = x if acc is None else acc + x
        for dt in dtypes:
            assert fits(x, F, dt) and fits(acc, F, dt), (what, k, np.dtype(dt).name)
    return acc


def _at_control(arr, D, cj):
    """arr (broadcast shape over n + m) at per-dim control indices cj -> shape over the state dims (singletons kept)."""
    return arr[(slice(None),) * D + tuple(cj[c] if arr.shape[D + c] > 1 else 0 for c in range(len(cj)))]


class _Located:
    """Cells and weights of every axis' query (optionally moved by a disturbance node's offset), exact."""

    def __init__(self, spec, offsets=None):
        n, m, D = spec.n, spec.m, spec.D
        g = n + m
        T = np.dtype(spec.dtype)
        TQ = np.dtype(spec.table_dtype or spec.dtype)
        W = 1 if offsets is None else offsets.shape[1]
        self.cells, self.ws = [[] for _ in range(W)], [[] for _ in range(W)]
        self.weights_seen = set()
        for a in range(D):
            q0 = _ordered_sum(spec.next_terms[a], g, (TQ,), ("next", a))
            k = to_fixed(spec.knots[a], ("knots", a))
            assert fits(k, F, TQ) and fits(k, F, T)
            dx = np.diff(k)
            assert np.all(dx > 0) and np.all(dx & (dx - 1) == 0), ("spacings must be powers of two: 1 / dx exact", a)
            for w in range(W):
                q = q0
                if offsets is not None and np.any(offsets[a] != 0):
                    q = q0 + to_fixed(offsets[a, w], ("offset", a, w))
                    assert fits(q, F, TQ)
                c = np.clip(np.searchsorted(k, q, side="right") - 1, 0, n[a] - 2)
                d = q - k[c]
                assert fits(d, F, TQ), ("q - k[c]", a)
                num = d << FW
                assert np.all(num % dx[c] == 0), ("weight finer than 2^-%d" % FW, a)
                wt = num // dx[c]
                assert fits(wt, FW, TQ) and fits(wt, FW, T), ("weight", a)
                self.cells[w].append(c)
                self.ws[w].append(wt)
                self.weights_seen.update(np.unique(wt).tolist())


def _lerp(Jg, cc, ww, D, T):
    """N-linear interpolation, axis 0 folded first; every difference and every partial result must be a value of T."""
    corner = np.arange(1 << D).reshape((-1,) + (1,) * D)
    vals = Jg[tuple(cc[a][None] + ((corner >> a) & 1) for a in range(D))]          # [2^D, n...]: bit a of the corner = axis a
    for a in range(D):
        v0, v1 = vals[0::2], vals[1::2]
        diff = v1 - v0
        assert fits(diff, F, T), "v1 - v0"
        assert np.abs(diff).max() < (1 << (60 - FW - 3)) and np.abs(ww[a]).max() < (1 << (FW + 3)), "int64 would overflow"
        p = ww[a][None] * diff
        assert np.all(p & ((1 << FW) - 1) == 0), "a partial lerp is finer than 2^-%d" % F
        vals = v0 + (p >> FW)
        assert fits(vals, F, T), "a partial lerp"
    return vals[0]


def stage_costs(spec):
    """g[state, visiting index] (int64 fixed point) of the stage cost: the ordered sum in the cost's type, then the arithmetic
    type."""
    n, m, D, C = spec.n, spec.m, spec.D, spec.C
    T = np.dtype(spec.dtype)
    gsum = _ordered_sum(spec.cost_terms, n + m, (np.dtype(spec.cost_dtype or T),), "cost")
    assert fits(gsum, F, T)
    full = np.broadcast_to(gsum, n + m).reshape((spec.nS,) + tuple(m), order="F")     # state column-major, control dims kept
    return np.ascontiguousarray(full.reshape(spec.nS, -1))                           # C order over control dims: dim 0 slowest


def exact_stage(spec, Jn_fx, loc=None, dist=None):
    """One backup from the stored cost-to-go Jn_fx [nS] (fixed point).  dist = (offsets [D, W], p [W] or None, 'expect' / 'worst'):
    the disturbance-aware stage - per node the interpolated value; expect: acc = p_0 v_0, then acc = fma(p_w, v_w, acc); worst:
    max_w; total = g + acc.  -> totals [nS, nU] in visiting order."""
    n, m, D, C = spec.n, spec.m, spec.D, spec.C
    T = np.dtype(spec.dtype)
    if loc is None:
        loc = _Located(spec, None if dist is None else np.asarray(dist[0], dtype=np.float64))
    W = len(loc.cells)
    if dist is not None and dist[2] == "expect":
        pw = np.full(W, 1.0 / W) if dist[1] is None else np.asarray(dist[1], dtype=np.float64)
        pf = np.rint(pw * (1 << FW)).astype(np.int64)
        assert np.array_equal(pf, pw * (1 << FW)) and fits(pf, FW, T)
    g = stage_costs(spec)
    Jg = np.asarray(Jn_fx, dtype=np.int64).reshape(n, order="F")
    assert fits(Jg, F, T)
    tot = np.empty((spec.nS, spec.nU), dtype=np.int64)
    for u in range(spec.nU):
        cj = np.unravel_index(u, tuple(m), order="C")
        acc = None
        for w in range(W):
            cc = [np.broadcast_to(_at_control(c, D, cj), n) for c in loc.cells[w]]
            ww = [np.broadcast_to(_at_control(x, D, cj), n) for x in loc.ws[w]]
            v = _lerp(Jg, cc, ww, D, T)
            if dist is None:
                acc = v
            elif dist[2] == "expect":
                p = pf[w] * v
                assert np.all(p % (1 << FW) == 0)
                acc = (p >> FW) if w == 0 else acc + (p >> FW)
                assert fits(acc, F, T), "the expectation's running sum"
            else:
                acc = v if w == 0 else np.maximum(acc, v)
        t = g[:, u] + acc.reshape(-1, order="F")
        assert fits(t, F, T), "a total"
        tot[:, u] = t
    return tot


def tie_reference(spec, terminal, stages, dist=None):
    """The backward sweep in exact arithmetic.  Column k of every [nS, stages] array is stage k; stage `stages - 1` is the first one
    computed, from `terminal` (the layout of the C twin's J_stages / idx_stages).
      J_stages        the stored cost-to-go, in the storage type (exactly representable: asserted)
      idx_stages      label of the FIRST minimiser in visiting order (control dim 0 slowest): column-major + index_base
      last_idx_stages label of the LAST minimiser in visiting order
      minimisers      per stage a bool array [nS, nU] over the visiting index
      g               the stage cost [nS, nU] over the visiting index, float64
      weights         every interpolation weight that occurred, as floats"""
    sto = np.dtype(spec.j_dtype)
    loc = _Located(spec, None if dist is None else np.asarray(dist[0], dtype=np.float64))
    lab = visiting_labels(spec.m, spec.index_base)
    J = to_fixed(np.asarray(terminal, dtype=np.float64).reshape(-1), "terminal")
    assert J.shape == (spec.nS,) and fits(J, F, sto)
    Js = np.zeros((spec.nS, stages), dtype=sto, order="F")
    first = np.zeros((spec.nS, stages), dtype=np.int64, order="F")
    last = np.zeros((spec.nS, stages), dtype=np.int64, order="F")
    masks = [None] * stages
    for k in range(stages - 1, -1, -1):
        tot = exact_stage(spec, J, loc, dist)
        J = tot.min(axis=1)
        mask = tot == J[:, None]
        Js[:, k] = from_fixed(J, sto)
        first[:, k] = lab[np.argmax(mask, axis=1)]
        last[:, k] = lab[spec.nU - 1 - np.argmax(mask[:, ::-1], axis=1)]
        masks[k] = mask
    return {"J_stages": Js, "idx_stages": first, "last_idx_stages": last, "minimisers": masks, "J": Js[:, 0].copy(),
            "idx": first[:, 0].copy(), "g": stage_costs(spec).astype(np.float64) / float(1 << F),
            "weights": sorted(x / float(1 << FW) for x in loc.weights_seen)}


# ---- what kinds of tie a sweep holds ---------------------------------------------------------------------------------------------
def tie_counts(spec, ref):
    """Counts over the states of every stage (summed over the stages unless said otherwise).  u* = the first minimiser's visiting
    index, u' any other minimiser of the same state.
      mixed_first / mixed_later   states with two or more minimisers whose stage costs g differ: first computed stage / later ones
      order                       states whose first minimiser in visiting order does not carry the lowest label (C >= 2 only)
      not_zero                    states whose first minimiser is not control 0
      three_way                   states with three or more minimisers
      pairs_first / pairs_later   sets of (u*, u') with g differing, first stage / later stages
      lower_lane, same_lane, last_pass       the control-split kernel's (64 lanes, lane = u % 64): u' >= 64 in a lower lane than
                                  u*; u' = u* + 64 j; u* in the last, partly filled pass
      trip_shared, trip_apart, inner, odd_first   the nested kernels' (outer step o = u // m_last, two steps per trip): u* and u' in
                                  steps 2t and 2t + 1; in steps of different trips; in one step; u* in an odd step"""
    stages = ref["J_stages"].shape[1]
    g = ref["g"]
    nU = spec.nU
    lab = visiting_labels(spec.m, 0)
    u_all = np.arange(nU)
    ml = spec.m[-1]
    out = dict(mixed_first=0, mixed_later=0, order=0, not_zero=0, three_way=0, pairs_first=set(), pairs_later=set(), lower_lane=0,
               same_lane=0, last_pass=0, trip_shared=0, trip_apart=0, inner=0, odd_first=0)
    for k in range(stages):
        mask = ref["minimisers"][k]
        us = np.argmax(mask, axis=1)
        gs = g[np.arange(spec.nS), us]
        mixed = mask & (g != gs[:, None])
        late = "first" if k == stages - 1 else "later"
        out["mixed_" + late] += int(mixed.any(axis=1).sum())
        out["pairs_" + late].update(zip(us[np.nonzero(mixed)[0]].tolist(), np.nonzero(mixed)[1].tolist()))
        out["order"] += int((np.where(mask, lab[None, :], nU).min(axis=1) != lab[us]).sum())
        out["not_zero"] += int((us != 0).sum())
        out["three_way"] += int((mask.sum(axis=1) >= 3).sum())
        other = mask & (u_all[None, :] != us[:, None])
        out["lower_lane"] += int((other & (u_all[None, :] >= 64) & ((u_all[None, :] % 64) < (us[:, None] % 64))).any(axis=1).sum())
        out["same_lane"] += int((other & ((u_all[None, :] - us[:, None]) % 64 == 0)).any(axis=1).sum())
        if nU % 64:
            out["last_pass"] += int((us >= 64 * (nU // 64)).sum())
        o_all, o_s = u_all // ml, us // ml
        tied_o = other & (o_all[None, :] != o_s[:, None])
        out["trip_shared"] += int((tied_o & (o_all[None, :] // 2 == o_s[:, None] // 2)).any(axis=1).sum())
        out["trip_apart"] += int((tied_o & (o_all[None, :] // 2 != o_s[:, None] // 2)).any(axis=1).sum())
        out["inner"] += int((other & (o_all[None, :] == o_s[:, None])).any(axis=1).sum())
        out["odd_first"] += int((other.any(axis=1) & (o_s % 2 == 1)).sum())
    return out


# ---- generators -----------------------------------------------------------------------------------------------------------------
def _spec(*args, **kw):
    from hjbdp import ProblemSpec
    return ProblemSpec(*args, **kw)


def _term(dims, data):
    from hjbdp import Term
    return Term(dims, np.asarray(data, dtype=np.float64))


def lattice_knots(n, h=1.0, uneven=False):
    """Integers times the power of two h, centred; uneven: spacings cycling 1, 2, 4 (times h)."""
    if uneven:
        k = np.concatenate([[0.0], np.cumsum(np.array([1.0, 2.0, 4.0])[np.arange(n - 1) % 3])])
        return (k - k[n // 2]) * h
    return (np.arange(n) - n // 2) * float(h)


def lattice_terminal(spec, seed=0, top=5):
    return np.random.default_rng(1000 + seed).integers(0, top + 1, spec.nS).astype(spec.j_dtype)


def _cyc(values, count, shift=0):
    v = np.asarray(values, dtype=np.float64)
    return v[(np.arange(count) + shift) % len(v)]


def _lattice_cost(rng, n, m, D, top=3):
    cost = [_term((a,), (np.arange(n[a]) + a) % 3) for a in range(D)]
    for c in range(len(m)):
        cost.append(_term((D + c,), rng.integers(0, top + 1, m[c])))
    return cost[:12]


def tie_free_problem(seed, n, m=(5,), dtype=np.float32, h=1.0, uneven=False, reach=2, late=False, **typing):
    """tests/problems.py's free shape (K1, K5, K7, K22, K24): axis a = knots + (D > 1) a state-only term over dim a + 1 of
    {0, +1, 0, -1} cells + one term per control dim c with c mod D == a (for C <= D: the dim a mod C) of whole cells drawn from
    -reach .. reach.  late: the LAST control in visiting order costs 0 and is the only one that moves every axis `reach + 1`
    cells - a candidate for a first minimiser in the control-split kernel's last pass."""
    rng = np.random.default_rng(seed)
    D, C = len(n), len(m)
    knots = [lattice_knots(n[a], h, uneven) for a in range(D)]
    drives = [[c for c in range(C) if c % D == a] or [a % C] for a in range(D)]
    nxt = []
    cost = _lattice_cost(rng, n, m, D)
    for a in range(D):
        terms = [_term((a,), knots[a])]
        if D > 1:
            d = (a + 1) % D
            terms.append(_term((d,), h * _cyc((0, 1, 0, -1), n[d], a)))
        for c in drives[a]:
            lev = rng.integers(-reach, reach + 1, m[c]).astype(np.float64)
            if late:
                lev[-1] = reach + 1 if c == drives[a][0] else 0
            terms.append(_term((D + c,), h * lev))
        nxt.append(terms)
    if late:
        for c in range(C):
            cost[D + c].data[-1] = 0.0
    return _spec(knots, m, nxt, cost, dtype=dtype, **typing)


def tie_nested_problem(seed, n, m, dtype=np.float32, mono="inc", row=False, h=1.0, index_base=1):
    """nested_problem's shape (K2, K3, K8): control dim c drives axis D - C + c only, by whole cells -2 .. 2 (the innermost control
    the LAST axis, its table increasing, decreasing or neither); every axis also couples to up to two other state dims by
    {0, 0, +1, 0, -1} cells.  row: no axis >= 1 sees state dim 0 (variant 6's rule)."""
    rng = np.random.default_rng(seed)
    D, C = len(n), len(m)
    g = tuple(n) + tuple(m)
    knots = [lattice_knots(n[a], h) for a in range(D)]
    nxt = []
    for a in range(D):
        terms = [_term((a,), knots[a])]
        others = [d for d in range(D) if d != a and not (row and a >= 1 and d == 0)]
        if others:
            pick = sorted(rng.choice(others, size=min(len(others), 2), replace=False).tolist())
            terms.append(_term(pick, h * rng.choice([0.0, 0.0, 1.0, 0.0, -1.0], size=tuple(g[d] for d in pick))))
        c = a - (D - C)
        if c >= 0:
            steps = np.sort(_cyc(STEPS, g[D + c], 0 if g[D + c] >= 5 else 1))
            if c == C - 1:
                lev = steps if mono == "inc" else (steps[::-1].copy() if mono == "dec" else np.concatenate([steps[1:2], steps[:1], steps[2:]]))
            else:
                lev = steps[rng.permutation(len(steps))]
            terms.append(_term((D + c,), h * lev))
        nxt.append(terms)
    return _spec(knots, m, nxt, _lattice_cost(rng, n, m, D), dtype=dtype, index_base=index_base)


CS_PAIRS = ((-2, -0.5), (0, -0.5), (2, -0.5), (-2, 0.0), (0, 0.0), (2, 0.0), (-1, 0.5), (1, 0.5), (0, 0.5))


def tie_colsweep_problem(seed, n, gax=3, dtype=np.float32, j_storage=None, a1_axis=None, whole=False, index_base=1, **typing):
    """placement_colsweep_problem's shape (K10 / K13), nine controls: the group axis `gax` moves -2 .. 2 whole cells with the
    control, the window axis by {-1/2, 0, +1/2} cell (that generator's nine (step, half-step) pairs, permuted), so `gax` is the
    axis the plan groups by.  Axes 0 and 1 move with the state only, by {-1, -1/2, 0, +1/2, +1} cell (whole: whole cells only -
    one fraction bit per stage instead of three, what binary16 storage keeps exact over two stages).  Axis 0 never moves a whole cell
    up: that would clamp the last TWO states of a row (the query of the last but one sits on the last knot), and the one-load form
    admits one state per row whose cell is not its neighbours' plus a constant.  a1_axis as in colsweep_problem."""
    rng = np.random.default_rng(seed)
    assert len(n) == 4
    nU = 9
    wax = 5 - gax
    knots = [lattice_knots(n[a]) for a in range(4)]
    sub = [-1.0, 0.0, 1.0] if whole else [-1.0, -0.5, 0.0, 0.5, 1.0]
    nxt = [None] * 4
    nxt[0] = [_term((0,), knots[0]), _term((2,), rng.choice(sub[:-1], n[2])), _term((3,), np.zeros(n[3]))]
    nxt[1] = [_term((1,), knots[1]), _term((3,), rng.choice(sub, n[3])), _term((2,), np.zeros(n[2]))]
    if a1_axis is not None:
        nxt[1] = [_term((1,), knots[1]), _term((a1_axis,), rng.choice(sub, n[a1_axis]))]
    pairs = np.array(CS_PAIRS)[rng.permutation(nU)]
    nxt[gax] = [_term((gax,), knots[gax]), _term((4,), pairs[:, 0])]
    nxt[wax] = [_term((wax,), knots[wax]), _term((4,), pairs[:, 1])]
    st = {a: _term((a,), (np.arange(n[a]) + a) % 3) for a in range(4)}
    cu = rng.integers(0, 4, nU)
    return _spec(knots, [nU], nxt, [st[0], st[2], st[3], st[1], _term((4,), cu)], dtype=dtype, index_base=index_base,
                 j_storage=j_storage, **typing)


def tie_rate_shared_problem(seed, n_so=(8, 4, 4), n_rates=(4, 4, 13), m=(3, 3, 11), dtype=np.float32, index_base=1, j_storage=None,
                            coarse=False):
    """placement_rate_shared_problem's shape (K15, and K3's three-plane window): the state-only axes tabulated over ALL state dims
    (moves of {-1/2, 0, +1/2} cell); rate axis c moves by {0, 0, +1, 0, -1} cells of the two other rates' indices plus a level of
    control dim c - the eleven inner levels (j - 5) / 8 cell (less than a cell per level, the admission rule), the outer ones
    from {-1, 0, +1/2, -1/2}.  coarse: inner levels (j - 5) / 4, outer ones whole cells, state-only axes at rest - two fraction bits
    per stage instead of six, what binary16 storage keeps exact over two stages."""
    rng = np.random.default_rng(seed)
    NP = len(n_so)
    n = tuple(n_so) + tuple(n_rates)
    D = len(n)
    knots = [lattice_knots(n[a]) for a in range(D)]
    nxt = []
    for a in range(NP):
        shape = [1] * D
        shape[a] = n[a]
        mv = rng.choice([0.0, 0.0, 0.5, -0.5], size=n) if a == 0 and not coarse else np.zeros(n)
        nxt.append([_term(tuple(range(D)), knots[a].reshape(shape) + mv)])
    for c in range(3):
        a = NP + c
        others = [NP + x for x in range(3) if x != c]
        lev = (np.arange(m[c]) - m[c] // 2) / (4.0 if coarse else 8.0) if c == 2 else \
            np.sort(_cyc((-1.0, 0.0, 1.0) if coarse else (-1.0, 0.0, 0.5, -0.5), m[c]))
        tab = rng.choice([0.0, 0.0, 1.0, 0.0, -1.0], size=(n[others[0]], n[others[1]]))[:, :, None] + lev[None, None, :]
        nxt.append([_term((a,), knots[a]), _term(tuple(others) + (D + c,), tab)])
    cost = [_term((NP + c,), (np.arange(n[NP + c]) + c) % 3) for c in range(3)]
    cost.append(_term(tuple(range(NP)), rng.integers(0, 3, tuple(n_so))))
    for c in range(3):
        cost.append(_term((D + c,), rng.integers(0, 4, m[c])))
    return _spec(knots, list(m), nxt, cost, dtype=dtype, index_base=index_base, j_storage=j_storage)


def tie_local2d_problem(seed, n=(13, 13), m=(4,), dtype=np.float64, half=True, index_base=1, **typing):
    """placement_local2d_problem's shape (K9: every query's cell is the state's own or the one below): axis a = knots + ONE term over
    (dim a, the control): level 0 stays on the node, 1 goes one cell down (i = 0: below the grid), 2 half a cell down and 3 half a
    cell up on axis 0 (i = n - 1, level 3: one cell up, beyond the grid, clamped into the last cell); axis 1 moves whole cells only.
    half=False: no sub-cell move at all.  K9 runs sixteen stages or more per solve and the extrapolated ends about double per stage,
    so the values need some 21 integer bits by then: with the half-cell moves' sixteen fraction bits that is float64's to hold,
    without them float32's 24 bits do.  Eight levels (the four, then the four reversed) are the general form."""
    rng = np.random.default_rng(seed)
    knots = [lattice_knots(n[a]) for a in range(2)]
    nxt = []
    for a in range(2):
        i = np.arange(n[a])
        h = 0.5 if (a == 0 and half) else 0.0
        lev = [np.zeros(n[a]), -np.ones(n[a]), np.where(i == 0, 0.0, -h), np.where(i == n[a] - 1, 1.0, h)]
        tab = np.stack([lev[j % 4] if (j // 4) % 2 == 0 else lev[3 - j % 4] for j in range(m[0])], axis=1)
        nxt.append([_term((a,), knots[a]), _term((a, 2), tab)])
    cost = [_term((0, 1), rng.integers(0, 3, tuple(n))), _term((2,), rng.integers(0, 4, m[0]))]
    return _spec(knots, list(m), nxt, cost, dtype=dtype, index_base=index_base, **typing)


# ---- the registered cases ------------------------------------------------------------------------------------------------------
class TieCase:
    """family decides which conditions assert_ties asks for: 'free' (the general ones), 'k5', 'colsweep' (the union over its seeds
    counts), 'nested'.  seeds: literals found by search on the CPU (the first seeds, counted up from the one given, whose problem
    meets the conditions).  top: the terminal cost is integers 0 .. top.  dist: (offsets [D, W], weights or None, mode) of the
    disturbance-aware backup, or None."""

    def __init__(self, family, seeds, stages, build, top=5, dist=None):
        self.family, self.seeds, self.stages, self.build, self.top, self.dist = family, list(seeds), stages, build, top, dist


FREE_SHAPES = {1: ((13,), (5,)), 2: ((13, 13), (5, 5)), 4: ((13, 3, 4, 13), (5, 5)), 6: ((13, 3, 3, 3, 3, 13), (5, 1, 5))}
NESTED_SHAPES = {2: ((13, 13), (5,)), 3: ((5, 13, 13), (3, 5, 5)), 5: ((4, 3, 4, 13, 13), (3, 5, 5)), 6: ((4, 3, 4, 3, 3, 13), (3, 3, 5))}
ROW_SHAPE = ((70, 13, 13), (5, 5))
COLSWEEP_SHAPE = (8, 5, 13, 13)
K5_STATES = (7, 7)
STAGES = 3
TIE_CASES = {}


def _register():
    f32, f64 = np.float32, np.float64

    class _Reg(dict):
        def __setitem__(self, name, v):
            TIE_CASES[name] = v if isinstance(v, TieCase) else TieCase(*v)
    T = _Reg()
    for D, (n, m) in FREE_SHAPES.items():
        for dt in (f32, f64):
            T["free-%d-%s" % (D, np.dtype(dt).name)] = (
                "free", [10 + D], 2 if D == 6 else STAGES,
                lambda s, n=n, m=m, dt=dt, D=D: tie_free_problem(s, n, m, dtype=dt, index_base=1, reach=1 if D == 6 else 2))
    T["free-2-uneven"] = ("free", [1], STAGES, lambda s: tie_free_problem(s, (13, 13), (5, 5), dtype=f32, uneven=True, index_base=0))
    T["free-2-half"] = ("free", [22], STAGES, lambda s: tie_free_problem(s, (13, 13), (5, 5), dtype=f64, h=0.5, index_base=0))
    T["free-2-tab64"] = ("free", [23], STAGES, lambda s: tie_free_problem(s, (13, 13), (5, 5), dtype=f32, table_dtype=f64, index_base=1))
    T["free-2-cost64"] = ("free", [24], STAGES, lambda s: tie_free_problem(s, (13, 13), (5, 5), dtype=f32, cost_dtype=f64, index_base=1))
    T["free-2-u8"] = ("free", [25], STAGES, lambda s: tie_free_problem(s, (13, 13), (5, 5), dtype=f32, idx_dtype=np.uint8, index_base=1))
    for name, m, dt, seed in (("k5-c1", (130,), f32, 15), ("k5-c2", (9, 15), f32, 64), ("k5-c3", (5, 5, 6), f64, 4), ("k5-small", (50,), f32, 2)):
        T[name] = ("k5" if name != "k5-small" else "free", [seed], STAGES,
                   lambda s, m=m, dt=dt: tie_free_problem(s, K5_STATES, m, dtype=dt, reach=2, late=True, index_base=1))
    # 130 x 130 float32 states are more than the control-split kernel stages in LDS: its form that reads J from memory
    T["k5-big"] = ("free", [5], 2, lambda s: tie_free_problem(s, (130, 130), (70,), dtype=f32, index_base=1))
    for D, (n, m) in NESTED_SHAPES.items():
        for mono in ("inc", "dec", None):
            T["nested-%d-%s" % (D, mono)] = ("nested", [40 + D], STAGES, lambda s, n=n, m=m, mono=mono: tie_nested_problem(s, n, m, mono=mono))
    T["nested-3-float64"] = ("nested", [49], STAGES, lambda s: tie_nested_problem(s, *NESTED_SHAPES[3], dtype=f64, index_base=0))
    T["row-float32"] = ("nested", [50], STAGES, lambda s: tie_nested_problem(s, *ROW_SHAPE, row=True))
    T["row-float64"] = ("nested", [51], STAGES, lambda s: tie_nested_problem(s, *ROW_SHAPE, row=True, dtype=f64))
    for gax in (2, 3):
        T["colsweep-g%d-f32" % gax] = ("colsweep", CS_SEEDS[gax], STAGES, lambda s, gax=gax: tie_colsweep_problem(s, COLSWEEP_SHAPE, gax=gax))
        T["colsweep-g%d-f16" % gax] = ("colsweep", CS_SEEDS_F16[gax], 2,
                                       lambda s, gax=gax: tie_colsweep_problem(s, COLSWEEP_SHAPE, gax=gax, j_storage=np.float16, whole=True), 3)
        T["colsweep-g%d-coop" % gax] = ("free", [70 + gax], STAGES, lambda s, gax=gax: tie_colsweep_problem(s, COLSWEEP_SHAPE, gax=gax, a1_axis=gax))
    T["colsweep-g3-tab64"] = ("free", [76], STAGES, lambda s: tie_colsweep_problem(s, COLSWEEP_SHAPE, gax=3, table_dtype=f64, idx_dtype=np.uint8))
    T["colsweep-g3-cost64"] = ("free", [77], STAGES, lambda s: tie_colsweep_problem(s, COLSWEEP_SHAPE, gax=3, cost_dtype=f64, index_base=0))
    T["rates"] = ("nested", [80], 2, lambda s: tie_rate_shared_problem(s))
    T["rates-f16"] = ("nested", [81], 2, lambda s: tie_rate_shared_problem(s, j_storage=np.float16, coarse=True), 1)
    # K9 runs from sixteen stages on (two launches of eight): what stays exact that long - see tie_local2d_problem
    for mm in ((4,), (8,)):
        T["local2d-f64-u%d" % mm[0]] = ("free", [90], 16, lambda s, mm=mm: tie_local2d_problem(s, m=mm, dtype=f64))
        T["local2d-f32-u%d" % mm[0]] = ("free", [91], 16, lambda s, mm=mm: tie_local2d_problem(s, m=mm, dtype=f32, half=False))
    T["local2d-tab64-u4"] = ("free", [91], 16, lambda s: tie_local2d_problem(s, m=(4,), dtype=f32, half=False, table_dtype=f64))
    # K24: two nodes of weight 1/2 a whole cell either way on axis 0, one and two cells on axis 1
    for mode in ("expect", "worst"):
        for dt in (f32, f64):
            T["dist-%s-%s" % (mode, np.dtype(dt).name)] = TieCase(
                "free", [61], STAGES, lambda s, dt=dt: tie_free_problem(s, (13, 13), (5, 5), dtype=dt, index_base=1),
                dist=(DIST_OFFSETS, (0.5, 0.5) if mode == "expect" else None, mode))


DIST_OFFSETS = np.array([[1.0, -1.0], [-1.0, 2.0]])
CS_SEEDS = {2: [1, 2, 3, 4, 5, 6], 3: [1, 2, 3, 4, 5, 6]}
CS_SEEDS_F16 = {2: [1, 2, 3, 4, 5, 6], 3: [1, 2, 3, 4, 5, 6]}
_register()
_BUILT = {}


def tie_case(name):
    """-> [(spec, terminal, exact reference)] per seed of the registered case, built once and never written to."""
    if name not in _BUILT:
        case = TIE_CASES[name]
        out = []
        for s in case.seeds:
            spec = case.build(s)
            term = lattice_terminal(spec, s, case.top)
            ref = tie_reference(spec, term, case.stages, case.dist)
            for v in (term, ref["J_stages"], ref["idx_stages"], ref["last_idx_stages"], ref["J"], ref["idx"], ref["g"]):
                v.setflags(write=False)
            out.append((spec, term, ref))
        _BUILT[name] = out
    return _BUILT[name]


def assert_ties(name):
    """The conditions that make a registered case worth running, asserted without the library.  -> the counts (sets as sizes)."""
    family = TIE_CASES[name].family
    members = tie_case(name)
    total = None
    for spec, term, ref in members:
        cnt = tie_counts(spec, ref)
        assert ref["J_stages"].shape[1] >= 2
        if total is None:
            total = cnt
        else:
            for key, v in cnt.items():
                total[key] = (total[key] | v) if isinstance(v, set) else total[key] + v
        # general, per member
        assert cnt["mixed_first"] >= 1 and cnt["mixed_later"] >= 1, (name, cnt)
        assert cnt["not_zero"] >= 1, (name, cnt)
        if spec.C >= 2 and min(spec.m) > 1:
            assert cnt["order"] >= 1, (name, cnt)
        w = ref["weights"]
        assert min(w) < 0 and max(w) > 1, (name, "no query beyond both grid ends", w)
    spec = members[0][0]
    if family == "k5":
        assert spec.nU >= 130 and spec.nU % 64
        for key in ("lower_lane", "same_lane", "last_pass"):
            assert total[key] >= 1, (name, key, total)
    elif family == "colsweep":
        want = {(a, b) for a in range(9) for b in range(a + 1, 9)}
        got = total["pairs_first"] | total["pairs_later"]
        assert len(members) <= 6 and got == want, (name, sorted(want - got))
        assert total["pairs_later"] == want, (name, "in stages after the first", sorted(want - total["pairs_later"]))
        assert total["three_way"] >= 1, name
    elif family == "nested":
        assert total["inner"] >= 1, (name, total)
        n_outer = spec.nU // spec.m[-1]
        if n_outer >= 2:
            assert total["trip_shared"] >= 1 and total["odd_first"] >= 1, (name, total)
        if n_outer >= 3:
            assert total["trip_apart"] >= 1, (name, total)
    return {k: (len(v) if isinstance(v, set) else v) for k, v in total.items()}
