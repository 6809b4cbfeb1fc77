"""Seeded synthetic problems for parity tests (not reference code: generators of
inputs).  Every generator returns an hjbdp.ProblemSpec."""
from __future__ import annotations

import numpy as np

from hjbdp import ProblemSpec, Term


def random_problem(seed, n, m, dtype=np.float64, nonuniform=False, spread=0.35, index_base=0):
    """D = len(n) state dims, C = len(m) control dims.  x_next_a = x_a + (terms
    mixing 1..3 other dims and controls); cost = sum of per-dim quadratics + a
    mixed state/control term; queries land inside, on and outside the grid."""
    rng = np.random.default_rng(seed)
    D, C = len(n), len(m)
    g = tuple(n) + tuple(m)
    knots = []
    for a in range(D):
        if nonuniform:
            k = np.cumsum(rng.uniform(0.5, 1.5, n[a]))
            k = (k - k[0]) / (k[-1] - k[0]) * 2.0 - 1.0
        else:
            k = np.linspace(-1.0, 1.0, n[a])
        knots.append(k.astype(dtype).astype(np.float64))
    nxt = []
    for a in range(D):
        terms = [Term((a,), knots[a].copy())]
        # a state-only coupling term over up to 2 other dims
        others = [d for d in range(D) if d != a]
        if others:
            pick = sorted(rng.choice(others, size=min(len(others), int(rng.integers(1, 3))), replace=False).tolist())
            shape = tuple(g[d] for d in pick)
            terms.append(Term(pick, spread * 0.5 * rng.standard_normal(shape)))
        # a control term (some axes have none, some mix a state dim in)
        r = rng.random()
        if r < 0.75:
            c = int(rng.integers(0, C))
            if r < 0.25 and D > 1:
                d = int(rng.choice(others))
                dims = (d, D + c)
                terms.append(Term(dims, spread * rng.standard_normal((g[d], g[D + c]))))
            else:
                terms.append(Term((D + c,), spread * rng.standard_normal(g[D + c])))
        if rng.random() < 0.3:  # a trailing state-only term after a control term
            terms.append(Term((a,), 0.05 * rng.standard_normal(g[a])))
        nxt.append(terms)
    cost = [Term((a,), (1.0 + a) * knots[a] ** 2) for a in range(D)]
    for c in range(C):
        cost.append(Term((D + c,), 0.3 * rng.standard_normal(m[c]) ** 2))
    if D + C <= 5:
        cost.append(Term((0, D), 0.1 * rng.random((g[0], g[D]))))
    return ProblemSpec(knots, m, nxt, cost[:12], dtype=dtype, index_base=index_base)


def random_terminal(spec, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random(spec.nS).astype(spec.dtype)


def nested_problem(seed, n, m, dtype=np.float32, nonuniform=False, spread=0.2, mixed_inner=False, monotone=None):
    """Structure of the spacecraft solvers: control dim c drives state axis
    D-C+c only (the innermost control dim drives the LAST axis); every axis also
    couples to other state dims.  mixed_inner adds an inner term that also
    depends on a state dim (a 'general' inner term for the nested kernel)."""
    rng = np.random.default_rng(seed)
    D, C = len(n), len(m)
    g = tuple(n) + tuple(m)
    knots = []
    for a in range(D):
        if nonuniform:
            k = np.cumsum(rng.uniform(0.5, 1.5, n[a]))
            k = (k - k[0]) / (k[-1] - k[0]) * 2.0 - 1.0
        else:
            k = np.linspace(-1.0, 1.0, n[a])
        knots.append(k.astype(dtype).astype(np.float64))
    nxt = []
    for a in range(D):
        terms = [Term((a,), knots[a].copy())]
        others = [d for d in range(D) if d != a]
        if others:
            pick = sorted(rng.choice(others, size=min(len(others), 2), replace=False).tolist())
            terms.append(Term(pick, spread * 0.5 * rng.standard_normal(tuple(g[d] for d in pick))))
        c = a - (D - C)
        if c >= 0:
            if mixed_inner and others:
                d = int(others[0])
                dims = tuple(sorted((d, D + c)))
                terms.append(Term(dims, spread * rng.standard_normal(tuple(g[x] for x in dims))))
                if mixed_inner == "only" and c == C - 1:     # the inner term depends on a state dim AND the control
                    nxt.append(terms)
                    continue
            tab = spread * rng.standard_normal(g[D + c])
            if monotone and c == C - 1:       # monotone inner control table (what real actuator levels are)
                tab = np.sort(tab) if monotone == "inc" else np.sort(tab)[::-1].copy()
            terms.append(Term((D + c,), tab))
        nxt.append(terms)
    cost = [Term((a,), (1.0 + a) * knots[a] ** 2) for a in range(D)]
    for c in range(C):
        cost.append(Term((D + c,), 0.3 * rng.standard_normal(m[c]) ** 2))
    return ProblemSpec(knots, m, nxt, cost[:12], dtype=dtype, index_base=1)


def colsweep_problem(seed, n, nU=9, nonuniform=False, gax=3, big=2.7, small=0.6, cost="fast", a1_amp=0.6, levels=5,
                     dtype=np.float32, index_base=1, j_storage=None, a1_axis=None):
    """The shape of the column-sweep stage kernel (variant 7, kernels_colsweep.h; pos-att with the axes relabelled
    (x, theta, v, w)): D = 4, one control dim; axes 0 and 1 move with the state only (axis 0 over dims {0,2,3}, axis 1
    over dims {1,2,3}); axes 2 and 3 move with the control - the "group" axis `gax` by `big` cells times one of
    `levels` distinct values, the other ("window") axis by less than `small` < 1 cells.  a1_amp > 1 makes the axis-1
    cell jump irregularly along a column (re-priming path).  cost: 'fast' (state terms, the dim-1 term last, one
    control term), 'step01' (first term over dims (0,1): nothing is column-invariant, per-step term not uniform),
    'multi' (two control-only terms), 'ctrl_only' (no state term at all).  a1_axis=d: axis 1 moves with dim 1 and
    dim d only, as pos-att's theta+ = theta + h w does (the cooperative form wants d = the group axis the plan picks)."""
    rng = np.random.default_rng(seed)
    assert len(n) == 4
    knots = []
    for a in range(4):
        if nonuniform:
            k = np.cumsum(rng.uniform(0.6, 1.4, n[a]))
            k = (k - k[0]) / (k[-1] - k[0]) * 2.0 - 1.0
        else:
            k = np.linspace(-1.0, 1.0, n[a])
        knots.append(k.astype(dtype).astype(np.float64))
    hs = [2.0 / (n[a] - 1) for a in range(4)]
    wax = 5 - gax
    lev = np.linspace(-1.0, 1.0, levels) if levels > 1 else np.zeros(1)
    d = lev[rng.permutation(nU) % levels]                       # group-axis displacement level of each control
    c = rng.uniform(-1.0, 1.0, nU)                              # window-axis displacement of each control
    nxt = [None] * 4
    nxt[0] = [Term((0,), knots[0].copy()), Term((2,), 0.7 * hs[0] * rng.uniform(-1, 1, n[2])),
              Term((3,), 0.25 * hs[0] * rng.uniform(-1, 1, n[3]))]
    nxt[1] = [Term((1,), knots[1].copy()), Term((3,), a1_amp * hs[1] * rng.uniform(-1, 1, n[3])),
              Term((2,), 0.2 * hs[1] * rng.uniform(-1, 1, n[2]))]
    if a1_axis is not None:
        nxt[1] = [Term((1,), knots[1].copy()), Term((a1_axis,), a1_amp * hs[1] * rng.uniform(-1, 1, n[a1_axis]))]
    nxt[gax] = [Term((gax,), knots[gax].copy()), Term((4,), big * hs[gax] * d)]
    nxt[wax] = [Term((wax,), knots[wax].copy()), Term((4,), small * hs[wax] * c)]
    cu = 0.3 * np.round(rng.uniform(0, 3, nU)) ** 2             # repeated values: exact ties between controls
    st = {a: Term((a,), (1.0 + a) * knots[a] ** 2) for a in range(4)}
    if cost == "fast":
        ct = [st[0], st[2], st[3], st[1], Term((4,), cu)]
    elif cost == "step01":
        ct = [Term((0, 1), 0.1 * rng.random((n[0], n[1]))), st[2], st[3], Term((4,), cu)]
    elif cost == "multi":
        ct = [st[0], st[1], st[3], Term((4,), cu), Term((4,), 0.1 * rng.random(nU))]
    elif cost == "ctrl_only":
        ct = [Term((4,), cu)]
    else:
        raise ValueError(cost)
    return ProblemSpec(knots, [nU], nxt, ct, dtype=dtype, index_base=index_base, j_storage=j_storage)


def uphill_problem(seed=0, n=(8, 6, 17), dtype=np.float32, index_base=1):
    """A problem whose LAST axis drifts upward only - the halo a slab needs is not symmetric (hjbdp.sharded.required_halo:
    (1, 2) planes; the one low plane is the last cell's clamp).  D = 3, one control dim of 4 levels: axis 0 moves with dim 1 and
    axis 1 with dim 2 by at most 0.4 cells, axis 2 by (0.2, 0.7, 1.3, 1.8) cells with the control.  cost = per-axis quadratics
    + 0.3 u^2."""
    rng = np.random.default_rng(seed)
    assert len(n) == 3
    knots = [np.linspace(-1.0, 1.0, n[a]).astype(dtype).astype(np.float64) for a in range(3)]
    hs = [2.0 / (n[a] - 1) for a in range(3)]
    nxt = [[Term((0,), knots[0].copy()), Term((1,), 0.4 * hs[0] * rng.uniform(-1, 1, n[1]))],
           [Term((1,), knots[1].copy()), Term((2,), 0.4 * hs[1] * rng.uniform(-1, 1, n[2]))],
           [Term((2,), knots[2].copy()), Term((3,), hs[2] * np.array([0.2, 0.7, 1.3, 1.8]))]]
    cost = [Term((a,), (1.0 + a) * knots[a] ** 2) for a in range(3)] + [Term((3,), 0.3 * np.arange(4.0) ** 2)]
    return ProblemSpec(knots, [4], nxt, cost, dtype=dtype, index_base=index_base)


def rate_shared_problem(seed, n_so, n_rates, m=(11, 11, 11), gain=(0.55, 0.5, 0.6), nonuniform=False, so_move=0.7,
                        dtype=np.float32, index_base=1, j_storage=None):
    """The shape of K15 (kernels_uniwin.h; Solver_attitude.run with the angle axes first): the state-only axes `n_so`, whose
    next value is tabulated over ALL state dims, then three 'rate' axes whose next value depends on the three rates and on
    ONE control dim each (control dim c drives rate axis c; the innermost control the LAST axis).  gain[c] = the move of rate
    axis c, in cells, from the middle to either end of its control's range; costs repeat values (exact ties)."""
    rng = np.random.default_rng(seed)
    NP = len(n_so)
    n = tuple(n_so) + tuple(n_rates)
    D = len(n)
    knots = []
    for a in range(D):
        if nonuniform:
            k = np.cumsum(rng.uniform(0.6, 1.4, n[a]))
            k = (k - k[0]) / (k[-1] - k[0]) * 2.0 - 1.0
        else:
            k = np.linspace(-1.0, 1.0, n[a])
        knots.append(k.astype(dtype).astype(np.float64))
    hs = [2.0 / (n[a] - 1) for a in range(D)]
    all_dims = tuple(range(D))
    nxt = []
    for a in range(NP):
        shape = [1] * D
        shape[a] = n[a]
        tab = knots[a].reshape(shape) + so_move * hs[a] * rng.uniform(-1.0, 1.0, n)
        nxt.append([Term(all_dims, tab)])
    for c in range(3):
        a = NP + c
        others = [NP + x for x in range(3) if x != c]
        dims = tuple(others) + (D + c,)
        tab = 0.08 * hs[a] * rng.standard_normal((n[others[0]], n[others[1]]))[:, :, None] + \
            gain[c] * hs[a] * np.linspace(-1.0, 1.0, m[c])[None, None, :]
        nxt.append([Term((a,), knots[a].copy()), Term(dims, tab)])
    cost = [Term((NP + c,), (1.0 + c) * knots[NP + c] ** 2) for c in range(3)]
    cost.append(Term(tuple(range(NP)), 2.0 * rng.random(tuple(n_so))))
    for c in range(3):
        cost.append(Term((D + c,), 0.25 * np.round(rng.uniform(0, 3, m[c])) ** 2))
    return ProblemSpec(knots, list(m), nxt, cost, dtype=dtype, index_base=index_base, j_storage=j_storage)


def pos_att_channel_spec(cost_mode="f64", n=120, j_storage=None, channel="x"):
    """Solver_pos_att's channel on n^4 states exactly as bench.build_spec("c4") builds it (axes FAST_AXIS_ORDER =
    (x, theta, w, v), float64-built query tables, uint8 labels) but with the stage cost typed by `cost_mode`: 'f64' is the
    reference's own single(double sum) (Solver_pos_att.m:800-801, the mirror's default), 'terms' the bench's float32 terms.
    channel: 'x', 'z' or 'failure' (the x channel with thruster 0 failed, Solver_pos_att.m:236-240).  j_storage=np.float16:
    binary16 cost-to-go storage (C5)."""
    import hjbdp
    pa = hjbdp.Solver_pos_att()
    pa.cost_mode = cost_mode
    pa.n_mesh_x = pa.n_mesh_v = pa.n_mesh_t = pa.n_mesh_w = n
    sx, sv, st, sw = pa.grids()
    args = {"x": (st[0], pa.F_Thr0, pa.F_Thr1, pa.F_Thr6, pa.F_Thr7, pa.Qx1, pa.Qv1, pa.Qt1, pa.Qw1, pa.R1, pa.J2),
            "z": (st[2], pa.F_Thr4, pa.F_Thr5, pa.F_Thr10, pa.F_Thr11, pa.Qx3, pa.Qv3, pa.Qt3, pa.Qw3, pa.R3, pa.J1),
            "failure": (st[0], [0.0], pa.F_Thr1, pa.F_Thr6, pa.F_Thr7, pa.Qx1, pa.Qv1, pa.Qt1, pa.Qw1, pa.R1, pa.J2)}[channel]
    spec, _ = pa.build_channel_spec(sx, sv, args[0], sw, *args[1:])
    spec, _ = hjbdp.permute_state_axes(spec, hjbdp.Solver_pos_att.FAST_AXIS_ORDER)
    if j_storage is not None:
        spec = hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, dtype=np.float32, index_base=1,
                                 j_storage=j_storage, idx_dtype=spec.idx_dtype, table_dtype=spec.table_dtype,
                                 cost_dtype=spec.cost_dtype)
    assert spec.table_dtype == np.float64 and spec.idx_np_dtype == np.uint8
    assert (spec.cost_dtype == np.float64) == (cost_mode == "f64")
    return spec


# ---- placement problems: next-state queries that land on knots, beside them and beyond the ends BY CONSTRUCTION ------------------
# Every located axis starts with Term((a,), knots[a]) and goes on with terms whose values are integer multiples s * h_a of the
# grid step (h_a = (k[-1] - k[0]) / (n_a - 1), s in PLACEMENT_STEPS for the control-driven axes), cast to the type the queries are
# formed in.  The ordered sum fl(k_i + fl(s h)) is then a knot or one unit in the last place beside one, the first and the last
# knot included, and up to two cells beyond either end.  tests/test_placement_problems.py asserts the classes below without the
# library; tests/test_gpu_placements.py asserts them again on the problems it runs.
PLACEMENT_STEPS = (-2, -1, 0, 1, 2)
PLACEMENT_N = 13
PLACEMENT_CLASSES = ("on_knot", "ulp_below", "ulp_above", "first_knot", "last_knot", "outside", "guess_short", "guess_far")


def placement_knots(dtype, grid="even", n=PLACEMENT_N):
    """The located axis' knots as float64 values of `dtype`.  'even': linspace(-1, 1, n).  'near' / 'far' (n = 13 only): interior
    knots moved so that the host's deviation from evenly spaced (hjbdp_setup.hip upload_axes: max |k_i - (k_0 + i hstep)|) is
    1.4 hstep - still flagged uniform, the arithmetic first guess two cells off either way - and 1.6 hstep: the binary search."""
    k = np.linspace(-1.0, 1.0, n)
    if grid != "even":
        assert n == 13 and grid in ("near", "far")
        lo = -1.4 if grid == "near" else -1.6
        shift = np.array([0.0, -0.45, -0.9, lo, lo, -1.0, -0.5, 0.0, 0.5, 1.2, 1.4, 0.7, 0.0])  # narrowest cell 0.3 hstep
        k = k + shift * (2.0 / (n - 1))
    k = k.astype(dtype).astype(np.float64)
    assert np.all(np.diff(k) > 0)
    return k


def placement_deviation(k):
    """The host's uniformity measure of a knot vector, in units of its mean step (upload_axes flags uniform at <= 1.5)."""
    k = np.asarray(k, dtype=np.float64)
    h = (k[-1] - k[0]) / (len(k) - 1)
    return float(np.max(np.abs(k - (k[0] + np.arange(len(k)) * h))) / h)


def _step(k):
    return (k[-1] - k[0]) / (len(k) - 1)


def _cyc(values, count, shift=0):
    """`count` values cycling through `values`, starting `shift` places in."""
    v = np.asarray(values, dtype=np.float64)
    return v[(np.arange(count) + shift) % len(v)]


def _placement_cost(knots, m, rng, D):
    cost = [Term((a,), (1.0 + a) * knots[a] ** 2) for a in range(D)]
    for c in range(len(m)):
        cost.append(Term((D + c,), 0.3 * np.round(rng.uniform(0, 3, m[c])) ** 2))      # repeated values: exact ties between controls
    return cost[:12]


def locate_dtype(spec):
    """The type a spec's queries are formed and located in."""
    return np.dtype(spec.table_dtype or spec.dtype)


def placement_queries(spec, a):
    """Axis a's next-state query at every (state, control), shape n + m: the terms' ordered sum in the locate type (the first
    term as it is, every later one added and rounded), as tests/float64_refs.ordered_sum forms it."""
    dt = locate_dtype(spec)
    g = spec.n + spec.m
    acc = None
    for t in spec.next_terms[a]:
        x = np.asarray(t.data).astype(dt).reshape([g[d] if d in t.dims else 1 for d in range(len(g))])
        acc = x if acc is None else (acc + x).astype(dt)
    return np.broadcast_to(acc, g)


def placement_cells(k, q):
    """clip(upper_bound(k, q) - 1, 0, n - 2): the cell the twin's binary search finds."""
    return np.clip(np.searchsorted(k, q, side="right") - 1, 0, len(k) - 2)


def placement_guess(k, q, dtype):
    """The library's arithmetic first guess (find_cell, hjbdp_canon.h): (q - x0) * inv_h in `dtype`, inv_h = 1 / hstep formed in
    float64 and rounded to the type, clamped to [0, n - 2], truncated."""
    dt = np.dtype(dtype).type
    kk = np.asarray(k, dtype=np.float64)
    n = len(kk)
    inv_h = dt(1.0 / ((kk[-1] - kk[0]) / (n - 1)))
    f = ((np.asarray(q).astype(dt) - dt(kk[0])).astype(dt) * inv_h).astype(dt)
    return np.clip(f, dt(0), dt(n - 2)).astype(np.int64)


def placement_counts(k, q, dtype):
    """How many of the queries q fall in each of PLACEMENT_CLASSES on the knots k (float64 values of `dtype`), plus 'guess_short2' /
    'guess_far2': the first guess two or more cells below / above the cell."""
    dt = np.dtype(dtype).type
    kd = np.asarray(k).astype(dt)
    q = np.asarray(q).astype(dt).ravel()
    cell = placement_cells(kd, q)
    guess = placement_guess(k, q, dtype)
    on = np.isin(q, kd)
    return {
        "on_knot": int(on.sum()),
        "ulp_below": int(np.isin(np.nextafter(q, dt(np.inf)), kd).sum()),
        "ulp_above": int(np.isin(np.nextafter(q, dt(-np.inf)), kd).sum()),
        "first_knot": int((q == kd[0]).sum()),
        "last_knot": int((q == kd[-1]).sum()),
        "outside": int(((q < kd[0]) | (q > kd[-1])).sum()),
        "guess_short": int((guess < cell).sum()),
        "guess_far": int((guess > cell).sum()),
        "guess_short2": int((guess <= cell - 2).sum()),
        "guess_far2": int((guess >= cell + 2).sum()),
    }


def placement_crossings(spec, a, mono):
    """Over the innermost control's sweep of axis a: how many (state, outer control, j >= 1) have the query exactly on the lower knot
    of its cell where a one-sided test decides - increasing tables: the cell has just changed (a crossing taken at equality);
    decreasing tables: the query has come down onto the knot of a cell >= 1 and must stay in it (`<` taken as `<=` would leave)."""
    dt = locate_dtype(spec).type
    k = spec.knots[a].astype(dt)
    q = np.asarray(placement_queries(spec, a)).astype(dt)
    cell = placement_cells(k, q)
    on = q == k[cell]
    qj, qp = q[..., 1:], q[..., :-1]
    if mono == "inc":
        hit = on[..., 1:] & (cell[..., 1:] > cell[..., :-1]) & (qj > qp)
    else:
        hit = on[..., 1:] & (cell[..., 1:] >= 1) & (qj < qp)
    return int(hit.sum())


def _knots_for(n, located, dtype, grid):
    """Per axis: the 13-knot placement grid (`grid`) on the located axes of that length, linspace(-1, 1, n_a) elsewhere."""
    return [placement_knots(dtype, grid if (a in located and n[a] == PLACEMENT_N) else "even", n[a]) for a in range(len(n))]


def placement_free_problem(seed, n, m=(5,), dtype=np.float64, grid="even", table_dtype=None, index_base=1, identity=False):
    """Free shape (K1, K5, K7, K22, K24): every axis is located by the kernel itself.  Axis a = knots + (for D > 1) a state-only
    term over dim a + 1 with multiples {0, +1, 0, -1} h_a + a control term PLACEMENT_STEPS h_a over control dim a mod C, its
    levels rotated by a.  identity: ONE control whose displacement is +0 on every axis and no other term - the next state of
    node s is node s."""
    rng = np.random.default_rng(seed)
    D = len(n)
    m = (1,) if identity else tuple(m)
    C = len(m)
    qt = np.dtype(table_dtype or dtype)
    knots = _knots_for(n, range(D), qt, grid)
    nxt = []
    for a in range(D):
        h = _step(knots[a])
        terms = [Term((a,), knots[a].copy())]
        if identity:
            terms.append(Term((D,), np.zeros(1)))
        else:
            if D > 1:
                d = (a + 1) % D
                terms.append(Term((d,), h * _cyc((0, 1, 0, -1), n[d], a)))
            c = a % C
            terms.append(Term((D + c,), h * _cyc(PLACEMENT_STEPS, m[c], a)))
        nxt.append(terms)
    return ProblemSpec(knots, m, nxt, _placement_cost(knots, m, rng, D), dtype=dtype, index_base=index_base, table_dtype=table_dtype)


def placement_nested_problem(seed, n, m, dtype=np.float32, mono="inc", mixed_inner=False, grid="even", row=False, couple=True):
    """nested_problem's shape: control dim c drives axis D - C + c only, by PLACEMENT_STEPS h_a (the innermost control the LAST
    axis, its table increasing ('inc'), decreasing ('dec') or neither (None)); every axis also couples to up to two other state
    dims by multiples {0, 0, +1, 0, -1} h_a.  mixed_inner='only': the last axis' inner term also depends on a state dim, a
    multiple of h_a still.  row: no axis >= 1 sees state dim 0 (variant 6's rule).  The placement grid sits on the last axis
    (and on every other axis of 13 knots)."""
    rng = np.random.default_rng(seed)
    D, C = len(n), len(m)
    g = tuple(n) + tuple(m)
    knots = _knots_for(n, range(D), dtype, grid)
    nxt = []
    for a in range(D):
        h = _step(knots[a])
        terms = [Term((a,), knots[a].copy())]
        others = [d for d in range(D) if d != a and not (row and a >= 1 and d == 0)]
        if others and couple:
            pick = sorted(rng.choice(others, size=min(len(others), 2), replace=False).tolist())
            tab = rng.choice([0.0, 0.0, 1.0, 0.0, -1.0], size=tuple(g[d] for d in pick))
            terms.append(Term(pick, h * tab))
        c = a - (D - C)
        if c >= 0:
            steps = np.sort(_cyc(PLACEMENT_STEPS, g[D + c], 0 if g[D + c] >= 5 else 1))
            if c == C - 1:
                lev = steps if mono == "inc" else (steps[::-1].copy() if mono == "dec" else steps[rng.permutation(len(steps))])
                if mono is None and len(lev) > 2 and (np.all(np.diff(lev) > 0) or np.all(np.diff(lev) < 0)):
                    lev = np.concatenate([lev[1:2], lev[:1], lev[2:]])        # the permutation came out sorted: swap two levels
            else:
                lev = steps[rng.permutation(len(steps))]
            if mixed_inner == "only" and c == C - 1 and D > 1:
                d = [x for x in range(D) if x != a][0]
                terms.append(Term((d, D + c), h * (_cyc((0, 1, 0, -1), g[d])[:, None] + lev[None, :])))
            else:
                terms.append(Term((D + c,), h * lev))
        nxt.append(terms)
    return ProblemSpec(knots, m, nxt, _placement_cost(knots, m, rng, D), dtype=dtype, index_base=1)


def placement_colsweep_problem(seed, n, gax=3, dtype=np.float32, j_storage=None, a1_axis=None, a0_exact=False, index_base=1):
    """colsweep_problem's shape (variant 7), nine controls: the group axis `gax` moves by PLACEMENT_STEPS whole cells with the
    control, the window axis by {-h/2, 0, +h/2} (the middle window knot and the cell midpoint both occur).  The host groups by the
    axis that needs fewer groups (hjbdp_colsweep.hip): the (step, half-step) pairs below need five grouped by `gax` - one window
    [i - 1, i] per whole-cell step - and six grouped the other way (steps {-2, 0, 2} beside -h/2, {-2, .., 2} beside 0 / +h/2:
    three two-cell windows each), so `gax` is the axis the plan picks.  Axes 0 and 1 move with the state only, by random sub-cell
    amounts; on every third row of axis 1 (a0_exact: of axis 0 too, which rules the one-load form out wherever fl(k + h) falls
    beside a knot) by a multiple of h.  a1_axis as in colsweep_problem."""
    rng = np.random.default_rng(seed)
    assert len(n) == 4
    nU = 9
    wax = 5 - gax
    knots = _knots_for(n, (gax, wax), dtype, "even")
    hs = [_step(k) for k in knots]

    def rows(count, amp, shift, exact=True):
        r = amp * rng.uniform(-1, 1, count)
        if exact:
            r[shift % 3::3] = _cyc((1, 0, -1), len(r[shift % 3::3]), shift)
        return r

    nxt = [None] * 4
    nxt[0] = [Term((0,), knots[0].copy()), Term((2,), hs[0] * rows(n[2], 0.7, 0, a0_exact)), Term((3,), hs[0] * rows(n[3], 0.25, 1, a0_exact))]
    nxt[1] = [Term((1,), knots[1].copy()), Term((3,), hs[1] * rows(n[3], 0.6, 2)), Term((2,), hs[1] * rows(n[2], 0.2, 0))]
    if a1_axis is not None:
        nxt[1] = [Term((1,), knots[1].copy()), Term((a1_axis,), hs[1] * rows(n[a1_axis], 0.6, 2))]
    pairs = np.array([(-2, -0.5), (0, -0.5), (2, -0.5), (-2, 0.0), (0, 0.0), (2, 0.0), (-1, 0.5), (1, 0.5), (0, 0.5)])[rng.permutation(nU)]
    d, c = pairs[:, 0], pairs[:, 1]
    nxt[gax] = [Term((gax,), knots[gax].copy()), Term((4,), hs[gax] * d)]
    nxt[wax] = [Term((wax,), knots[wax].copy()), Term((4,), hs[wax] * c)]
    cu = 0.3 * np.round(rng.uniform(0, 3, nU)) ** 2
    st = {a: Term((a,), (1.0 + a) * knots[a] ** 2) for a in range(4)}
    return ProblemSpec(knots, [nU], nxt, [st[0], st[2], st[3], st[1], Term((4,), cu)], dtype=dtype, index_base=index_base,
                       j_storage=j_storage)


def placement_rate_shared_problem(seed, n_so=(8, 4, 4), n_rates=(4, 4, 13), m=(3, 3, 11), dtype=np.float32, grid="even", so_move=0.7,
                                  index_base=1, j_storage=None):
    """rate_shared_problem's shape (K15): the state-only axes as there (their product >= 128 states, K15's chunk); rate axis c moves
    by a multiple {0, 0, +1, 0, -1} h of the two other rates' indices plus a level of control dim c.  K15 and the three-plane
    window it rests on are admitted only when the inner control moves the last axis by less than a cell per level, and take their
    fast path where a sweep changes cell once: so the eleven inner levels are (j - 5) h / 8 - the sweep comes up onto the knot
    exactly at j = 5, where the cell changes - and the outer levels {-1, 0, +1/2} h: two cells, unless fl(k - h) falls one unit
    below the knot - then the point takes K15's slow path, which the same run covers."""
    rng = np.random.default_rng(seed)
    NP = len(n_so)
    n = tuple(n_so) + tuple(n_rates)
    D = len(n)
    knots = _knots_for(n, range(NP, D), dtype, grid)
    hs = [_step(k) for k in knots]
    nxt = []
    for a in range(NP):
        shape = [1] * D
        shape[a] = n[a]
        nxt.append([Term(tuple(range(D)), knots[a].reshape(shape) + so_move * hs[a] * rng.uniform(-1.0, 1.0, n))])
    for c in range(3):
        a = NP + c
        others = [NP + x for x in range(3) if x != c]
        lev = (np.arange(m[c]) - m[c] // 2) / 8.0 if c == 2 else _cyc((-1.0, 0.0, 0.5, -0.5), m[c])
        lev = np.sort(lev)
        tab = rng.choice([0.0, 0.0, 1.0, 0.0, -1.0], size=(n[others[0]], n[others[1]]))[:, :, None] + lev[None, None, :]
        nxt.append([Term((a,), knots[a].copy()), Term(tuple(others) + (D + c,), hs[a] * tab)])
    cost = [Term((NP + c,), (1.0 + c) * knots[NP + c] ** 2) for c in range(3)]
    cost.append(Term(tuple(range(NP)), 2.0 * rng.random(tuple(n_so))))
    for c in range(3):
        cost.append(Term((D + c,), 0.25 * np.round(rng.uniform(0, 3, m[c])) ** 2))
    return ProblemSpec(knots, list(m), nxt, cost, dtype=dtype, index_base=index_base, j_storage=j_storage)


def placement_local2d_problem(seed, n=(PLACEMENT_N, PLACEMENT_N), m=(4,), dtype=np.float32, table_dtype=None, j_storage=None,
                              index_base=1):
    """Local 2-D shape (K9: every query's cell is the state's own or the one below).  Axis a = knots + ONE term over (dim a, the
    control), whose entry for state i is fl(target - k_i) in the type - kept only where fl(k_i + entry) IS the target, else 0:
    level 0 stays on the node; level 1 goes onto knot i - 1 (i = 0: one step below the grid); level 2 one unit in the last place
    below knot i + 1 (i = n - 2: onto the last knot; i = n - 1: one step above the grid - both clamp to the last cell); level 3 one
    unit in the last place above knot i - 1 (odd i) or half a cell down (even i > 0).  One control dim of four levels is the
    cached form, eight levels (the four, then the four reversed) the general one."""
    rng = np.random.default_rng(seed)
    qt = np.dtype(table_dtype or dtype).type
    knots = [placement_knots(qt, "even", n[a]) for a in range(2)]
    nxt = []
    for a in range(2):
        k = knots[a].astype(qt)
        h = qt(_step(knots[a]))
        i = np.arange(n[a])
        below, above = k[np.maximum(i - 1, 0)], k[np.minimum(i + 1, n[a] - 1)]

        def entry(target):
            e = (target - k).astype(qt)
            return np.where((k + e).astype(qt) == target, e, qt(0)).astype(np.float64)

        onto = np.where(i == 0, (k - h).astype(qt), below)
        under = np.where(i == n[a] - 1, (k + h).astype(qt), np.where(i == n[a] - 2, above, np.nextafter(above, qt(-np.inf))))
        over = np.where(i == 0, k, np.where(i % 2 == 1, np.nextafter(below, qt(np.inf)), (k - (h / qt(2))).astype(qt)))
        lev = [np.zeros(n[a]), entry(onto), entry(under), entry(over)]
        tab = np.stack([lev[j % 4] if (j // 4) % 2 == 0 else lev[3 - j % 4] for j in range(m[0])], axis=1)
        terms = [Term((a,), knots[a].copy()), Term((a, 2), tab)]
        for c in range(1, len(m)):
            terms.append(Term((2 + c,), np.zeros(m[c])))
        nxt.append(terms)
    cost = [Term((0, 1), rng.random(tuple(n)))] + [Term((2 + c,), 0.25 * np.round(rng.uniform(0, 3, m[c]))) for c in range(len(m))]
    return ProblemSpec(knots, list(m), nxt, cost, dtype=dtype, index_base=index_base, table_dtype=table_dtype, j_storage=j_storage)


def assert_placement(spec, axes, grid="even", mono=None, classes=PLACEMENT_CLASSES):
    """The conditions on the INPUTS that make a placement problem worth running, per located axis in `axes`, checked in numpy
    without the library: on the even grid every class of `classes` occurs at least once; on the 'near' grid the host's deviation is
    in (1.3, 1.5) and some first guess is two or more cells off in each direction; on the 'far' grid the deviation is in (1.5, 1.7);
    mono 'inc' / 'dec': a one-sided crossing test of the LAST axis is decided at equality (placement_crossings).  Returns the
    counts per axis."""
    dt = locate_dtype(spec)
    out = {}
    for a in axes:
        k = spec.knots[a]
        assert np.array_equal(k, k.astype(dt).astype(np.float64)), a
        cnt = placement_counts(k, placement_queries(spec, a), dt)
        dev = placement_deviation(k)
        if grid == "even":
            assert dev < 0.01, (a, dev)
            for name in classes:
                assert cnt[name] >= 1, (a, name, cnt)
        elif grid == "near":
            assert 1.3 < dev < 1.5, (a, dev)
            assert cnt["guess_short2"] >= 1 and cnt["guess_far2"] >= 1, (a, cnt)
            assert cnt["outside"] >= 1, (a, cnt)
        else:
            assert 1.5 < dev < 1.7, (a, dev)
            assert cnt["outside"] >= 1, (a, cnt)
        out[a] = cnt
    if mono in ("inc", "dec"):
        hits = placement_crossings(spec, spec.D - 1, mono)
        assert hits >= 1, (mono, hits)
        out["crossings"] = hits
    return out


# ---- the placement problems the suite runs: name -> (spec builder, located axes, grid, mono, classes) ---------------------------------
# tests/test_placement_problems.py asserts assert_placement on every entry; tests/test_gpu_placements.py builds its problems through
# placement_case, which asserts it again, so a change to a generator cannot hollow a GPU case out unnoticed.
_EDGE = ("on_knot", "first_knot", "last_knot", "outside")                       # what half-cell steps can reach (the window axis)
_LOCAL = PLACEMENT_CLASSES[:6]                                                  # what a local problem can reach (K9's rule)
FREE_SHAPES = {1: ((13,), (5,)), 2: ((13, 13), (5, 5)), 4: ((13, 3, 4, 13), (5, 5)), 6: ((13, 3, 3, 3, 3, 13), (5, 1, 5))}
NESTED_SHAPES = {2: ((13, 13), (5,)), 3: ((5, 13, 13), (3, 5, 5)), 5: ((4, 3, 4, 13, 13), (3, 5, 5)), 6: ((4, 3, 4, 3, 3, 13), (3, 3, 5))}
ROW_SHAPE = ((70, 13, 13), (5, 5))
COLSWEEP_SHAPE = {3: (8, 5, 13, 13), 2: (8, 5, 13, 13)}
PLACEMENT_CASES = {}


def _thirteen(n):
    return tuple(a for a in range(len(n)) if n[a] == PLACEMENT_N)


def _register():
    f32, f64 = np.float32, np.float64
    for dt in (f32, f64):
        t = np.dtype(dt).name
        for D, (n, m) in FREE_SHAPES.items():
            PLACEMENT_CASES["free-%d-%s" % (D, t)] = (lambda n=n, m=m, dt=dt, D=D: placement_free_problem(10 + D, n, m, dtype=dt),
                                                      _thirteen(n), "even", None, PLACEMENT_CLASSES)
        for grid in ("near", "far"):
            PLACEMENT_CASES["free-2-%s-%s" % (t, grid)] = (lambda dt=dt, grid=grid: placement_free_problem(20, (13, 13), (5, 5), dtype=dt, grid=grid),
                                                           (0, 1), grid, None, PLACEMENT_CLASSES)
        for D in (2, 4):
            n = FREE_SHAPES[D][0]
            PLACEMENT_CASES["identity-%d-%s" % (D, t)] = (lambda n=n, dt=dt: placement_free_problem(30, n, dtype=dt, identity=True),
                                                          _thirteen(n), "even", None, ("on_knot", "first_knot", "last_knot"))
        for D in (2, 3, 6) if dt == f64 else (2, 3, 5, 6):
            n, m = NESTED_SHAPES[D]
            for mono in ("inc", "dec", None):
                PLACEMENT_CASES["nested-%d-%s-%s" % (D, t, mono)] = (
                    lambda n=n, m=m, dt=dt, mono=mono, D=D: placement_nested_problem(40 + D, n, m, dtype=dt, mono=mono),
                    _thirteen(n), "even", mono, PLACEMENT_CLASSES)
        for grid in ("near", "far"):
            PLACEMENT_CASES["nested-3-%s-inc-%s" % (t, grid)] = (
                lambda dt=dt, grid=grid: placement_nested_problem(43, *NESTED_SHAPES[3], dtype=dt, mono="inc", grid=grid),
                (1, 2), grid, "inc", PLACEMENT_CLASSES)
        PLACEMENT_CASES["row-%s" % t] = (lambda dt=dt: placement_nested_problem(50, *ROW_SHAPE, dtype=dt, mono="inc", row=True),
                                         (1, 2), "even", "inc", PLACEMENT_CLASSES)
    PLACEMENT_CASES["free-2-tab64"] = (lambda: placement_free_problem(12, (13, 13), (5, 5), dtype=f32, table_dtype=f64),
                                       (0, 1), "even", None, PLACEMENT_CLASSES)
    for D in (2, 3, 5, 6):
        n, m = NESTED_SHAPES[D]
        for mono in ("inc", "dec"):
            PLACEMENT_CASES["mixed-%d-%s" % (D, mono)] = (
                lambda n=n, m=m, mono=mono, D=D: placement_nested_problem(60 + D, n, m, dtype=f32, mono=mono, mixed_inner="only"),
                (len(n) - 1,), "even", mono, PLACEMENT_CLASSES)
    for gax in (2, 3):
        for sto in (None, np.float16):
            for coop in (False, True):
                name = "colsweep-g%d-%s%s" % (gax, "f16" if sto else "f32", "-coop" if coop else "")
                PLACEMENT_CASES[name] = (lambda gax=gax, sto=sto, coop=coop: placement_colsweep_problem(
                    70 + gax, COLSWEEP_SHAPE[gax], gax=gax, j_storage=sto, a1_axis=gax if coop else None), (gax,), "even", None,
                    PLACEMENT_CLASSES)
        PLACEMENT_CASES["colsweep-g%d-f32-a0" % gax] = (lambda gax=gax: placement_colsweep_problem(
            75 + gax, COLSWEEP_SHAPE[gax], gax=gax, a0_exact=True), (gax,), "even", None, PLACEMENT_CLASSES)
    for grid in ("even", "near", "far"):
        PLACEMENT_CASES["rates-%s" % grid] = (lambda grid=grid: placement_rate_shared_problem(80, grid=grid), (5,), grid,
                                              "inc" if grid == "even" else None, PLACEMENT_CLASSES)
    for typing, kw in (("f32", dict(dtype=f32)), ("f64", dict(dtype=f64)), ("tab64", dict(dtype=f32, table_dtype=f64))):
        for m in ((4,), (8,)):
            PLACEMENT_CASES["local2d-%s-u%d" % (typing, m[0])] = (lambda kw=kw, m=m: placement_local2d_problem(90, m=m, **kw), (0, 1),
                                                                  "even", None, _LOCAL)


_register()


def placement_case(name):
    """-> (spec, counts): the registered problem, its input conditions asserted (assert_placement); for the column-sweep shape the
    window axis too: queries on a knot, on the first and the last one, outside, and on a cell midpoint."""
    build, axes, grid, mono, classes = PLACEMENT_CASES[name]
    spec = build()
    counts = assert_placement(spec, axes, grid, mono, classes)
    if name.startswith("colsweep"):
        wax = 5 - axes[0]
        if grid == "even":
            counts.update(assert_placement(spec, (wax,), "even", None, _EDGE))
            dt = locate_dtype(spec).type
            k = spec.knots[wax].astype(dt)
            q = np.asarray(placement_queries(spec, wax)).astype(dt)
            c = placement_cells(k, q)
            assert np.any((q - k[c]).astype(dt) == (k[c + 1] - q).astype(dt)), "no query on a cell midpoint of the window axis"
    return spec, counts
