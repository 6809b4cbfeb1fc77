"""GPU tests (-m gpu): K9, the several-stages-per-launch kernels of local 2-D problems (csrc/kernels_tile2d.h), at their tile, halo
and launch-count edges.

K9 keeps a 16 x 8 tile of J plus a halo of 8 cells in LDS and performs up to eight backups per launch; only the last stage of a
launch leaves the CU.  A state computed from a stale or unloaded patch cell is therefore a finite, plausible J that is carried
forward, and the host check that lets K9 run at all (examine_tile2d, csrc/hjbdp_tables.hip) decides from the (cell, weight) tables
that no query leaves the state's own cell or the one below.  Both are checked here the only way that sees such faults: J and labels
of the LAST stage bit for bit against the C oracle's one-stage-at-a-time sweep (c_oracle.sweep) - under option temporal = 2, which
makes hjb_solve fail unless K9 is the path that ran, under temporal = 0 on the same handle, and in the fall-back cases under the
default temporal = 1.  Labels also lie in [index_base, index_base + nU).  No tolerance appears anywhere.

Problems come from one generator (_problem) whose arithmetic is exact: knots are small integers times a power of two (cell widths
1, or 1 / 2 / 4 in the non-uniform variant), every next-state term is a dyadic fraction of the local cell width, and every partial
sum of a query is asserted to be a float32 value.  The interpolation cell of every (state, control) is therefore recomputed in numpy
(the same for float32 and float64 problems and tables) and every case asserts on the CPU what it stands for: _is_local restates
examine_tile2d's rule, positive cases are local, boundary cases are non-local by exactly one entry.  Costs and terminals are random
and of order one (terminals rounded to the J storage type first), so that a wrong halo cell is still visible after 16 stages.

Covered: both forms (cached: one control dim, nU 1 .. 4; general: nU 5 and 64, two and three control dims) under a rotation of
typings (f32, f64, f16 storage, float64-built tables), label types and index bases; last-launch depths 1, 2, 3, 7 and 0, even and
odd launch counts; graph replay at 63 / 64 / 65 / 95 / 96 stages, further solves on one handle and the temporal 2 -> 0 -> 2 switch;
grids from 2 x 2 to one state past two tiles; drift through all four patch corners on uniform and non-uniform knots; one- and
three-dimensional table domains; exact ties; the edge of applicability on both axes, in full and in reduced table domains; and every hjb_solve condition that must
switch K9 off.

Not covered: problems larger than 40 x 40 or sweeps longer than 100 stages (tests/test_gpu_parity.py and test_gpu_solvers.py run
the solvers' own shapes), A/B builds with other tile sizes (-DHJB_TILE_X/Y/K), and which of the two forms a launch took - no option
reports it; it follows from C and nU (stage_tile2d: the cached form when its plan exists), which every case asserts from its inputs.
A slab handle cannot be swept by hjb_solve at all (whatever `temporal` says): its fall-back check is one stage against the oracle.

Wall time of the default `-m gpu` run on one MI355X box, runs back to back (tests/conftest.py states a 540 s budget):
389 s at the parent commit (732 tests), 391 s with this file (865 tests) - the difference is the box's run-to-run noise; this file's
133 device tests take 1.1 s when run alone (0.2 s the slowest, the first, which loads the library), so nothing of it is `extended`."""
import functools

import numpy as np
import pytest

gpu = pytest.mark.gpu            # (not a module mark: the input-condition tests at the end need no device)

TILE_X, TILE_Y, TILE_K = 16, 8, 8         # csrc/kernels_tile2d.h: owned states per workgroup, stages per launch
MAX_CACHED_U = 4                          # kTileMaxU: the cached form keeps up to four controls in registers
GRAPH_STAGES = 32                         # kGraphStages: stages per graph replay (four K9 launches); replay from 2 x 32 stages up


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi, c_oracle


# ---- the problem generator --------------------------------------------------------------------------------------------------------
TYPINGS = {"f32": dict(dtype=np.float32), "f64": dict(dtype=np.float64), "f16s": dict(dtype=np.float32, j_storage=np.float16),
           "tab64": dict(dtype=np.float32, table_dtype=np.float64)}
LABELS = (np.uint8, np.uint16, np.int32)


def _problem(n, m, moves, seed, typing="f32", idx_dtype=np.int32, index_base=1, nonuniform=False, scale=2.0 ** -3, ties=False,
             own=(True, True), **spec_kw):
    """A 2-D problem with exact next-state arithmetic -> (spec, cells, terminal).

    Axis a's next state is knots[a] (unless own[a] is False) plus the terms of moves[a], each (dims, frac): frac, an array over the
    grid dims `dims` (states 0 / 1, controls 2 ..), is the displacement in units of the LOCAL cell width - the cell above the state
    for frac >= 0, the cell below for frac < 0 (needs a in dims on a non-uniform axis); (dims, data, "abs") is an absolute term in
    units of `scale`.  cells[a] over (n0, n1, *m) is the interpolation cell of every query: upper_bound(knots, q) - 1 clamped to
    [0, n - 2], on queries whose every partial sum is asserted to be a float32 value."""
    import hjbdp
    from hjbdp import Term
    rng = np.random.default_rng(seed)
    n, m = tuple(n), tuple(m)
    g = n + m
    nxt, cells, knots = [], [], []
    for a in range(2):
        w = (rng.choice([1, 2, 4], n[a] - 1) if nonuniform else np.ones(n[a] - 1)) * scale
        k = np.concatenate([[0.0], np.cumsum(w)])
        k = k - k[n[a] // 2]
        knots.append(k)
        i = np.arange(n[a])
        up, dn = w[np.minimum(i, n[a] - 2)], w[np.maximum(i - 1, 0)]
        terms = [Term((a,), k)] if own[a] else []
        for mv in moves[a]:
            dims, frac = tuple(mv[0]), np.asarray(mv[1], dtype=np.float64)
            assert frac.shape == tuple(g[d] for d in dims), (a, dims, frac.shape)
            if len(mv) == 3:
                assert mv[2] == "abs"
                terms.append(Term(dims, frac * scale))
            elif a in dims:
                sh = [-1 if d == a else 1 for d in dims]
                terms.append(Term(dims, frac * np.where(frac >= 0, up.reshape(sh), dn.reshape(sh))))
            else:
                assert np.all(w == w[0]), "a term that does not see x_a cannot follow a non-uniform axis' cell widths"
                terms.append(Term(dims, frac * w[0]))
        q = None
        for t in terms:                                    # the library's own left-to-right sum, every step exact in float32
            x = t.data.reshape([g[d] if d in t.dims else 1 for d in range(len(g))])
            q = x if q is None else q + x
            assert np.array_equal(q, q.astype(np.float32).astype(np.float64)), (a, t.dims, "a partial sum is no float32 value")
        q = np.broadcast_to(q, g)
        cells.append(np.clip(np.searchsorted(k, q, side="right") - 1, 0, n[a] - 2))
        nxt.append(terms)
    if ties:                                               # controls without effect on the cost
        cost = [Term((0, 1), rng.random(n))] + [Term((2 + c,), np.full(m[c], 0.5)) for c in range(len(m))]
    else:
        cost = ([Term((0, 1), rng.random(n))] + [Term((2 + c,), rng.random(m[c])) for c in range(len(m))] +
                [Term((1, 2), 0.5 * rng.random((n[1], m[0])))])
    kw = dict(TYPINGS[typing], idx_dtype=idx_dtype, index_base=index_base)
    kw.update(spec_kw)
    spec = hjbdp.ProblemSpec(knots, list(m), nxt, cost, **kw)
    term = (2.0 * rng.random(spec.nS)).astype(spec.j_dtype)
    return spec, cells, term


def _local_moves(n, m, seed, nonuniform=False):
    """Random local dynamics: axis a moves by a term over the other state (at most 6/16 of a cell) and one term per control dim
    (8/16 of a cell between them): the total stays inside (-1, 1) cells.  On non-uniform knots every term also spans x_a."""
    rng = np.random.default_rng(seed + 1000)
    g = tuple(n) + tuple(m)
    b = 8 // len(m)
    moves = []
    for a in range(2):
        sd = (0, 1) if nonuniform else (1 - a,)
        ms = [(sd, rng.integers(-6, 7, [g[d] for d in sd]) / 16.0)]
        for c in range(len(m)):
            cd = (a, 2 + c) if nonuniform else (2 + c,)
            ms.append((cd, rng.integers(-b, b + 1, [g[d] for d in cd]) / 16.0))
        moves.append(ms)
    return moves


def _total(n, m, moves_a):
    """The summed displacement of one axis over the full (n0, n1, *m) grid, in cells."""
    g = tuple(n) + tuple(m)
    tot = np.zeros(g)
    for dims, frac in moves_a:
        tot = tot + np.asarray(frac, dtype=np.float64).reshape([g[d] if d in dims else 1 for d in range(len(g))])
    return tot


def _outside(cells):
    """How many (axis, state, control) entries break examine_tile2d's rule: cell in [max(i - 1, 0), min(i, n - 2)] on both axes."""
    bad = 0
    for a, c in enumerate(cells):
        na = c.shape[a]
        i = np.arange(na).reshape([-1 if d == a else 1 for d in range(c.ndim)])
        lo, hi = np.maximum(i - 1, 0), np.minimum(i, na - 2)
        bad += int(np.count_nonzero((c < lo) | (c > hi)))
    return bad


def _is_local(cells):
    return _outside(cells) == 0


def _form(spec):
    """Which K9 kernel serves the spec (examine_tile2d builds the cached form's plan for one control dim of at most four values)."""
    return "cached" if spec.C == 1 and spec.nU <= MAX_CACHED_U else "general"


def _tiles(n):
    return -(-n[0] // TILE_X) * -(-n[1] // TILE_Y)


def _launch_depths(n_stages):
    """The K of every K9 launch of a sweep (hjb_solve: whole graphs first, then launches of up to eight stages)."""
    return [TILE_K] * (n_stages // TILE_K) + ([n_stages % TILE_K] if n_stages % TILE_K else [])


# ---- the checker ------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _assert_equal(out, ref, spec, what, n_stages=None):
    assert n_stages is None or out["stages_done"] == n_stages, (what, out["stages_done"])
    assert out["J"].dtype == spec.j_dtype and out["idx"].dtype == spec.idx_np_dtype, what
    bad = np.flatnonzero(_bits(out["J"]) != _bits(ref["J"]))
    assert bad.size == 0, (what, "J", bad.size, bad[:8], out["J"][bad[:4]], ref["J"][bad[:4]])
    bad = np.flatnonzero(out["idx"].astype(np.int64) != ref["idx"])
    assert bad.size == 0, (what, "labels", bad.size, bad[:8], out["idx"][bad[:4]], ref["idx"][bad[:4]])
    assert out["idx"].min() >= spec.index_base and out["idx"].max() < spec.index_base + spec.nU, what


def _oracle(env, spec, n_stages, term, **kw):
    _, _abi, c_oracle = env
    ref = c_oracle.sweep(_abi, spec, n_stages, terminal=term, nthreads=8, **kw)
    assert np.isfinite(ref["J"].astype(np.float64)).all(), "the oracle's sweep is not finite: not a case bit equality can check"
    return ref


def _k9_and_stagewise(env, prob, stage_counts, what):
    """One handle: every count under temporal = 2 (K9 or an error), then every count under temporal = 0, against the oracle."""
    hjbdp = env[0]
    spec, cells, term = prob
    assert _is_local(cells), what
    refs = {k: _oracle(env, spec, k, term) for k in stage_counts}
    outs = {}
    with hjbdp.Backup(spec) as bk:
        for temporal in (2, 0):
            bk.set_option("temporal", temporal)
            for k in stage_counts:
                assert k >= 2 * TILE_K
                outs[temporal, k] = bk.solve(k, terminal=term)
                _assert_equal(outs[temporal, k], refs[k], spec, (what, "temporal %d" % temporal, k), k)
    return outs


def _refused(env, bk, *args, **kw):
    hjbdp, _abi, _ = env
    with pytest.raises(hjbdp.HjbError) as ei:
        bk.solve(*args, **kw)
    assert ei.value.status == _abi.HJB_E_UNSUPPORTED, str(ei.value)


# ---- 1. both forms at every control count, typing, label type and index base -------------------------------------------------------
GRID_3X3 = (33, 17)                       # 3 x 3 tiles, each axis one state past a tile
CONTROLS = [(1,), (2,), (3,), (4,), (5,), (64,), (2, 2), (2, 2, 2)]


def _rotation():
    cases = []
    for r in (0, 1):                       # two turns of the rotation; the second on non-uniform knots
        for i, m in enumerate(CONTROLS):
            cases.append((m, list(TYPINGS)[(i + r) % 4], LABELS[(i + 2 * r) % 3], (i + r) % 2, bool(r)))
    return cases


ROTATION = _rotation()


def _rotation_id(c):
    return "m%s-%s-%s-base%d-%s" % ("x".join(map(str, c[0])), c[1], np.dtype(c[2]).name, c[3], "nonuniform" if c[4] else "uniform")


def _rotation_problem(case):
    m, typing, idx_dtype, base, nonuniform = case
    return _problem(GRID_3X3, m, _local_moves(GRID_3X3, m, 11 + len(m), nonuniform), 100 + int(np.prod(m)), typing=typing,
                    idx_dtype=idx_dtype, index_base=base, nonuniform=nonuniform)


@gpu
@pytest.mark.parametrize("case", ROTATION, ids=_rotation_id)
def test_both_forms_at_every_control_count(env, case):
    """19 stages = 8 + 8 + 3 on 3 x 3 tiles: the `u < nU` guards of the cached form for nU = 1 .. 3, the general form's control
    odometer and label composition for one, two and three control dims."""
    prob = _rotation_problem(case)
    spec = prob[0]
    assert _tiles(spec.n) == 9 and spec.n[0] % TILE_X == 1 and spec.n[1] % TILE_Y == 1
    assert _form(spec) == ("cached" if case[0] in [(1,), (2,), (3,), (4,)] else "general")
    assert spec.idx_np_dtype == np.dtype(case[2]) and spec.index_base == case[3] and spec.index_base + spec.nU - 1 <= 255
    assert (spec.table_dtype == np.float64) == (case[1] == "tab64") and (spec.j_dtype == np.float16) == (case[1] == "f16s")
    _k9_and_stagewise(env, prob, [19], _rotation_id(case))


def test_every_factor_met_both_forms_were_exercised():
    """From the parameter list: every control count, and for each of the two forms every typing, label type and index base."""
    met = {"cached": [set(), set(), set(), set()], "general": [set(), set(), set(), set()]}
    for m, typing, idx_dtype, base, nonuniform in ROTATION:
        form = "cached" if len(m) == 1 and m[0] <= MAX_CACHED_U else "general"
        for s, v in zip(met[form], (m, typing, np.dtype(idx_dtype), base)):
            s.add(v)
    assert met["cached"][0] == {(1,), (2,), (3,), (4,)} and met["general"][0] == {(5,), (64,), (2, 2), (2, 2, 2)}, met
    for form, (_, typings, labels, bases) in met.items():
        assert typings == set(TYPINGS) and labels == {np.dtype(x) for x in LABELS} and bases == {0, 1}, (form, met[form])
    assert {c[4] for c in ROTATION} == {False, True}


# ---- 2. / 3. launch depth, ping-pong parity, graph replay ---------------------------------------------------------------------------
GRID_2X2 = (17, 9)                        # 2 x 2 tiles, each axis one state past a tile


@functools.lru_cache(maxsize=None)
def _pair(form):
    """The two problems of the launch-count cases: cached (3 controls, f32, uint8 labels from 1) and general (5 controls, f64,
    int32 labels from 0)."""
    if form == "cached":
        return _problem(GRID_2X2, (3,), _local_moves(GRID_2X2, (3,), 21), 201, typing="f32", idx_dtype=np.uint8, index_base=1)
    return _problem(GRID_2X2, (5,), _local_moves(GRID_2X2, (5,), 22), 202, typing="f64", idx_dtype=np.int32, index_base=0)


_REFS = {}


def _pair_ref(env, form, n_stages):
    if (form, n_stages) not in _REFS:
        spec, _, term = _pair(form)
        _REFS[form, n_stages] = _oracle(env, spec, n_stages, term)
    return _REFS[form, n_stages]


DEPTH_STAGES = [16, 17, 18, 19, 23, 24, 25, 31, 32, 33]
GRAPH_STAGE_COUNTS = [63, 64, 65, 95, 96]


def _pair_check(env, form, n_stages):
    hjbdp = env[0]
    spec, cells, term = _pair(form)
    assert _is_local(cells) and _form(spec) == form and _tiles(spec.n) == 4
    ref = _pair_ref(env, form, n_stages)
    with hjbdp.Backup(spec) as bk:
        for temporal in (2, 0):
            bk.set_option("temporal", temporal)
            _assert_equal(bk.solve(n_stages, terminal=term), ref, spec, (form, n_stages, "temporal %d" % temporal), n_stages)


@gpu
@pytest.mark.parametrize("form", ["cached", "general"])
@pytest.mark.parametrize("n_stages", DEPTH_STAGES)
def test_last_launch_depth_and_final_buffer(env, n_stages, form):
    assert 2 * TILE_K <= n_stages < 2 * GRAPH_STAGES                 # K9 applies, no graph
    _pair_check(env, form, n_stages)


def test_launch_depths_were_exercised():
    depths = {k: _launch_depths(k) for k in DEPTH_STAGES}
    assert {d[-1] for d in depths.values()} >= {1, 2, 3, 7, 8}, depths           # the last launch's K
    assert {len(d) % 2 for d in depths.values()} == {0, 1}, depths               # the final J in either ping-pong buffer
    assert {len(d) % 2 for d in depths.values() if d[-1] == 8} == {0, 1}, depths  # ... also when the count ends on a launch boundary


@gpu
@pytest.mark.parametrize("form", ["cached", "general"])
@pytest.mark.parametrize("n_stages", GRAPH_STAGE_COUNTS)
def test_graph_replay_edges(env, n_stages, form):
    """63: no graph; 64: two replays and nothing after; 65: one K = 1 launch after them; 95: 8 + 8 + 8 + 7 after; 96: three."""
    after = {63: None, 64: [], 65: [1], 95: [8, 8, 8, 7], 96: []}[n_stages]
    if n_stages < 2 * GRAPH_STAGES:
        assert after is None
    else:
        assert _launch_depths(n_stages % GRAPH_STAGES) == after and n_stages // GRAPH_STAGES >= 2
    _pair_check(env, form, n_stages)


@gpu
@pytest.mark.parametrize("form", ["cached", "general"])
def test_one_handle_across_counts_and_temporal_switches(env, form):
    """95, 64 and 17 stages on one handle (the graph of the first solve serves the second; the third has none), then temporal
    2 -> 0 -> 2 with 65 stages after each switch: the graph of K9 launches must not be replayed for the stage kernel, nor back."""
    hjbdp = env[0]
    spec, cells, term = _pair(form)
    assert _is_local(cells)
    with hjbdp.Backup(spec) as bk:
        bk.set_option("temporal", 2)
        for k in (95, 64, 17):
            _assert_equal(bk.solve(k, terminal=term), _pair_ref(env, form, k), spec, (form, "temporal 2", k), k)
        for temporal in (0, 2):
            bk.set_option("temporal", temporal)
            assert bk.get_option("temporal") == temporal
            _assert_equal(bk.solve(65, terminal=term), _pair_ref(env, form, 65), spec, (form, "after the switch to", temporal), 65)


# ---- 4. grid extents ---------------------------------------------------------------------------------------------------------------
EXTENTS = [(2, 2), (2, 40), (40, 2), (5, 3), (15, 7), (16, 8), (17, 9), (31, 16), (32, 17)]


def _extent_problem(n, form):
    m = (3,) if form == "cached" else (6,)
    return _problem(n, m, _local_moves(n, m, 31 + n[0]), 300 + 41 * n[0] + n[1], typing="f32" if n[0] % 2 else "f64",
                    idx_dtype=np.uint8, index_base=1)


@gpu
@pytest.mark.parametrize("form", ["cached", "general"])
@pytest.mark.parametrize("n", EXTENTS, ids=lambda n: "%dx%d" % n)
def test_grid_extents(env, n, form):
    """17 (8 + 8 + 1) and 24 stages at the minimum grid, grids smaller than the halo, one state short of a tile, a whole tile (one
    workgroup), one state past it, and the same around two tiles."""
    prob = _extent_problem(n, form)
    assert _form(prob[0]) == form
    assert _tiles(n) == {(2, 2): 1, (2, 40): 5, (40, 2): 3, (5, 3): 1, (15, 7): 1, (16, 8): 1, (17, 9): 4, (31, 16): 4, (32, 17): 6}[n]
    _k9_and_stagewise(env, prob, [17, 24], (n, form))


def test_extents_stand_for_their_edges():
    assert any(n[0] < TILE_K and n[1] < TILE_K for n in EXTENTS)                              # smaller than the halo on both axes
    assert (TILE_X, TILE_Y) in EXTENTS and _tiles((TILE_X, TILE_Y)) == 1                      # a launch of one workgroup
    for d in (-1, 1):                                                                         # one state short of / past a tile
        assert (TILE_X + d, TILE_Y + d) in EXTENTS
    assert (2 * TILE_X - 1, 2 * TILE_Y) in EXTENTS and (2 * TILE_X, 2 * TILE_Y + 1) in EXTENTS  # ... and around two tiles
    assert min(min(n) for n in EXTENTS) == 2 and max(max(n) for n in EXTENTS) == 40
    for n in EXTENTS:
        for form in ("cached", "general"):
            assert _is_local(_extent_problem(n, form)[1]), (n, form)


# ---- 5. drift through the patch corner, table domains -------------------------------------------------------------------------------
DRIFTS = [(s0, s1, d, False) for s0 in (1, -1) for s1 in (1, -1) for d in (0.75, 0.25)] + \
         [(s0, s1, (0.75 if s0 == s1 else 0.25), True) for s0 in (1, -1) for s1 in (1, -1)]


def _drift_problem(case, form):
    s0, s1, d, nonuniform = case
    m = (3,) if form == "cached" else (5,)
    moves = [[((0,), np.full(GRID_3X3[0], s0 * d))], [((1,), np.full(GRID_3X3[1], s1 * d))]]
    return _problem(GRID_3X3, m, moves, 400 + int(8 * d) + 3 * s0 + s1, typing="f32", idx_dtype=np.int32, index_base=1,
                    nonuniform=nonuniform)


def _drift_cells_ok(case, cells):
    """Every state reads its own cell (drift up) or the one below (drift down), clamped: after eight stages J at a tile's corner
    depends on the state eight cells away diagonally, the extreme corner of the halo."""
    ok = True
    for a, s in enumerate(case[:2]):
        na = cells[a].shape[a]
        i = np.arange(na).reshape([-1 if d == a else 1 for d in range(cells[a].ndim)])
        ok = ok and np.array_equal(cells[a], np.broadcast_to(np.clip(i if s > 0 else i - 1, 0, na - 2), cells[a].shape))
    return ok


@gpu
@pytest.mark.parametrize("form", ["cached", "general"])
@pytest.mark.parametrize("case", DRIFTS, ids=lambda c: "%+d%+d-%g-%s" % (c[0], c[1], c[2], "nonuniform" if c[3] else "uniform"))
def test_drift_through_the_patch_corner(env, case, form):
    prob = _drift_problem(case, form)
    assert _form(prob[0]) == form and _drift_cells_ok(case, prob[1])
    _k9_and_stagewise(env, prob, [16], (case, form))


def _domain_problem(kind, form):
    """own: x0+ depends on x0 alone (a one-dimensional table domain beside a full one); ctrl: x0+ = f(x0, u) and x1+ = f(x1, x0)
    (domains (0, 2) and (0, 1): the control's stride in one table is n0, a state's stride in the other is n0 too)."""
    n = GRID_3X3
    m = (3,) if form == "cached" else (5,)
    rng = np.random.default_rng(55)
    full = _local_moves(n, m, 56)
    if kind == "own":
        moves = [[((0,), rng.integers(-14, 15, n[0]) / 16.0)], full[1]]
    else:
        moves = [[((0,), rng.integers(-6, 7, n[0]) / 16.0), ((2,), rng.integers(-8, 9, m[0]) / 16.0)],
                 [((1,), rng.integers(-6, 7, n[1]) / 16.0), ((0,), rng.integers(-8, 9, n[0]) / 16.0)]]
    return _problem(n, m, moves, 500 + len(kind), typing="tab64" if kind == "own" else "f32", idx_dtype=np.uint16, index_base=0), moves


@gpu
@pytest.mark.parametrize("form", ["cached", "general"])
@pytest.mark.parametrize("kind", ["own", "ctrl"])
def test_table_domain_strides(env, kind, form):
    prob, moves = _domain_problem(kind, form)
    dims = [sorted({a} | {d for mv in moves[a] for d in mv[0]}) for a in range(2)]
    assert dims == ([[0], [0, 1, 2]] if kind == "own" else [[0, 2], [0, 1]]), dims
    _k9_and_stagewise(env, prob, [16, 21], (kind, form))


# ---- 6. ties ------------------------------------------------------------------------------------------------------------------------
def _ties_problem(m):
    return _problem(GRID_2X2, m, [[((1,), np.full(GRID_2X2[1], 0.5))], [((0,), np.full(GRID_2X2[0], -0.25))]], 600 + len(m),
                    typing="f32", idx_dtype=np.uint8, index_base=1, ties=True)


@gpu
@pytest.mark.parametrize("m", [(4,), (7,), (2, 3)], ids=lambda m: "x".join(map(str, m)))
def test_exact_ties_keep_the_first_control(env, m):
    """Controls without effect and of equal cost: the strict `<` keeps control 0 everywhere, in both forms."""
    spec, cells, term = prob = _ties_problem(m)
    flat = [c.reshape(c.shape[0], c.shape[1], -1) for c in cells]
    assert all(np.all(c == c[:, :, :1]) for c in flat)                   # no control moves a query
    assert all(np.all(t.data == t.data.flat[0]) for t in spec.cost_terms if max(t.dims) >= 2)
    outs = _k9_and_stagewise(env, prob, [17], ("ties", m))
    assert all(np.all(o["idx"] == spec.index_base) for o in outs.values()), m


# ---- 7. the edge of applicability ---------------------------------------------------------------------------------------------------
EDGE_GRID = (40, 20)                      # the last tile of either axis has an interior: states 32 .. 39, 16 .. 19


def _edge_problem(kind, axis, form):
    """A local base problem over the full (x0, x1, u) domain on both axes, bent at chosen entries of `axis` by a last term over
    that full domain so that the TOTAL displacement there is an exact number of cells."""
    n = EDGE_GRID
    m = (3,) if form == "cached" else (5,)
    g = n + m
    if kind == "minus_one_everywhere":
        moves = [[((0,), np.full(n[0], -1.0))], [((1,), np.full(n[1], -1.0))]]
        return _problem(n, m, moves, 700, typing="f32", idx_dtype=np.uint8)
    moves = _local_moves(n, m, 71)
    na = n[axis]
    i = np.arange(na).reshape([-1 if d == axis else 1 for d in range(3)])
    at = np.zeros(g, dtype=bool)
    entry = [(36, 17, m[0] - 1), (3, 17, m[0] - 1)][axis]           # (x0, x1, u): inside the last tile of `axis`, below n - 2
    if kind == "plus_one_at_n_minus_2":
        both = []
        for a in range(2):                                          # at every entry of state n - 2, on each axis
            ia = np.arange(n[a]).reshape([-1 if d == a else 1 for d in range(3)])
            both.append(np.broadcast_to(ia == n[a] - 2, g))
        bent = [moves[a] + [((0, 1, 2), np.where(both[a], 1.0 - _total(n, m, moves[a]), 0.0))] for a in range(2)]
        return _problem(n, m, bent, 701, typing="f32", idx_dtype=np.uint8)
    if kind == "plus_five_from_the_top_two":
        at[:] = np.broadcast_to(i >= na - 2, g)
        target = 5.0
    elif kind == "plus_one_inside_the_last_tile":
        at[entry] = True
        target = 1.0
    elif kind == "plus_five_from_n_minus_3":
        entry = tuple(na - 3 if d == axis else e for d, e in enumerate(entry))
        at[entry] = True
        target = 5.0
    elif kind == "minus_two":
        at[entry] = True
        target = -2.0
    else:
        raise ValueError(kind)
    bent = list(moves)
    bent[axis] = moves[axis] + [((0, 1, 2), np.where(at, target - _total(n, m, moves[axis]), 0.0))]
    return _problem(n, m, bent, 702 + axis, typing="f32" if axis else "f64", idx_dtype=np.uint8)


LOCAL_EDGES = [("minus_one_everywhere", 0), ("plus_one_at_n_minus_2", 0), ("plus_five_from_the_top_two", 0),
               ("plus_five_from_the_top_two", 1)]
NONLOCAL_EDGES = [(k, a) for k in ("plus_one_inside_the_last_tile", "plus_five_from_n_minus_3", "minus_two") for a in (0, 1)]


@gpu
@pytest.mark.parametrize("form", ["cached", "general"])
@pytest.mark.parametrize("kind,axis", LOCAL_EDGES, ids=["%s-axis%d" % e for e in LOCAL_EDGES])
def test_queries_on_the_edge_of_the_rule_run_k9(env, kind, axis, form):
    """A query exactly on the knot below (t = 0), exactly on the last knot from state n - 2 (clamped to the top cell, t = 1), and
    far above the grid from the top two states (clamped into the state's own cell) are all local: K9 runs and is right."""
    _k9_and_stagewise(env, _edge_problem(kind, axis, form), [17], (kind, axis, form))


@gpu
@pytest.mark.parametrize("form", ["cached", "general"])
@pytest.mark.parametrize("kind,axis", NONLOCAL_EDGES, ids=["%s-axis%d" % e for e in NONLOCAL_EDGES])
def test_one_entry_past_the_rule_switches_k9_off(env, kind, axis, form):
    """One (state, control) entry of one axis' table one cell past the rule: required K9 is refused, the default is the oracle's."""
    hjbdp = env[0]
    spec, cells, term = _edge_problem(kind, axis, form)
    assert _outside(cells) == 1 and _outside(_only(cells, axis)) == 1 and _is_local(_only(cells, 1 - axis))
    ref = _oracle(env, spec, 17, term)
    with hjbdp.Backup(spec) as bk:
        bk.set_option("temporal", 2)
        _refused(env, bk, 17, terminal=term)
        bk.set_option("temporal", 1)
        _assert_equal(bk.solve(17, terminal=term), ref, spec, (kind, axis, form, "default"), 17)


def _only(cells, a):
    """cells with the other axis replaced by one that is trivially local (every state in its own cell)."""
    other = 1 - a
    no = cells[other].shape[other]
    i = np.arange(no).reshape([-1 if d == other else 1 for d in range(cells[other].ndim)])
    triv = np.broadcast_to(np.minimum(i, no - 2), cells[other].shape)
    return [cells[0], triv] if a == 0 else [triv, cells[1]]


REDUCED_DOMAINS = {0: (0, 2), 1: (0, 1)}       # the table domains of _domain_problem("ctrl"): x0+ = f(x0, u), x1+ = f(x1, x0)


def _reduced_nonlocal_problem(axis, form):
    """_domain_problem("ctrl") bent at ONE entry of `axis`' reduced table domain by a last term over that domain: +1 cell at
    (x0 = 20, the last control) of axis 0's (x0, u) table, -2 cells at (x0 = 5, x1 = 10) of axis 1's (x0, x1) table, where the
    entry's own-axis index is e / n0 and not e % n0."""
    n = GRID_3X3
    m = (3,) if form == "cached" else (5,)
    g = n + m
    moves = _domain_problem("ctrl", form)[1]
    dims = REDUCED_DOMAINS[axis]
    entry, target = [((20, m[0] - 1), 1.0), ((5, 10), -2.0)][axis]
    missing = [d for d in range(3) if d not in dims]
    total = np.take(_total(n, m, moves[axis]), 0, axis=missing[0])          # (the total does not vary along the missing dim)
    bump = np.zeros([g[d] for d in dims])
    bump[entry] = target - total[entry]
    bent = list(moves)
    bent[axis] = moves[axis] + [(dims, bump)]
    return _problem(n, m, bent, 750 + axis, typing="f32", idx_dtype=np.uint16, index_base=0), bent, entry


def _reduced_entries_outside(axis, prob):
    """The entries of `axis`' own table domain that break the rule, as coordinates on the domain's dims (and 0 elsewhere)."""
    spec, cells, _ = prob
    c = cells[axis]
    na = spec.n[axis]
    i = np.arange(na).reshape([-1 if d == axis else 1 for d in range(3)])
    bad = np.argwhere((c < np.maximum(i - 1, 0)) | (c > np.minimum(i, na - 2)))
    bad[:, [d for d in range(3) if d not in REDUCED_DOMAINS[axis]]] = 0
    return np.unique(bad, axis=0)


@gpu
@pytest.mark.parametrize("form", ["cached", "general"])
@pytest.mark.parametrize("axis", [0, 1])
def test_one_entry_past_the_rule_in_a_reduced_table_domain_switches_k9_off(env, axis, form):
    """The same refusal where the table holds fewer dims than the grid: examine_tile2d must take each entry's own-axis index
    from that table's strides."""
    hjbdp = env[0]
    prob, bent, entry = _reduced_nonlocal_problem(axis, form)
    spec, cells, term = prob
    assert sorted({axis} | {d for mv in bent[axis] for d in mv[0]}) == list(REDUCED_DOMAINS[axis])
    assert len(_reduced_entries_outside(axis, prob)) == 1 and _is_local(_only(cells, 1 - axis))
    ref = _oracle(env, spec, 17, term)
    with hjbdp.Backup(spec) as bk:
        bk.set_option("temporal", 2)
        _refused(env, bk, 17, terminal=term)
        bk.set_option("temporal", 1)
        _assert_equal(bk.solve(17, terminal=term), ref, spec, ("reduced domain", axis, form, "default"), 17)


@gpu
@pytest.mark.parametrize("axis", [0, 1])
def test_an_axis_that_does_not_see_its_own_state_switches_k9_off(env, axis):
    """x_a+ = (a value inside the grid) + f(the other state): no term spans x_a."""
    hjbdp = env[0]
    spec, cells, term = _own_free_problem(axis)
    assert all(axis not in t.dims for t in spec.next_terms[axis]) and not _is_local(cells)
    ref = _oracle(env, spec, 17, term)
    with hjbdp.Backup(spec) as bk:
        bk.set_option("temporal", 2)
        _refused(env, bk, 17, terminal=term)
        bk.set_option("temporal", 1)
        _assert_equal(bk.solve(17, terminal=term), ref, spec, ("own-free", axis), 17)


def _own_free_problem(axis):
    n, m = GRID_2X2, (3,)
    moves = _local_moves(n, m, 81)
    o = 1 - axis
    moves[axis] = [((o,), np.full(n[o], 1.0), "abs")] + moves[axis]          # one knot above the middle of the axis
    own = (axis != 0, axis != 1)
    return _problem(n, m, moves, 800 + axis, typing="f32", idx_dtype=np.uint8, own=own)


# ---- 8. what must switch K9 off -----------------------------------------------------------------------------------------------------
def _switch_problem(m=(3,), **kw):
    return _problem(GRID_2X2, m, _local_moves(GRID_2X2, m, 91), 900, typing="f32", idx_dtype=np.uint8, index_base=1, **kw)


SOLVE_OPTIONS = ["monitor", "keep_J", "keep_idx", "probe", "progress_every_stage", "fifteen_stages"]


@gpu
@pytest.mark.parametrize("cond", SOLVE_OPTIONS)
def test_solve_options_that_switch_k9_off(env, cond):
    """Per-stage outputs, read-backs and sweeps shorter than two launches: required K9 is refused, the default runs stage by stage
    and equals the oracle (per-stage planes included), and the handle still takes K9 for a plain 16-stage sweep afterwards."""
    hjbdp = env[0]
    spec, cells, term = _switch_problem()
    assert _is_local(cells) and _form(spec) == "cached"
    n_st = 15 if cond == "fifteen_stages" else 20
    assert (n_st < 2 * TILE_K) == (cond == "fifteen_stages")
    calls = []
    kw = {"monitor": dict(monitor_period=4, monitor_tol=0.0), "keep_J": dict(keep_J=True), "keep_idx": dict(keep_idx=True),
          "probe": dict(probe={"lo": [0, 0], "hi": [3, 2], "control": [1], "want": ("g", "j_interp")}),
          "progress_every_stage": dict(progress=lambda k_s, e, e2, sec: calls.append(k_s), progress_every_stage=True),
          "fifteen_stages": {}}[cond]
    okw = {k: v for k, v in kw.items() if k in ("monitor_period", "monitor_tol", "keep_J", "keep_idx")}
    ref = _oracle(env, spec, n_st, term, **okw)
    ref16 = _oracle(env, spec, 16, term)
    with hjbdp.Backup(spec) as bk:
        bk.set_option("temporal", 2)
        _assert_equal(bk.solve(n_st + 5, terminal=term), _oracle(env, spec, n_st + 5, term), spec, (cond, "K9 takes the plain sweep"))
        _refused(env, bk, n_st, terminal=term, **kw)
        _assert_equal(bk.solve(16, terminal=term), ref16, spec, (cond, "16 stages after the refusal"), 16)
        bk.set_option("temporal", 1)
        out = bk.solve(n_st, terminal=term, **kw)
        _assert_equal(out, ref, spec, (cond, "default"), n_st)
        assert not out["stopped_early"] and not ref["stopped_early"]
        if cond == "keep_J":
            assert np.array_equal(_bits(out["J_stages"]), _bits(ref["J_stages"]))
        if cond == "keep_idx":
            assert np.array_equal(out["idx_stages"], ref["idx_stages"])
        if cond == "monitor":
            assert out["last_e2"] == ref["last_e2"]                    # (the label sums of the last two monitor points: integers)
        if cond == "probe":                                    # (that the taps came back; their values are test_gpu_parity.py's)
            assert out["probe"]["g"].shape == (3, 2, n_st) and np.isfinite(out["probe"]["j_interp"]).all()
        if cond == "progress_every_stage":
            assert calls == list(range(n_st, 0, -1)), calls


HANDLE_CONDITIONS = ["forced_variant", "cost64", "sixty_five_controls"]


@gpu
@pytest.mark.parametrize("cond", HANDLE_CONDITIONS)
def test_handle_properties_that_switch_k9_off(env, cond):
    hjbdp, _abi, _ = env
    if cond == "cost64":
        prob = _switch_problem(cost_dtype=np.float64)
    elif cond == "sixty_five_controls":
        prob = _switch_problem(m=(65,))
    else:
        prob = _switch_problem()
    spec, cells, term = prob
    assert _is_local(cells)
    assert (spec.nU > 64) == (cond == "sixty_five_controls") and (spec.cost_dtype == np.float64) == (cond == "cost64")
    ref = _oracle(env, spec, 20, term)
    with hjbdp.Backup(spec, variant=5 if cond == "forced_variant" else None) as bk:
        assert bk.get_option("temporal") == 1
        assert (bk.info()["cost_dtype"] == _abi.HJB_COST_F64) == (cond == "cost64")
        _assert_equal(bk.solve(20, terminal=term), ref, spec, (cond, "default"), 20)
        bk.set_option("temporal", 2)
        _refused(env, bk, 20, terminal=term)
        bk.set_option("temporal", 1)
        _assert_equal(bk.solve(20, terminal=term), ref, spec, (cond, "default, after the refusal"), 20)
        if cond == "forced_variant":                       # the automatic choice again: K9 applies
            bk.set_option("variant", -1)
            bk.set_option("temporal", 2)
            _assert_equal(bk.solve(20, terminal=term), ref, spec, (cond, "unforced"), 20)


@gpu
def test_a_slab_handle_is_never_swept(env):
    """A slab with halos: hjb_solve refuses it whatever `temporal` says (slabs are driven stage by stage with a halo exchange), so
    what the default computes on it is one stage - the oracle's stage of the slab on the owned planes."""
    hjbdp, _abi, c_oracle = env
    spec, cells, term = _switch_problem()
    assert _is_local(cells)
    b, e = 3, 6
    with hjbdp.Backup(spec) as bk:
        need = bk.info()
    hl, hh = min(need["halo_needed_lo"], b), min(need["halo_needed_hi"], spec.n[1] - e)
    assert hl >= 1 and hh >= 1, (need["halo_needed_lo"], need["halo_needed_hi"])
    sub = np.ascontiguousarray(term.reshape(spec.n, order="F")[:, b - hl:e + hh].reshape(-1, order="F"))
    Jr, ir = c_oracle.backup_stage(_abi, spec, sub, slab=(b, e, hl, hh))
    own = slice(hl * spec.n[0], (hl + e - b) * spec.n[0])
    with hjbdp.Backup(spec, slab=(b, e, hl, hh)) as bk:
        assert bk.info()["j_elems"] == sub.size and bk.info()["n_states"] == (e - b) * spec.n[0]
        for temporal in (2, 1):
            bk.set_option("temporal", temporal)
            _refused(env, bk, 20)
        Jg, ig = bk.backup_stage(sub)
        assert np.array_equal(_bits(Jg[own]), _bits(Jr[own])) and np.array_equal(ig, ir)


# ---- the input conditions, without a device -------------------------------------------------------------------------------------------
def test_positive_cases_are_local():
    for case in ROTATION:
        spec, cells, _ = _rotation_problem(case)
        assert _is_local(cells), _rotation_id(case)
        assert cells[0].shape == spec.n + spec.m
    for form in ("cached", "general"):
        assert _is_local(_pair(form)[1])
        for case in DRIFTS:
            cells = _drift_problem(case, form)[1]
            assert _is_local(cells) and _drift_cells_ok(case, cells), (case, form)
        for kind in ("own", "ctrl"):
            assert _is_local(_domain_problem(kind, form)[0][1]), (kind, form)
        for kind, axis in LOCAL_EDGES:
            assert _is_local(_edge_problem(kind, axis, form)[1]), (kind, axis, form)
    for m in [(4,), (7,), (2, 3)]:
        assert _is_local(_ties_problem(m)[1])
    for kw in ({}, {"cost_dtype": np.float64}, {"m": (65,)}):
        assert _is_local(_switch_problem(**kw)[1])


def test_edge_cases_sit_exactly_on_the_rule():
    """What the local edge cases stand for, from their cells: the knot below everywhere; the clamped top cell from n - 2; the
    state's own cell from the top two states."""
    for form in ("cached", "general"):
        cells = _edge_problem("minus_one_everywhere", 0, form)[1]
        for a in range(2):
            i = np.arange(EDGE_GRID[a]).reshape([-1 if d == a else 1 for d in range(3)])
            assert np.array_equal(cells[a], np.broadcast_to(np.maximum(i - 1, 0), cells[a].shape))
        cells = _edge_problem("plus_one_at_n_minus_2", 0, form)[1]
        for a in range(2):
            assert np.all(np.take(cells[a], EDGE_GRID[a] - 2, axis=a) == EDGE_GRID[a] - 2)
        for axis in range(2):
            cells = _edge_problem("plus_five_from_the_top_two", axis, form)[1]
            assert np.all(np.take(cells[axis], [EDGE_GRID[axis] - 2, EDGE_GRID[axis] - 1], axis=axis) == EDGE_GRID[axis] - 2)


def test_boundary_cases_are_nonlocal_by_exactly_one_entry():
    for form in ("cached", "general"):
        for kind, axis in NONLOCAL_EDGES:
            spec, cells, _ = _edge_problem(kind, axis, form)
            assert not _is_local(cells) and _outside(cells) == 1, (kind, axis, form, _outside(cells))
            assert _outside(_only(cells, axis)) == 1 and _is_local(_only(cells, 1 - axis)), (kind, axis, form)
            na = spec.n[axis]
            i = np.arange(na).reshape([-1 if d == axis else 1 for d in range(3)])
            off = (cells[axis] - i)[(cells[axis] < np.maximum(i - 1, 0)) | (cells[axis] > np.minimum(i, na - 2))]
            state = np.broadcast_to(i, cells[axis].shape)[(cells[axis] < np.maximum(i - 1, 0)) | (cells[axis] > np.minimum(i, na - 2))]
            want = {"plus_one_inside_the_last_tile": 1, "plus_five_from_n_minus_3": 1, "minus_two": -2}[kind]
            assert off.tolist() == [want], (kind, axis, form, off)        # (+5 from n - 3 is clamped to the top cell: one cell up)
            if kind == "plus_one_inside_the_last_tile":
                tile = (TILE_X, TILE_Y)[axis]
                assert state[0] // tile == (na - 1) // tile and 0 < state[0] % tile and state[0] + 1 < na - 1, state
            if kind == "plus_five_from_n_minus_3":
                assert state[0] == na - 3
    for axis in range(2):
        assert not _is_local(_own_free_problem(axis)[1])
        for form in ("cached", "general"):
            prob, _, entry = _reduced_nonlocal_problem(axis, form)
            bad = _reduced_entries_outside(axis, prob)
            dims = REDUCED_DOMAINS[axis]
            assert len(bad) == 1 and tuple(bad[0][list(dims)]) == entry, (axis, form, bad)
            assert _is_local(_only(prob[1], 1 - axis)) and not _is_local(prob[1])
            assert _is_local(_domain_problem("ctrl", form)[0][1])            # ... and local without the bent entry
