"""GPU tests (-m gpu): every site of the stage kernels that locates or tracks a cell, driven to the inputs where `<` and `<=` differ.

The problems are tests/problems.py's placement problems (PLACEMENT_CASES): next-state queries that land ON knots, one unit in the
last place beside them, on the first and the last knot and up to two cells beyond either end, by construction in the problem's
own type; on the 'near' grid the arithmetic first guess of find_cell is two or more cells off either way.  placement_case asserts
those input conditions again before anything runs (tests/test_placement_problems.py asserts them without a GPU).

The twin (oracle/hjb_oracle.c) finds a cell by plain binary search; every comparison here is bit for bit against it - J, labels,
and the halo status where a slab is used - over three stages from a random terminal cost, so that stages 2 and 3 read a J whose
neighbouring values differ: a query on knot i located in cell i - 1 with weight 1 gives fma(1, v1 - v0, v0) instead of v0, a
last-bit difference, and near a tie another label.  Two checks do not go through the twin (node identity, and k_probe against
np.searchsorted): a mistake the twin shared would still show there."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAGES = 3


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi, c_oracle


_CASES = {}


def _case(env, name, stages=STAGES):
    """(spec, terminal, the twin's sweep of `stages` stages with every stage kept) of a registered placement problem - built, its
    input conditions asserted and its reference computed once per module, shared by every test that runs it, never written to."""
    key = (name, stages)
    if key not in _CASES:
        from problems import placement_case
        _, _abi, c_oracle = env
        spec, _ = placement_case(name)
        term = np.random.default_rng(len(name)).random(spec.nS).astype(spec.j_dtype)
        ref = c_oracle.sweep(_abi, spec, stages, terminal=term, keep_J=True, keep_idx=True)
        assert np.isfinite(ref["J_stages"].astype(np.float64)).all()
        for a in (ref["J_stages"], ref["idx_stages"], ref["J"], ref["idx"], term):
            a.setflags(write=False)
        _CASES[key] = (spec, term, ref)
    return _CASES[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_sweep(out, ref, what):
    for key in ("J_stages", "idx_stages"):
        a, b = out[key], ref[key]
        bad = np.argwhere(_bits(a) != _bits(b)) if key == "J_stages" else np.argwhere(a.astype(np.int64) != b)
        assert bad.shape[0] == 0, (what, key, bad.shape[0], bad[:6].tolist())
    assert np.array_equal(_bits(out["J"]), _bits(ref["J"])) and np.array_equal(out["idx"], ref["idx"]), what


def _sweep(bk, term, ref, what):
    _same_sweep(bk.solve(STAGES, terminal=term, keep_J=True, keep_idx=True), ref, what)


FREE = ["free-%d-%s" % (D, t) for D in (1, 2, 4, 6) for t in ("float32", "float64")] + \
       ["free-2-%s-%s" % (t, g) for t in ("float32", "float64") for g in ("near", "far")]


# ---- K1, K5: find_cell (csrc/hjbdp_canon.h) on every axis ----------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 3])
@pytest.mark.parametrize("name", FREE)
def test_plain_kernels_find_cell(env, name, variant):
    """K1 k_backup_generic (variant 0) and K5 k_backup_ctrlsplit (variant 3) locate every axis of every (state, control) with
    find_cell, csrc/hjbdp_canon.h:20-39: the clamped guess, `while (i > 0 && q < k[i]) --i`, `while (i < n - 2 && q >= k[i + 1])
    ++i`, and the binary search's `k[mid] <= q` on the 'far' grid.  Aimed at `q >= k[i + 1]` (a query on knot i + 1 with a short
    guess must step up) and `q < k[i]` (a query on knot i with a far guess must stop); the 'near' grid makes either loop run twice."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name)
    with hjbdp.Backup(spec, variant=variant) as bk:
        assert bk.info()["kernel_variant"] == variant
        _sweep(bk, term, ref, (name, variant))


# ---- K7 and the table builds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FREE + ["free-2-tab64"])
def test_tabled_kernel_and_its_table_build(env, name):
    """K7 k_backup_tabled (variant 5) reads cells and weights that k_prep_axis_table found (csrc/kernels_tabled.h:58, HJB_LOCATE ->
    find_cell): both index forms (option tabled_i32 1 / 0).  free-2-tab64: table_dtype float64 on a float32 problem - the queries
    are formed and located in double on the float64 knots (the grid whose counts the case asserts), the weight rounded once."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name)
    for form in (1, 0):
        with hjbdp.Backup(spec, variant=5) as bk:
            assert bk.info()["kernel_variant"] == 5
            bk.set_option("tabled_i32", form)
            assert bk.get_option("tabled_i32") == form
            _sweep(bk, term, ref, (name, form))


@pytest.mark.parametrize("name", ["free-2-float32", "free-4-float32", "free-2-float32-near", "nested-3-float32-inc", "nested-6-float32-dec"])
def test_mfma_table_build(env, name):
    """K12 (csrc/kernels_prep_mfma.h:96: find_cell on the MFMA-formed query): the same tables as the vector build (table_hash) and
    the twin's result, as test_gpu_parity.py::test_mfma_table_build_is_bit_identical does it, on queries that sit on knots."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name)
    with hjbdp.Backup(spec, variant=5) as bk:
        bk.set_option("prep_mfma", 0)
        h0, n_tab = bk.get_option("table_hash"), bk.get_option("prep_tables")
        _sweep(bk, term, ref, (name, "vector build"))
        bk.set_option("prep_mfma", 1)
        h1, n_mfma = bk.get_option("table_hash"), bk.get_option("prep_mfma_tables")
        assert n_tab >= 1 and n_mfma >= 1, (n_tab, n_mfma)
        assert h0 == h1
        _sweep(bk, term, ref, (name, "MFMA build"))


# ---- K8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["row-float32", "row-float64"])
def test_rowwise_kernel(env, name):
    """K8 k_backup_rowwise (variant 6, csrc/kernels_rowwise.h) takes axis 0 from the (cell, weight) table (kernels_tabled.h:58) and
    the other axes' cells per row: lean and plain forms (row_lean 1 / 0).  Axis 0 has 70 knots - a row spans more than a wave -,
    axes 1 and 2 the placement grid."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name)
    assert spec.n[0] == 70
    for lean in (1, 0):
        with hjbdp.Backup(spec, variant=6) as bk:
            assert bk.info()["kernel_variant"] == 6
            bk.set_option("row_lean", lean)
            _sweep(bk, term, ref, (name, lean))


# ---- K2 ------------------------------------------------------------------------------------------------------------------------
NESTED = ["nested-%d-%s-%s" % (D, t, mono) for D in (2, 3, 6) for t in ("float32", "float64") for mono in ("inc", "dec", None)] + \
         ["nested-3-%s-inc-%s" % (t, g) for t in ("float32", "float64") for g in ("near", "far")]


@pytest.mark.parametrize("name", NESTED)
def test_nested_kernel_track_update(env, name):
    """K2 k_backup_nested (variant 1) keeps the last axis' cell across the inner control sweep: track_update,
    csrc/kernels_nested.h:110-120, `q >= c.lo && q < c.hi` keeps the cell, else find_cell.  Aimed at `q < c.hi`: with whole-cell
    steps the next query sits exactly on c.hi (increasing table) or on c.lo (decreasing) - `<=` there would keep cell i - 1 with
    weight 1.  Non-monotone tables jump two cells and back."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name)
    with hjbdp.Backup(spec, variant=1) as bk:
        assert bk.info()["kernel_variant"] == 1
        _sweep(bk, term, ref, name)


# ---- K3 / K4: the packed kernels ----------------------------------------------------------------------------------------------
_PACKED_MODES = {}
PACKED = ["nested-%d-float32-%s" % (D, mono) for D in (2, 3, 5, 6) for mono in ("inc", "dec")]


@pytest.mark.parametrize("variant", [2, 4])
@pytest.mark.parametrize("name", PACKED + ["nested-3-float32-inc-near", "nested-3-float32-inc-far"])
def test_packed_kernels_crossing_masks(env, name, variant):
    """The packed kernels replace the search on the last axis by one-sided tests over the monotone inner table: variant 2
    csrc/kernels_packed.h:393 (`up ? q >= hi : q < lo`), variant 4 csrc/kernels_packed2.h:993-1007 (the crossing mask `cm`, its
    first crossing served from prefetched corners, later ones by find_cell) and find_cell_g, kernels_packed2.h:114-123.  Increasing
    tables cross AT equality (q == hi enters the next cell), decreasing ones STAY at equality (q == lo stays); placement_case has
    asserted both happen.  Every window / hierarchical mode the shapes reach is recorded for the test below."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name)
    with hjbdp.Backup(spec, variant=variant) as bk:
        assert bk.info()["kernel_variant"] == variant
        if variant == 4:
            mode = bk.get_option("packed2_mode")
            _PACKED_MODES.setdefault(mode, []).append(name)
        _sweep(bk, term, ref, (name, variant))
        if variant == 4 and mode == 5:
            bk.set_option("window_planes", 4)
            assert bk.get_option("packed2_mode") == 2
            _PACKED_MODES.setdefault(2, []).append(name)
            _sweep(bk, term, ref, (name, variant, "four planes"))


@pytest.mark.parametrize("name", ["mixed-%d-%s" % (D, mono) for D in (2, 3, 5, 6) for mono in ("inc", "dec")])
def test_packed2_state_dependent_inner_term(env, name):
    """Variant 4 with a last-axis inner term over (a state dim, the control) - mixed_inner='only' -: the per-lane table form of the
    same crossing tests (kernels_packed2.h:999, `b_data[boff + j * b_stride]`)."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name)
    with hjbdp.Backup(spec, variant=4) as bk:
        assert bk.info()["kernel_variant"] == 4
        _PACKED_MODES.setdefault(bk.get_option("packed2_mode"), []).append(name)
        _sweep(bk, term, ref, name)


def test_packed2_modes_were_reached():
    """Runs after the cases above: the window modes the 5-D and 6-D shapes exist for (mode 2, and mode 5 where the host admits
    three planes) and a non-window mode were all run.  (Mode 3 needs the on-the-fly quaternion model, whose queries no term table
    can place: test_gpu_parity.py::test_packed_modes_2_and_3_slab keeps it.)"""
    assert 2 in _PACKED_MODES, _PACKED_MODES
    assert set(_PACKED_MODES) - {2, 5}, _PACKED_MODES
    print("packed2 modes reached:", {k: len(v) for k, v in _PACKED_MODES.items()})


# ---- K15 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rates-even", "rates-near", "rates-far"])
def test_uniwin_kernel(env, name):
    """K15 (csrc/kernels_uniwin.h, variant 4 mode 7): k_uniwin_plan fixes per point the cell of every inner control and the
    control `jc` at which the cell changes (kernels_uniwin.h:120, find_cell_g; `c != prev`), the stage applies it (:382).  The
    inner sweep comes up onto a knot exactly at its sixth level: the change must be taken AT that control.  Points whose sweep or
    level axes span more cells take the slow path in the same launch (the uneven grids: most of them).  K15 is forced on and must
    be the mode that ran; K3's three-plane window (mode 5, kernels_packed2.h) and its four-plane form (mode 2) on the same handle
    give the same bits."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name)
    with hjbdp.Backup(spec) as bk:
        assert bk.info()["kernel_variant"] == 4 and bk.get_option("uniwin_ok") == 1
        slow, points = bk.get_option("uniwin_slow_points"), spec.nS // int(np.prod(spec.n[:3]))
        print("%s: %d of %d points on the slow path" % (name, slow, points))
        assert name != "rates-even" or 0 < slow < points                 # both paths run
        bk.set_option("uniwin", 1)
        assert bk.get_option("packed2_mode") == 7 and bk.get_option("uniwin") == 1
        _sweep(bk, term, ref, (name, "uniwin"))
        bk.set_option("uniwin", 0)
        assert bk.get_option("packed2_mode") == 5
        _PACKED_MODES.setdefault(5, []).append(name)
        _sweep(bk, term, ref, (name, "mode 5"))
        bk.set_option("window_planes", 4)
        assert bk.get_option("packed2_mode") == 2
        _sweep(bk, term, ref, (name, "mode 2"))


# ---- K10 / K13 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["colsweep-g%d-%s" % (g, s) for g in (2, 3) for s in ("f32", "f16", "f32-a0")])
def test_colsweep_kernel(env, name):
    """K10 (variant 7, csrc/kernels_colsweep.h) runs on host-built plans: per control the group-axis cell and which pair of the
    three window knots the query lies between (csrc/hjbdp_colsweep.hip:33-79, from the tables of kernels_tabled.h:58).  The group
    axis moves whole cells, the window axis {-h/2, 0, +h/2}: a query on the middle window knot belongs to the upper pair with
    weight 0.  The one-load (DPP) form, which the f32 / f16 cases must get, and the two-loads form (cs_dpp 0; the -a0 cases, whose
    axis-0 queries sit on knots too, get whichever the host admits); float32 and binary16 storage."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name)
    with hjbdp.Backup(spec, variant=7) as bk:
        assert bk.info()["kernel_variant"] == 7
        assert bk.get_option("cs_group_axis") == int(name[10])
        dpp = bk.get_option("cs_dpp")
        assert dpp == 1 or name.endswith("-a0"), "the host did not admit the one-load form"
        _sweep(bk, term, ref, (name, "dpp %d" % dpp))
        if dpp:
            bk.set_option("cs_dpp", 0)
            assert bk.get_option("cs_dpp") == 0
            _sweep(bk, term, ref, (name, "two loads"))


_COOP = []


@pytest.mark.parametrize("name", ["colsweep-g%d-%s-coop" % (g, s) for g in (2, 3) for s in ("f32", "f16")])
def test_colsweep_cooperative_kernel(env, name):
    """K13 (csrc/kernels_colcoop.h, option cs_coop): the same plans, corner rows shared through LDS."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name)
    with hjbdp.Backup(spec, variant=7) as bk:
        bk.set_option("cs_coop", 1)
        _COOP.append((name, bk.get_option("cs_coop"), bk.get_option("cs_coop_why")))
        _sweep(bk, term, ref, name)


def test_colsweep_cooperative_kernel_ran():
    assert _COOP and all(on == 1 for _, on, _ in _COOP), _COOP


# ---- K9 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["local2d-%s-u%d" % (t, u) for t in ("f32", "f64", "tab64") for u in (4, 8)])
def test_tile2d_kernels(env, name):
    """K9 (csrc/kernels_tile2d.h): several stages per launch on a local 2-D problem; the cached form (one control dim of four
    levels) applies a host-built plan of cells, the general form reads the (cell, weight) tables.  temporal = 2 makes hjb_solve
    fail unless K9 ran; 19 stages = two launches of eight and one of three.  Queries sit on the state's own knot, on the knot
    below, one unit in the last place above it, one below the knot above, and beyond both ends."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name, stages=19)
    with hjbdp.Backup(spec) as bk:
        for temporal in (2, 0):
            bk.set_option("temporal", temporal)
            out = bk.solve(19, terminal=term)
            assert out["stages_done"] == 19
            assert np.array_equal(_bits(out["J"]), _bits(ref["J"])) and np.array_equal(out["idx"], ref["idx"]), (name, temporal)


# ---- K22 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["free-1-float64", "free-2-float32", "free-2-float32-near", "free-4-float64", "free-6-float32", "free-2-tab64"])
def test_evaluate_kernel(env, name):
    """K22 k_evaluate (csrc/kernels_evaluate.h) on the twin's own policy: stage k evaluated from the twin's J of stage k + 1 with
    the twin's labels must be the twin's J of stage k.  Both term sources (eval_tables 0: canon_locate -> find_cell on the terms'
    sum; 1: the tables of kernels_tabled.h:58) and both index widths (eval_i32 1 / 0)."""
    hjbdp, _abi, _ = env
    spec, term, ref = _case(env, name)
    ran = set()
    with hjbdp.Backup(spec, variant=5) as bk:
        for src in (0, 1):
            try:
                bk.set_option("eval_tables", src)
            except hjbdp.HjbError as e:
                assert e.status == _abi.HJB_E_UNSUPPORTED
                continue
            ran.add(src)
            for i32 in (1, 0):
                bk.set_option("eval_i32", i32)
                for k in range(STAGES):
                    Jn = term if k == STAGES - 1 else ref["J_stages"][:, k + 1]
                    got = bk.evaluate_stage(Jn, ref["idx_stages"][:, k].astype(spec.idx_np_dtype))
                    assert np.array_equal(_bits(got), _bits(ref["J_stages"][:, k])), (name, src, i32, k)
    assert 1 in ran and (0 in ran or spec.table_dtype is not None), ran


# ---- K24 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["free-2-float32", "free-2-float64", "free-4-float32", "free-2-float32-near", "free-2-tab64"])
def test_disturbed_kernel(env, name):
    """K24 k_backup_disturb (variant 8, csrc/kernels_disturb.h) locates every node's query with canon_locate (hjbdp_canon.h:107).
    The node offsets are themselves multiples of h (-2 .. 2 cells), so the offset queries land on knots and beyond the ends again;
    E_w and max_w, both index forms (dist_i32).  Reference: tests/disturbance_refs.py (numpy, np.searchsorted); with every offset
    zero the same reference is the twin's stage, which is asserted first."""
    hjbdp, _abi, _ = env
    from disturbance_refs import DisturbedRef
    spec, term, ref = _case(env, name)
    hs = np.array([(k[-1] - k[0]) / (len(k) - 1) for k in spec.knots])
    mult = np.array([[0, 1, -1, 2, -2][(w + a) % 5] for a in range(spec.D) for w in range(3)]).reshape(spec.D, 3)
    off = mult * hs[:, None]
    zero = DisturbedRef(spec, np.zeros((spec.D, 1)), None, "worst").backup(term)
    assert np.array_equal(_bits(zero[0]), _bits(ref["J_stages"][:, STAGES - 1])) and np.array_equal(zero[1], ref["idx_stages"][:, STAGES - 1])
    with hjbdp.Backup(spec) as bk:
        for mode, w in (("expect", (0.5, 0.25, 0.25)), ("worst", None)):
            dref = DisturbedRef(spec, off, w, mode)
            for a, (below, above, split) in dref.coverage().items():
                assert below and above and split, (a, below, above, split)
            Jr, ir = dref.backup(term)
            bk.set_disturbance(off, w, mode)
            assert bk.info()["kernel_variant"] == 8
            for i32 in (1, 0):
                bk.set_option("dist_i32", i32)
                assert bk.get_option("dist_form") == i32
                J, idx = bk.backup_stage(term)
                assert np.array_equal(_bits(J), _bits(Jr)) and np.array_equal(idx, ir), (name, mode, i32, int(np.sum(_bits(J) != _bits(Jr))))
            bk.set_option("dist_i32", 1)
            bk.clear_disturbance()


# ---- not through the twin: node identity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["identity-%d-%s" % (D, t) for D in (2, 4) for t in ("float32", "float64")])
def test_node_identity(env, name):
    """One control whose displacement is +0 on every axis: the next state of node s is node s, every weight +0, so the stage
    value is fl(g(s) + J_next[s]) in the type (numpy, the cost terms' ordered sum) at every state that is on the last knot of no
    axis - through K1 (variant 0), K7 (variant 5) and K22.  A cell search that put a query on knot i into cell i - 1 would read
    fma(1, J[i] - J[i - 1], J[i - 1]) instead, which differs from J[i] wherever the difference rounds."""
    hjbdp, _abi, _ = env
    from float64_refs import ordered_sum
    from problems import placement_case
    spec, _ = placement_case(name)
    dt = spec.dtype
    rng = np.random.default_rng(5)
    Jn = (rng.random(spec.nS) * np.exp2(rng.integers(-6, 7, spec.nS))).astype(dt)        # neighbours of very different size
    full = spec.n + spec.m                                                               # m = (1,): the one control is index 0
    g = ordered_sum([np.broadcast_to(np.asarray(t.data).reshape([full[d] if d in t.dims else 1 for d in range(len(full))]), full)[..., 0]
                     for t in spec.cost_terms], dt)
    want = (g + Jn.reshape(spec.n, order="F")).astype(dt)
    inner = np.ones(spec.n, dtype=bool)
    for a in range(spec.D):
        inner[tuple(slice(None) if d != a else spec.n[a] - 1 for d in range(spec.D))] = False
    assert inner.sum() == np.prod([n - 1 for n in spec.n])
    wf, mf = want.reshape(-1, order="F"), inner.reshape(-1, order="F")
    for variant in (0, 5):
        with hjbdp.Backup(spec, variant=variant) as bk:
            assert bk.info()["kernel_variant"] == variant
            J, idx = bk.backup_stage(Jn)
            assert np.all(idx == spec.index_base)
            bad = np.flatnonzero((_bits(J) != _bits(wf)) & mf)
            assert bad.size == 0, (name, variant, bad.size, bad[:6])
            Je = bk.evaluate_stage(Jn, idx)
            bad = np.flatnonzero((_bits(Je) != _bits(wf)) & mf)
            assert bad.size == 0, (name, variant, "evaluate", bad.size, bad[:6])


# ---- not through the twin: k_probe against np.searchsorted ---------------------------------------------------------------------
def _lerp_by_searchsorted(spec, q, Jn):
    """N-linear interpolation of Jn at the queries q [N, D] with cell = clip(searchsorted(k, q, 'right') - 1, 0, n - 2) and
    weight = fl(fl(q - k[c]) * rdx[c]), rdx = fl(1 / fl(k[c + 1] - k[c])); axis 0 folded first, each fold one fused
    multiply-add in the type (tests/evaluate_refs._fma32 / tests/disturbance_refs.fma64: exact)."""
    from disturbance_refs import fma64
    from evaluate_refs import _fma32
    dt = spec.dtype.type
    fma = _fma32 if spec.dtype == np.float32 else fma64
    cells, ws = [], []
    for a in range(spec.D):
        k = spec.knots[a].astype(dt)
        c = np.clip(np.searchsorted(k, q[:, a], side="right") - 1, 0, len(k) - 2)
        rdx = (dt(1) / (k[1:] - k[:-1]).astype(dt)).astype(dt)
        cells.append(c)
        ws.append(((q[:, a] - k[c]).astype(dt) * rdx[c]).astype(dt))
    J = np.asarray(Jn).astype(dt).reshape(spec.n, order="F")
    vals = [J[tuple(cells[a] + ((corner >> a) & 1) for a in range(spec.D))] for corner in range(1 << spec.D)]
    for a in range(spec.D):
        vals = [np.asarray(fma(ws[a], (vals[j + 1] - vals[j]).astype(dt), vals[j])).astype(dt) for j in range(0, len(vals), 2)]
    return vals[0], cells


@pytest.mark.parametrize("name", ["free-1-float32", "free-2-float32", "free-2-float64", "free-2-float32-near", "free-2-float64-near",
                                  "free-4-float64", "nested-3-float32-dec"])
def test_probe_kernel_against_searchsorted(env, name):
    """K11 k_probe (csrc/kernels_probe.h) returns the query and the interpolated value of every state of a block at one control
    (it has no output for the cell and the weight themselves): the query must be the terms' ordered sum bit for bit, and the
    value the one numpy gets with cell = clip(searchsorted(k, q, 'right') - 1, 0, n - 2) and weight = fl(fl(q - k[c]) * rdx[c]) -
    a cell one off at an equality changes the value's last bits on a J whose neighbours differ in size."""
    hjbdp, _abi, _ = env
    from problems import placement_case, placement_queries
    spec, _ = placement_case(name)
    rng = np.random.default_rng(3)
    Jn = (rng.random(spec.nS) * np.exp2(rng.integers(-6, 7, spec.nS))).astype(spec.dtype)
    lo, hi = (0,) * spec.D, spec.n
    on_knot = 0
    with hjbdp.Backup(spec) as bk:
        for u in range(spec.nU):
            ctrl = tuple(int(x) for x in np.unravel_index(u, spec.m, order="F"))
            got = bk.probe_stage({"lo": lo, "hi": hi, "control": ctrl}, J_next=Jn)
            for a in range(spec.D):
                assert np.array_equal(_bits(got["x_next"][..., a]), _bits(np.ascontiguousarray(placement_queries(spec, a)[(Ellipsis,) + ctrl]))), (u, a)
            q = got["x_next"].reshape(-1, spec.D, order="F")
            want, cells = _lerp_by_searchsorted(spec, q, Jn)
            bad = np.flatnonzero(_bits(got["j_interp"].reshape(-1, order="F")) != _bits(want))
            assert bad.size == 0, (name, ctrl, bad.size, bad[:6])
            on_knot += sum(int(np.sum(q[:, a] == spec.knots[a].astype(spec.dtype)[cells[a]])) for a in range(spec.D))
            if spec.nU > 10 and u >= 9:
                break
    assert on_knot > 0


# ---- slabs: a query on the knot of the outermost halo plane ---------------------------------------------------------------------
def _slab_planes(spec, b, e):
    """Over the owned planes [b, e) of the last axis: (lowest cell, highest cell + 1) any query's cell touches, and whether some
    owned query sits EXACTLY on the lower knot of the lowest / of the highest cell touched."""
    from problems import locate_dtype, placement_cells, placement_queries
    dt = locate_dtype(spec).type
    a = spec.D - 1
    k = spec.knots[a].astype(dt)
    q = np.asarray(placement_queries(spec, a)).astype(dt)
    q = q[tuple(slice(b, e) if d == a else slice(None) for d in range(q.ndim))]
    c = placement_cells(k, q)
    return int(c.min()), int(c.max()) + 1, bool(np.any(q[c == c.min()] == k[c.min()])), bool(np.any(q[c == c.max()] == k[c.max()]))


@pytest.mark.parametrize("name,variant,b,e,ends", [("nested-3-float32-inc", 4, 5, 8, True), ("free-4-float32", 5, 5, 8, True),
                                                   ("row-float32", 6, 5, 8, True), ("colsweep-g3-f32", 7, 4, 8, True),
                                                   ("colsweep-g2-f32", 7, 4, 8, False)])
def test_slab_with_a_query_on_the_last_halo_knot(env, name, variant, b, e, ends):
    """One slab of the last axis per family that takes slabs (variants 4, 5, 6, 7; for 7 with the group axis last and with the
    window axis last).  The halos are exactly the planes the owned queries' cells touch (numpy, np.searchsorted), which the
    handle's conservative halo_needed_lo / _hi must cover.  ends: some owned query sits exactly on the knot of the FIRST halo plane
    (its cell's lower corner) and another exactly on the lower knot of the LAST halo cell, whose upper corner is the last plane
    granted - asserted from the inputs; the window axis moves half cells, so there the outermost queries are midpoints.  The owned
    planes equal the whole-grid twin's and the status is clean; with one plane fewer on either side HJB_E_HALO is raised, as
    test_gpu_parity.py::test_packed_modes_2_and_3_slab checks it.  A cell taken one too low at the low equality leaves the halo
    (an error where none is due); one too low at the high equality fits the narrower halo (no error where one is due)."""
    hjbdp, _abi, c_oracle = env
    spec, term, ref = _case(env, name)
    nl = spec.n[-1]
    inner = spec.nS // nl
    Jw, iw = ref["J_stages"][:, STAGES - 1], ref["idx_stages"][:, STAGES - 1]
    T2 = term.reshape(inner, nl, order="F")
    c_lo, c_hi, on_lo, on_hi = _slab_planes(spec, b, e)
    lo, hi = b - c_lo, c_hi - (e - 1)
    assert lo >= 1 and hi >= 1 and c_lo >= 1 and c_hi <= nl - 2, (c_lo, c_hi)     # neither outermost cell is a clamped one
    assert (on_lo and on_hi) or not ends
    with hjbdp.Backup(spec, variant=variant) as bk:
        need = bk.info()
    print("%s: touched halo (%d, %d), halo_needed (%d, %d)" % (name, lo, hi, need["halo_needed_lo"], need["halo_needed_hi"]))
    assert need["halo_needed_lo"] >= lo and need["halo_needed_hi"] >= hi, (need["halo_needed_lo"], need["halo_needed_hi"], lo, hi)

    def cut(l, h):
        return np.asfortranarray(T2[:, b - l:e + h]).reshape(-1, order="F")

    with hjbdp.Backup(spec, slab=(b, e, lo, hi), variant=variant) as bk:
        assert bk.info()["kernel_variant"] == variant
        Jo, io = bk.backup_stage(cut(lo, hi))                                    # a dirty status would raise
    assert np.array_equal(_bits(np.ascontiguousarray(Jo.reshape(inner, -1, order="F")[:, lo:lo + e - b])),
                          _bits(np.ascontiguousarray(Jw.reshape(inner, nl, order="F")[:, b:e])))
    assert np.array_equal(io, iw.reshape(inner, nl, order="F")[:, b:e].reshape(-1, order="F"))
    for l, h in ((lo - 1, hi), (lo, hi - 1)):
        with hjbdp.Backup(spec, slab=(b, e, l, h), variant=variant) as bk:
            with pytest.raises(hjbdp.HjbError) as ei:
                bk.backup_stage(cut(l, h))
            assert ei.value.status == _abi.HJB_E_HALO, (l, h)
