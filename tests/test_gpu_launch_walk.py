"""GPU tests (-m gpu): the grid-stride stage kernels under launches SMALLER than their work (and larger).

Every grid-stride stage kernel walks its work in passes (`for (v = first; v < n; v += gridDim.x)`), several of them behind a remap
of blockIdx.x that gives each XCD a contiguous share of every pass (csrc/hjbdp_walk.h, kernels_packed2.h).  choose_launch sizes
the launch to the work up to a cap, so on the small problems of the parity suite every workgroup goes through its loop exactly
once: the second and later passes - and what must survive from one pass to the next: per-lane LDS windows and masks, prefetched
cells, per-wave scratch, J staged in LDS once - ran at full size only, checked on samples.  A wrong walk writes a state twice or
never; a state never written keeps the ping-pong buffer's value of two stages earlier, a finite and plausible J.

Here each kernel family and form gets a problem of W >= 40 workgroup-sized work units that the automatic launch covers in ONE
pass (asserted), and is then swept under option "grid" = G for G in {1, 2, 7, 8, 9, 16, the largest multiple of 8 below W / 2, an
odd value near W / 3, W - 1, W, W + 1, 2 W + 3}: three stages against the C oracle bit for bit, J and labels of every stage; for
G in {1, 9, W - 1} also one hjb_backup_stage_device into a NaN-prefilled J buffer and a 0xff-prefilled label buffer, of which
nothing may be left.  The pass counts the grids stand for are asserted from W and G (_grids).  Beside the matrix: slab handles
with halos (the halo planes of the output stay NaN), hjb_multi_set_option's forwarding, a graph-replayed sweep and a batched
launch with a different multi-pass grid per problem (hjbdp.solve_batch(options=...) sets them on the handles it creates).

One exception to "one pass at the automatic launch": the control-split kernel (variant 3) WITHOUT J in LDS.  Its J exceeds
64 KiB, so it has more than 8192 states at four states per workgroup, and its launch is capped at 1024 workgroups: the automatic
launch of that form is itself a walk of several passes (asserted as such); W is the number of work units, computed from the
problem.  Option "block" does not re-choose variant 3's grid either, so its W is computed for the block in effect throughout.

Not covered here: variants 7 and 1 and K15 (their launch is part of their plan; the refusal of "grid" is pinned by
test_gpu_launch_choice.py), packed2's model modes 3 / 6 (no generator reaches them; they share the walk of modes 2 / 5), and the
lookup, probe, fill and gather kernels (test_gpu_aux_kernels.py).

Wall time of the default `-m gpu` run on one MI355X box, both runs back to back (tests/conftest.py states a 540 s budget): 365 s
at the parent commit (410 tests), 356 s with this file (472 tests) - the difference is the box's run-to-run noise; this file's
62 tests take 3.5 s of it (4.3 s when run alone), so nothing of it is `extended`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAGES = 3
STAGE_GRIDS = ("1", "9", "W-1")      # the grids that also get the single-stage check into prefilled buffers


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi, c_oracle


# ---- launch sizes -----------------------------------------------------------------------------------------------------------------
def _passes(W, G):
    return -(-W // G)


def _grids(W):
    """{name: G} for W work units, with the conditions the set stands for asserted: a walk of three or more passes with a ragged
    last pass, two or more passes at a multiple of 8 and at a non-multiple (packed2's window modes remap only multiples of 8;
    xcd_share's remainder term works only at non-multiples), and idle workgroups."""
    assert W >= 40, W
    m8 = (-(-W // 2) - 1) // 8 * 8                    # the largest multiple of 8 below W / 2
    odd = (W // 3) | 1                                # an odd value near W / 3
    g = {"1": 1, "2": 2, "7": 7, "8": 8, "9": 9, "16": 16, "m8": m8, "odd": odd, "W-1": W - 1, "W": W, "W+1": W + 1, "2W+3": 2 * W + 3}
    assert m8 % 8 == 0 and 16 <= m8 < W / 2 and odd % 2 == 1 and abs(odd - W / 3) <= 2, (W, m8, odd)
    G = list(g.values())
    assert any(_passes(W, x) >= 3 and W % x != 0 for x in G), (W, G)
    assert any(x % 8 == 0 and _passes(W, x) >= 2 for x in G) and any(x % 8 != 0 and _passes(W, x) >= 2 for x in G), (W, G)
    assert _passes(W, W - 1) == 2 and _passes(W, W) == 1 and any(x > W for x in G), (W, G)
    assert all(1 <= x <= (1 << 20) for x in G), (W, G)
    return g


def _work_units(spec, n_owned, variant, block):
    """Workgroup-sized work units of a stage on n_owned states (csrc/hjbdp_choose.hip, the kernels' own loops)."""
    if variant == 6:                                   # one wave per 64-state chunk of a grid row, four waves per workgroup
        return -(-((n_owned // spec.n[0]) * -(-spec.n[0] // 64)) // 4)
    per = {0: 256, 4: 256, 5: 256, 2: 512, 3: block // 64}[variant]
    return -(-n_owned // per)


# ---- problems ---------------------------------------------------------------------------------------------------------------------
def _respec(spec, **kw):
    import hjbdp
    args = dict(dtype=spec.dtype, index_base=spec.index_base, j_storage=None if spec.j_dtype == spec.dtype else spec.j_dtype,
                idx_dtype=spec.idx_dtype, table_dtype=spec.table_dtype, cost_dtype=spec.cost_dtype, model=spec.model)
    args.update(kw)
    return hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, **args)


RAND_SHAPES = {3: ((24, 22, 20), (4, 3)), 4: ((12, 10, 9, 10), (3, 2, 2))}          # 10,560 and 10,800 states: 42 / 43 chunks of 256


def _rand(D, typing):
    from problems import random_problem
    n, m = RAND_SHAPES[D]
    base = random_problem(7000 + D, n, m, dtype=np.float64, nonuniform=(typing == "tab64"), index_base=1)
    return {"f64": lambda: base,
            "f32": lambda: _respec(base, dtype=np.float32),
            "f16s": lambda: _respec(base, dtype=np.float32, j_storage=np.float16),
            "tab64": lambda: _respec(base, dtype=np.float32, table_dtype=np.float64),
            "cost64": lambda: _respec(base, dtype=np.float32, cost_dtype=np.float64)}[typing]()


def _packed(name, storage):
    """The shapes of test_gpu_launch_choice.py's corpus for the packed2 modes, scaled up to 50 - 130 chunks of 256 states."""
    from problems import nested_problem, rate_shared_problem
    spec = {
        "c2": lambda: nested_problem(8, (30, 24, 32), (3, 4, 6)),                                  # C2 shape: mode 4 (1 with the axis-0 table)
        "c2ctrl": lambda: nested_problem(4, (30, 24, 18), (5, 7)),                                 # two control dims: the plain mode 0
        "mixed": lambda: nested_problem(5, (30, 24, 32), (3, 4, 6), mixed_inner="only"),           # general inner term: mode 1
        "win": lambda: nested_problem(3, (40, 9, 6, 9), (3, 3, 5)),                                # four-plane window, chunks in state order
        "win_mono": lambda: nested_problem(3, (40, 9, 6, 9), (3, 3, 5), monotone="inc", spread=0.05),   # three-plane window
        # 540 states per point of the level axes = two chunks and a remainder: the transposed visiting order over a 2 x 64 rectangle
        # that covers 127 chunks (one position past the last chunk is skipped)
        "win5": lambda: nested_problem(3, (36, 15, 4, 3, 5), (3, 3, 5)),
        "win5_mono": lambda: nested_problem(3, (36, 15, 4, 3, 5), (3, 3, 5), monotone="inc", spread=0.05),
        "rate": lambda: rate_shared_problem(1503, (8, 6, 6), (4, 4, 5), m=(7, 7, 7)),              # K15's shape with K15 off: mode 5
    }[name]()
    return _respec(spec, j_storage=np.float16) if storage == "f16s" else spec


def _kirk(prec, dx):
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision=prec)
    ds.N, ds.dx, ds.du = 13, dx, 100
    return ds.build_spec()


def _colsweep(storage):
    from problems import colsweep_problem
    return colsweep_problem(1, (70, 9, 8, 11), nU=9, gax=3, cost="fast", j_storage=np.float16 if storage == "f16s" else None)


# ---- the checks -------------------------------------------------------------------------------------------------------------------
def _buffers(hjbdp, bk, spec, J):
    """Device input / NaN-prefilled output / 0xff-prefilled label buffer (as tests/test_gpu_streams.py::_buffers)."""
    inf = bk.info()
    jd, idt = np.dtype(spec.j_dtype), np.dtype(spec.idx_np_dtype)
    dIn = hjbdp.DeviceBuffer(J.nbytes)
    dIn.upload(J)
    dOut = hjbdp.DeviceBuffer(inf["j_elems"] * jd.itemsize)
    dOut.upload(np.full(inf["j_elems"], np.nan, dtype=jd))
    dI = hjbdp.DeviceBuffer(inf["n_states"] * idt.itemsize)
    dI.upload(np.full(inf["n_states"] * idt.itemsize, 0xff, dtype=np.uint8))
    return dIn, dOut, dI


def _stage_into_prefilled(hjbdp, bk, spec, J_in, J_ref, i_ref, own, what):
    """One hjb_backup_stage_device into prefilled buffers: the owned part equals the oracle's stage and holds no prefill value,
    everything outside it (the halo planes of a slab) is still NaN."""
    J_in = np.ascontiguousarray(J_in, dtype=spec.j_dtype)
    bufs = _buffers(hjbdp, bk, spec, J_in)
    try:
        bk.backup_stage_device(*bufs)
        bk.check_device_status()
        Jg, ig = bufs[1].download(spec.j_dtype), bufs[2].download(spec.idx_np_dtype)
    finally:
        for d in bufs:
            d.free()
    prefill = np.frombuffer(b"\xff" * ig.dtype.itemsize, dtype=ig.dtype)[0]
    left = np.flatnonzero(np.isnan(Jg[own].astype(np.float64)))
    assert left.size == 0, (what, "owned states never written", left.size, left[:8])
    left = np.flatnonzero(ig == prefill)
    assert left.size == 0, (what, "labels never written", left.size, left[:8])
    bad = np.flatnonzero(Jg[own] != J_ref[own])
    assert bad.size == 0, (what, "J", bad.size, bad[:8], Jg[own][bad[:4]], J_ref[own][bad[:4]])
    bad = np.flatnonzero(ig != i_ref)
    assert bad.size == 0, (what, "labels", bad.size, bad[:8])
    outside = np.ones(Jg.size, dtype=bool)
    outside[own] = False
    assert np.isnan(Jg[outside].astype(np.float64)).all(), (what, "a write outside the owned planes",
                                                            np.flatnonzero(outside & ~np.isnan(Jg.astype(np.float64)))[:8])


def _set_grid(bk, G):
    bk.set_option("grid", G)
    assert bk.get_option("grid") == G and bk.info()["grid"] == G


def _walk_matrix(env, spec, bk, variant, what, seed=5):
    """The matrix of one handle (its form options already set): W from the automatic launch, every G of _grids(W)."""
    hjbdp, _abi, c_oracle = env
    from problems import random_terminal
    inf = bk.info()
    assert inf["kernel_variant"] == variant, (what, inf["kernel_variant"])
    auto = bk.get_option("grid")
    assert auto == inf["grid"]
    W = _work_units(spec, spec.nS, variant, inf["block"])
    if variant == 3:
        # "block" keeps the grid hjb_create chose for the form's own block (512 with J in LDS: up to 2048 workgroups; else 256: 1024)
        b0 = 512 if inf["lds_bytes"] else 256
        units0 = _work_units(spec, spec.nS, 3, b0)
        assert auto == min(units0, 2048 if b0 == 512 else 1024), (what, auto, units0)
        assert (auto == units0) == bool(inf["lds_bytes"]), (what, "one pass with J in LDS, a capped launch without", auto, units0)
    else:
        assert auto == W, (what, "the automatic launch covers the work in one pass", auto, W)
    grids = _grids(W)
    if spec.D == 2:
        bk.set_option("temporal", 0)                   # the stage kernel sweeps, not the several-stages-per-launch kernel
    term = random_terminal(spec, seed)
    ref = c_oracle.sweep(_abi, spec, STAGES, terminal=term, keep_J=True, keep_idx=True)
    assert np.isfinite(ref["J_stages"].astype(np.float64)).all(), (what, "the oracle's sweep is not finite: pick another seed")
    first = STAGES - 1                                 # the first computed stage's column
    for name, G in grids.items():
        _set_grid(bk, G)
        out = bk.solve(STAGES, terminal=term, keep_J=True, keep_idx=True)
        for k in range(STAGES - 1, -1, -1):
            bad = np.flatnonzero(out["J_stages"][:, k] != ref["J_stages"][:, k])
            assert bad.size == 0, (what, "grid %s = %d of W = %d" % (name, G, W), "J of stage column %d" % k, bad.size, bad[:8],
                                   out["J_stages"][bad[:4], k], ref["J_stages"][bad[:4], k])
            bad = np.flatnonzero(out["idx_stages"][:, k] != ref["idx_stages"][:, k])
            assert bad.size == 0, (what, "grid %s = %d of W = %d" % (name, G, W), "labels of stage column %d" % k, bad.size, bad[:8])
        assert np.array_equal(out["J"], ref["J"]) and np.array_equal(out["idx"], ref["idx"]), (what, name, G)
        assert bk.get_option("grid") == G
        if name in STAGE_GRIDS:
            _stage_into_prefilled(hjbdp, bk, spec, term, ref["J_stages"][:, first], ref["idx_stages"][:, first], slice(0, spec.nS),
                                  (what, "grid %s = %d of W = %d" % (name, G, W)))
    return W


# ---- the matrix -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typing", ["f32", "f64", "f16s"])
@pytest.mark.parametrize("D", [3, 4])
def test_generic_kernel_walk(env, D, typing):
    """Variant 0: one state per thread, 256 states per workgroup pass."""
    hjbdp = env[0]
    spec = _rand(D, typing)
    with hjbdp.Backup(spec, variant=0) as bk:
        _walk_matrix(env, spec, bk, 0, ("v0", D, typing))


_TABLED_FORMS = set()


@pytest.mark.parametrize("i32", [1, 0])
@pytest.mark.parametrize("typing", ["f32", "f64", "f16s"])
@pytest.mark.parametrize("D", [3, 4])
def test_table_kernel_walk(env, D, typing, i32):
    """Variant 5 in its 32-bit form (tabled32_body: an `int` state index and stride behind xcd_share) and its 64-bit form."""
    hjbdp = env[0]
    spec = _rand(D, typing)
    with hjbdp.Backup(spec, variant=5) as bk:
        bk.set_option("tabled_i32", i32)
        assert bk.get_option("tabled_i32") == i32
        _walk_matrix(env, spec, bk, 5, ("v5", D, typing, i32))
        assert bk.get_option("tabled_i32") == i32
    _TABLED_FORMS.add(i32)


@pytest.mark.parametrize("typing", ["tab64", "cost64"])
def test_table_kernel_walk_float64_tables_and_costs(env, typing):
    """Variant 5 on a float32 problem with float64-built query tables / float64 cost terms (the typings only it and 6 / 7 serve)."""
    hjbdp, _abi, _ = env
    spec = _rand(3, typing)
    with hjbdp.Backup(spec, variant=5) as bk:
        inf = bk.info()
        assert (inf["cost_dtype"] == _abi.HJB_COST_F64) == (typing == "cost64")
        _walk_matrix(env, spec, bk, 5, ("v5", typing))


def test_both_table_kernel_forms_were_walked():
    """Runs after the parametrised cases."""
    assert _TABLED_FORMS == {0, 1}, _TABLED_FORMS


def test_packed_kernel_walk(env):
    """Variant 2: blocks of 512 states (two per thread)."""
    hjbdp = env[0]
    spec = _packed("c2", "f32")                        # 23,040 states = 45 blocks
    with hjbdp.Backup(spec, variant=2) as bk:
        _walk_matrix(env, spec, bk, 2, ("v2",))


_PACKED2_MODES = []

# (problem, storage, option sequences to try: each a list of (key, value) set after hjb_create, the matrix runs once per mode reached)
PACKED2 = [
    ("c2", "f32", ([], [("variant", 2), ("variant", 4)])),     # mode 4; forcing variant 2 first builds the axis-0 table: mode 1
    ("c2", "f16s", ([],)),
    ("c2ctrl", "f32", ([],)),
    ("c2ctrl", "f16s", ([],)),
    ("mixed", "f32", ([],)),
    ("win", "f32", ([], [("window_planes", 3)])),
    ("win", "f16s", ([],)),
    ("win_mono", "f32", ([("window_planes", 3)], [("window_planes", 4)])),
    ("win_mono", "f16s", ([("window_planes", 3)], [("window_planes", 4)])),
    ("win5", "f32", ([],)),
    ("win5_mono", "f32", ([("window_planes", 3)], [("window_planes", 4)])),
    ("rate", "f32", ([("uniwin", 0)], [("uniwin", 0), ("window_planes", 4)])),
]


@pytest.mark.parametrize("name,storage,sequences", PACKED2, ids=["%s_%s" % (c[0], c[1]) for c in PACKED2])
def test_packed2_kernel_walk(env, name, storage, sequences):
    """Variant 4 outside K15: the plain and C2-shape modes (the q / r split of every pass over the XCDs) and the window modes
    (XCD remap only at multiples of 8, chunks in transposed order, positions past the last chunk skipped), whose per-lane LDS
    windows, cell-change masks and prefetched cells are rebuilt for every further chunk a workgroup takes."""
    hjbdp, _abi, _ = env
    spec = _packed(name, storage)
    ran = []
    for seq in sequences:
        with hjbdp.Backup(spec) as bk:
            refused = False
            for key, value in seq:
                try:
                    bk.set_option(key, value)
                except hjbdp.HjbError as e:            # window_planes where the handle does not qualify (the inner control skips a cell)
                    assert key == "window_planes" and e.status == _abi.HJB_E_UNSUPPORTED, (name, key, value, str(e))
                    refused = True
            mode = bk.get_option("packed2_mode")
            assert bk.info()["kernel_variant"] == 4 and 0 <= mode <= 6, (name, seq, bk.info()["kernel_variant"], mode)
            if refused or mode in ran:
                continue
            _walk_matrix(env, spec, bk, 4, ("v4", name, storage, "mode %d" % mode))
            assert bk.get_option("packed2_mode") == mode
            ran.append(mode)
            _PACKED2_MODES.append((name, storage, mode))
    assert ran, (name, storage)


def test_packed2_mode_families_were_walked():
    """Runs after the parametrised cases: the plain mode, a C2-shape mode, a four-plane and a three-plane window mode."""
    modes = {m for _, _, m in _PACKED2_MODES}
    print("\n[walk] packed2 modes walked: %s" % sorted(_PACKED2_MODES))
    assert 0 in modes and modes & {1, 4} and modes & {2, 3} and modes & {5, 6}, _PACKED2_MODES
    assert {s for _, s, m in _PACKED2_MODES if m in (2, 3, 5, 6)} == {"f32", "f16s"}, _PACKED2_MODES


_CTRLSPLIT_FORMS = set()


@pytest.mark.parametrize("block", [256, 512, 1024])
@pytest.mark.parametrize("prec,dx,in_lds", [("single", 35, True), ("double", 35, True), ("single", 130, False), ("double", 95, False)])
def test_ctrlsplit_kernel_walk(env, prec, dx, in_lds, block):
    """Variant 3 on Kirk's problem (one wave per state, the 100 controls across its lanes, block / 64 states per workgroup pass):
    J staged in LDS once before the per-wave loop (1,225 states) and read from memory (16,900 float32 / 9,025 float64 states:
    more than 64 KiB)."""
    hjbdp = env[0]
    spec = _kirk(prec, dx)
    with hjbdp.Backup(spec, variant=3) as bk:
        bk.set_option("temporal", 0)
        assert bool(bk.info()["lds_bytes"]) == in_lds, bk.info()
        bk.set_option("block", block)
        assert bk.info()["block"] == block and bool(bk.info()["lds_bytes"]) == in_lds
        _walk_matrix(env, spec, bk, 3, ("v3", prec, dx, block))
    _CTRLSPLIT_FORMS.add(in_lds)


def test_both_ctrlsplit_forms_were_walked():
    """Runs after the parametrised cases."""
    assert _CTRLSPLIT_FORMS == {True, False}, _CTRLSPLIT_FORMS


_ROWWISE_FORMS = set()


@pytest.mark.parametrize("storage", ["f32", "f16s"])
@pytest.mark.parametrize("lean", [0, 1])
def test_rowwise_kernel_walk(env, lean, storage):
    """Variant 6 (one wave per 64-state chunk of a grid row, four per workgroup; 396 workgroups): the general form and the lean
    form, whose per-wave LDS scratch is reused item after item."""
    hjbdp = env[0]
    spec = _colsweep(storage)
    with hjbdp.Backup(spec, variant=6) as bk:
        bk.set_option("row_lean", lean)
        assert bk.get_option("row_lean") == lean and bool(bk.info()["lds_bytes"]) == bool(lean), bk.info()     # the form in effect
        W = _walk_matrix(env, spec, bk, 6, ("v6", lean, storage))
        assert W == 396
    _ROWWISE_FORMS.add(lean)


def test_both_rowwise_forms_were_walked():
    """Runs after the parametrised cases."""
    assert _ROWWISE_FORMS == {0, 1}, _ROWWISE_FORMS


# ---- beside the matrix ------------------------------------------------------------------------------------------------------------
SLABS = [
    # (id, variant, spec, options, (begin, end) of the last axis, the two multi-pass grids)
    ("v0", 0, lambda: _respec(_slab_rand(), dtype=np.float32), [], (8, 22), (7, 8)),
    ("v5", 5, lambda: _respec(_slab_rand(), dtype=np.float32), [], (8, 22), (7, 8)),
    ("v6", 6, lambda: _colsweep_g2(), [], (3, 8), (7, 16)),
    ("v4_window", 4, lambda: _packed("win", "f32"), [], (2, 7), (7, 8)),
    ("v4_window3", 4, lambda: _packed("rate", "f32"), [("uniwin", 0)], (1, 4), (7, 8)),
]


def _slab_rand():
    from problems import random_problem
    return random_problem(7100, (24, 22, 30), (4, 3), dtype=np.float64, index_base=1)


def _colsweep_g2():
    from problems import colsweep_problem
    return colsweep_problem(2, (70, 9, 8, 11), nU=9, gax=2, cost="fast")


@pytest.mark.parametrize("case", SLABS, ids=[c[0] for c in SLABS])
def test_slab_walk_leaves_the_halo_planes_alone(env, case):
    """A slab handle with halos under two multi-pass grids: the owned planes equal the oracle's stage of the slab, the halo
    planes of the NaN-prefilled output are still NaN (only owned planes may be written)."""
    hjbdp, _abi, c_oracle = env
    from problems import random_terminal
    _, variant, make, opts, (b, e), grids = case
    spec = make()
    term = random_terminal(spec, 21).astype(spec.j_dtype)
    with hjbdp.Backup(spec, variant=variant) as bk:
        for k, v in opts:
            bk.set_option(k, v)
        need = bk.info()
    hl, hh = min(need["halo_needed_lo"], b), min(need["halo_needed_hi"], spec.n[-1] - e)
    assert hl >= 1 and hh >= 1, (need["halo_needed_lo"], need["halo_needed_hi"])
    inner = spec.nS // spec.n[-1]
    sub = np.asfortranarray(term.reshape(inner, -1, order="F")[:, b - hl:e + hh]).reshape(-1, order="F")
    Jr, ir = c_oracle.backup_stage(_abi, spec, sub, slab=(b, e, hl, hh))
    own = slice(hl * inner, (hl + e - b) * inner)
    assert np.isfinite(Jr[own].astype(np.float64)).all()
    with hjbdp.Backup(spec, slab=(b, e, hl, hh), variant=variant) as bk:
        for k, v in opts:
            bk.set_option(k, v)
        inf = bk.info()
        assert inf["kernel_variant"] == variant and inf["j_elems"] == sub.size and inf["n_states"] == (e - b) * inner
        if variant == 4:
            assert bk.get_option("packed2_mode") in (2, 3, 5, 6)
        W = bk.get_option("grid")
        assert W == _work_units(spec, (e - b) * inner, variant, inf["block"])
        for G in grids:
            assert _passes(W, G) >= 2 and W % G != 0, (W, G)
            _set_grid(bk, G)
            _stage_into_prefilled(hjbdp, bk, spec, sub, Jr, ir, own, (case[0], "grid %d of W = %d" % (G, W)))


def test_multi_slab_sweep_under_a_small_grid(env):
    """hjb_multi_set_option forwards "grid" to every slab's whole-slab handle and to its boundary and interior part handles:
    three slabs of 15 workgroups each (their parts fewer) on the table kernel under a grid of 4, five stages against the oracle."""
    hjbdp, _abi, c_oracle = env
    from problems import nested_problem, random_terminal
    spec = nested_problem(11, (24, 22, 21), (4, 3), spread=0.03)         # the last axis moves by a few cells: halos narrower than a slab
    term = random_terminal(spec, 3)
    ref = c_oracle.sweep(_abi, spec, 5, terminal=term, keep_J=True, keep_idx=True)
    assert np.isfinite(ref["J_stages"]).all()
    with hjbdp.MultiBackup(spec, [0, 0, 0]) as mb:
        mb.set_option("variant", 5)                      # (the automatic choice for this shape has a launch of its own plan)
        infos = [mb.slab_info(i) for i in range(3)]
        assert [i["kernel_variant"] for i in infos] == [5, 5, 5], infos
        assert [i["end"] - i["begin"] for i in infos] == [7, 7, 7] and all(i["split"] for i in infos), infos
        assert _passes(_work_units(spec, 24 * 22 * 7, 5, 256), 4) >= 3
        mb.set_option("grid", 4)
        out = mb.solve(5, terminal=term, keep_J=True, keep_idx=True)
    assert np.array_equal(out["J_stages"], ref["J_stages"]) and np.array_equal(out["idx_stages"], ref["idx_stages"])
    assert np.array_equal(out["J"], ref["J"]) and np.array_equal(out["idx"], ref["idx"])


@pytest.mark.parametrize("variant", [5, 0])
def test_graph_replayed_sweep_under_a_small_grid(env, variant):
    """75 stages of a contracting problem: the 32-stage graph is captured with the multi-pass launch (set before the first solve)
    and replayed twice, the rest runs eagerly."""
    hjbdp, _abi, c_oracle = env
    from problems import nested_problem, random_terminal
    spec = nested_problem(8, (60, 50), (3,), dtype=np.float64, spread=0.05)           # 3,000 states = 12 workgroups
    term = random_terminal(spec, 4)
    n_st = 75
    ref = c_oracle.sweep(_abi, spec, n_st, terminal=term)
    assert np.isfinite(ref["J"]).all()
    with hjbdp.Backup(spec, variant=variant) as bk:
        bk.set_option("temporal", 0)
        W = bk.get_option("grid")
        assert bk.info()["kernel_variant"] == variant and W == 12
        _set_grid(bk, 5)                                  # three passes, the last one of two workgroups
        a = bk.solve(n_st, terminal=term)
        a2 = bk.solve(n_st, terminal=term)                # the cached graph
        assert bk.get_option("grid") == 5
        bk.set_option("graph", 0)
        b = bk.solve(n_st, terminal=term)
    for o in (a, a2, b):
        assert o["stages_done"] == n_st
        assert np.array_equal(o["J"], ref["J"]) and np.array_equal(o["idx"], ref["idx"])


def test_batched_table_kernel_with_a_grid_per_problem(env):
    """hjb_solve_batch copies every handle's grid into the batched launch (blockIdx.x >= its grid returns at once): three problems
    of 42, 23 and 47 workgroups under grids 5, 9 and 16 in ONE launch per stage."""
    hjbdp, _abi, c_oracle = env
    from problems import random_problem
    shapes = [(24, 22, 20), (20, 18, 16), (16, 30, 25)]
    specs = [random_problem(7300 + i, n, (4, 3), dtype=np.float32, index_base=1) for i, n in enumerate(shapes)]
    grids = [5, 9, 16]
    for spec, G in zip(specs, grids):
        assert _passes(-(-spec.nS // 256), G) >= 3 and -(-spec.nS // 256) % G != 0
    outs, _, variants, sizes = hjbdp.solve_batch(specs, STAGES, options=[{"variant": 5, "grid": G} for G in grids])
    assert variants == [5, 5, 5] and sizes == [3], (variants, sizes)
    for spec, o in zip(specs, outs):
        ref = c_oracle.sweep(_abi, spec, STAGES)
        assert np.isfinite(ref["J"]).all()
        assert o["stages_done"] == STAGES
        assert np.array_equal(o["J"], ref["J"]) and np.array_equal(o["idx"], ref["idx"])
