"""GPU tests (-m gpu): the stage kernels' ARGMIN on exact ties between controls of different stage cost.

The problems are tests/tie_problems.py's lattice problems (TIE_CASES): integer knots, whole-cell (half-, eighth-cell) moves,
integer costs and terminal - no operation of the canonical arithmetic rounds, and g_a + v_a == g_b + v_b with g_a != g_b, v read
from different cells, occurs in the first and in later stages; assert_ties asserts per case which kinds of tie occur (a first
minimiser in a later-visited group, a higher lane's later pass, an odd outer step, ...) before anything runs, and
tests/test_tie_problems.py asserts the same without a GPU.

The expected J and labels are tie_reference's: int64 fixed-point arithmetic that shares nothing with the C twin.  The twin's sweep
is compared as well, so that a difference says which side moved.  Bit for bit, no tolerance anywhere; every variant / form is
asserted before the launch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi, c_oracle


_TWIN = {}


def _members(env, name):
    """[(spec, terminal, exact reference, the twin's sweep)] of a registered case: conditions asserted, built once per module."""
    import tie_problems as TP
    if name not in _TWIN:
        _, _abi, c_oracle = env
        TP.assert_ties(name)
        out = []
        for spec, term, ref in TP.tie_case(name):
            if TP.TIE_CASES[name].dist is not None:           # the twin has no disturbance-aware stage
                out.append((spec, term, ref, ref))
                continue
            twin = c_oracle.sweep(_abi, spec, ref["J_stages"].shape[1], terminal=term, keep_J=True, keep_idx=True)
            out.append((spec, term, ref, twin))
        _TWIN[name] = out
    return _TWIN[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(J, idx, ref, twin, k, what):
    """Stage k of a result against the exact reference; on a difference the twin's agreement with either side is reported."""
    for key, got in (("J_stages", J), ("idx_stages", idx)):
        want, tw = ref[key][:, k], twin[key][:, k]
        if key == "J_stages":
            bad = np.flatnonzero(_bits(got) != _bits(want))
        else:
            bad = np.flatnonzero(np.asarray(got).astype(np.int64) != want)
        if bad.size:
            s = bad[:6]
            pytest.fail("%r %s stage %d: %d states differ from the exact reference, first %s: kernel %s exact %s twin %s" % (
                what, key, k, bad.size, s.tolist(), np.asarray(got)[s].tolist(), want[s].tolist(), tw[s].tolist()))


def _sweep(bk, member, what):
    spec, term, ref, twin = member
    stages = ref["J_stages"].shape[1]
    out = bk.solve(stages, terminal=term, keep_J=True, keep_idx=True)
    assert out["idx_stages"].dtype == spec.idx_np_dtype and out["J_stages"].dtype == spec.j_dtype
    for k in range(stages - 1, -1, -1):
        _same(out["J_stages"][:, k], out["idx_stages"][:, k], ref, twin, k, what)


FREE = ["free-%d-%s" % (D, t) for D in (1, 2, 4, 6) for t in ("float32", "float64")] + \
       ["free-2-uneven", "free-2-half", "free-2-tab64", "free-2-cost64", "free-2-u8"]
K5 = ["k5-c1", "k5-c2", "k5-c3", "k5-small"]


# ---- K1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in FREE if n not in ("free-2-tab64", "free-2-cost64")] + K5)
def test_generic_kernel(env, name):
    """K1 k_backup_generic (variant 0): one thread per state, sequential `<` - the kernel closest to the twin: float32, float64,
    uint8 labels, index_base 0 and 1, unequal spacings 1, 2, 4 (float64 query tables and float64 cost are the table-driven
    kernels': test_tabled_kernel, test_colsweep_kernel)."""
    hjbdp = env[0]
    for member in _members(env, name):
        with hjbdp.Backup(member[0], variant=0) as bk:
            assert bk.info()["kernel_variant"] == 0
            _sweep(bk, member, (name, 0))


# ---- K5 ------------------------------------------------------------------------------------------------------------------------
_K5_FORMS = set()


@pytest.mark.parametrize("block", [256, 1024])
@pytest.mark.parametrize("name", K5 + ["k5-big", "free-2-float32", "free-2-float64", "free-2-uneven", "free-4-float32", "free-6-float32"])
def test_ctrlsplit_kernel(env, name, block):
    """K5 k_backup_ctrlsplit (variant 3, csrc/kernels_ctrlsplit.h:57-114): lane l keeps the first minimum of controls l, l + 64, ...
    with `<`; the butterfly takes the smaller value and, on equal values, the smaller visiting index.  The k5 cases (7 x 7 states,
    130 / 135 / 150 controls in one, two and three control dims, and 50 controls: fewer than lanes) hold ties whose later member
    sits in a LOWER lane (a butterfly that preferred the lower lane would take it), ties inside one lane, and first minimisers in
    the last, partly filled pass; k5-big (130 x 130 states) is the form that reads J from memory.  Four and sixteen waves a block (256 is the smallest block the option takes)."""
    hjbdp = env[0]
    for member in _members(env, name):
        with hjbdp.Backup(member[0], variant=3) as bk:
            bk.set_option("temporal", 0)
            bk.set_option("block", block)
            inf = bk.info()
            assert inf["kernel_variant"] == 3 and inf["block"] == block
            assert bool(inf["lds_bytes"]) == (name != "k5-big"), inf
            _K5_FORMS.add((bool(inf["lds_bytes"]), block))
            _sweep(bk, member, (name, 3, block))


def test_ctrlsplit_forms_were_reached():
    assert _K5_FORMS == {(lds, block) for lds in (True, False) for block in (256, 1024)}, _K5_FORMS


# ---- K7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FREE + ["k5-c2", "colsweep-g3-cost64", "colsweep-g3-tab64"])
def test_tabled_kernel(env, name):
    """K7 k_backup_tabled (variant 5): both index forms (tabled_i32 1 / 0)."""
    hjbdp = env[0]
    for member in _members(env, name):
        for form in (1, 0):
            with hjbdp.Backup(member[0], variant=5) as bk:
                assert bk.info()["kernel_variant"] == 5
                bk.set_option("tabled_i32", form)
                assert bk.get_option("tabled_i32") == form
                _sweep(bk, member, (name, 5, form))


# ---- K8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["row-float32", "row-float64"])
def test_rowwise_kernel(env, name):
    """K8 k_backup_rowwise (variant 6): lean and plain forms (row_lean 1 / 0), two control dims of five levels."""
    hjbdp = env[0]
    for member in _members(env, name):
        for lean in (1, 0):
            with hjbdp.Backup(member[0], variant=6) as bk:
                assert bk.info()["kernel_variant"] == 6
                bk.set_option("row_lean", lean)
                assert bk.get_option("row_lean") == lean
                _sweep(bk, member, (name, 6, lean))


# ---- K2 ------------------------------------------------------------------------------------------------------------------------
NESTED = ["nested-%d-%s" % (D, mono) for D in (2, 3, 5, 6) for mono in ("inc", "dec", None)]


@pytest.mark.parametrize("name", NESTED + ["nested-3-float64"])
def test_nested_kernel(env, name):
    """K2 k_backup_nested (variant 1, csrc/kernels_nested.h:298): strict `<` across outer steps, the inner sweep inside.  Ties between
    two outer steps, between two inner controls of one step, and a visiting order that is not the label order (C = 3)."""
    hjbdp = env[0]
    for member in _members(env, name):
        with hjbdp.Backup(member[0], variant=1) as bk:
            assert bk.info()["kernel_variant"] == 1
            _sweep(bk, member, (name, 1))


# ---- K3 / K4 -------------------------------------------------------------------------------------------------------------------
_PACKED_MODES = {}


@pytest.mark.parametrize("variant", [2, 4])
@pytest.mark.parametrize("name", ["nested-%d-%s" % (D, mono) for D in (2, 3, 5, 6) for mono in ("inc", "dec")])
def test_packed_kernels(env, name, variant):
    """The packed kernels (variant 2 csrc/kernels_packed.h; variant 4 csrc/kernels_packed2.h:5,1096) keep MINIMA only - two outer
    steps per trip in the halves of packed instructions, v_min3 over control pairs - and recover the label afterwards by
    re-evaluating the winning step.  assert_ties has asserted ties between the two steps of one trip, between steps of different
    trips, between inner controls of one step, and ties whose first member is in an odd step (the upper half).  Every window mode
    the shapes reach is recorded for the test below."""
    hjbdp = env[0]
    for member in _members(env, name):
        with hjbdp.Backup(member[0], variant=variant) as bk:
            assert bk.info()["kernel_variant"] == variant
            if variant == 4:
                mode = bk.get_option("packed2_mode")
                _PACKED_MODES.setdefault(mode, []).append(name)
            _sweep(bk, member, (name, variant))
            if variant == 4 and mode == 5:
                bk.set_option("window_planes", 4)
                assert bk.get_option("packed2_mode") == 2
                _PACKED_MODES.setdefault(2, []).append(name)
                _sweep(bk, member, (name, variant, "four planes"))


# ---- K15 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rates", "rates-f16"])
def test_uniwin_kernel(env, name):
    """K15 (csrc/kernels_uniwin.h:657-671, variant 4 mode 7) at both chunk sizes (uw_block 64 and the default), then K3's
    three-plane (mode 5) and four-plane (mode 2) windows on the same handle; float32 and binary16 storage."""
    hjbdp = env[0]
    for member in _members(env, name):
        with hjbdp.Backup(member[0]) as bk:
            assert bk.info()["kernel_variant"] == 4 and bk.get_option("uniwin_ok") == 1
            bk.set_option("uniwin", 1)
            assert bk.get_option("packed2_mode") == 7 and bk.get_option("uniwin") == 1
            default = bk.get_option("uw_block")
            _sweep(bk, member, (name, "uniwin", default))
            bk.set_option("uw_block", 64)
            assert bk.get_option("uw_block") == 64 != default and bk.get_option("packed2_mode") == 7
            _sweep(bk, member, (name, "uniwin", 64))
            bk.set_option("uniwin", 0)
            assert bk.get_option("packed2_mode") == 5
            _PACKED_MODES.setdefault(5, []).append(name)
            _sweep(bk, member, (name, "mode 5"))
            bk.set_option("window_planes", 4)
            assert bk.get_option("packed2_mode") == 2
            _PACKED_MODES.setdefault(2, []).append(name)
            _sweep(bk, member, (name, "mode 2"))


def test_packed2_modes_were_reached():
    """Runs after the cases above: a window mode (2), the three-plane window (5) and a non-window mode were all run."""
    assert 2 in _PACKED_MODES and 5 in _PACKED_MODES, _PACKED_MODES
    assert set(_PACKED_MODES) - {2, 5}, _PACKED_MODES
    print("packed2 modes reached:", {k: len(v) for k, v in _PACKED_MODES.items()})


# ---- K10 / K13 -----------------------------------------------------------------------------------------------------------------
_CS_SPLITS = set()


@pytest.mark.parametrize("name", ["colsweep-g%d-%s" % (g, s) for g in (2, 3) for s in ("f32", "f16")] + ["colsweep-g3-tab64", "colsweep-g3-cost64"])
def test_colsweep_kernel(env, name):
    """K10 (variant 7, csrc/kernels_colsweep.h:20-31,152-166,290-291) visits the controls in PLAN order - group by group, the
    groups in ascending order of their highest control - and repairs the order with take_tie only in the slots the host flagged
    (csrc/hjbdp_colsweep.hip:109).  Over the seeds of a case every one of the 36 control pairs a < b occurs as (first minimiser,
    another minimiser of different stage cost), at least half of them in a later stage, and three-way ties occur (assert_ties).
    One-load and two-loads forms (cs_dpp 1 / 0), one and several parts per column (cs_split), float32 and binary16 storage;
    float64 query tables with uint8 labels and float64 cost on their own cases."""
    hjbdp = env[0]
    for i, member in enumerate(_members(env, name)):
        with hjbdp.Backup(member[0], variant=7) as bk:
            assert bk.info()["kernel_variant"] == 7
            assert bk.get_option("cs_group_axis") == int(name[10])
            assert bk.get_option("cs_dpp") == 1, "the host did not admit the one-load form"
            _sweep(bk, member, (name, i, "dpp 1"))
            bk.set_option("cs_dpp", 0)
            assert bk.get_option("cs_dpp") == 0
            _sweep(bk, member, (name, i, "dpp 0"))
            if i == 0:
                for dpp in (1, 0):
                    bk.set_option("cs_dpp", dpp)
                    for split in (1, 3):
                        bk.set_option("cs_split", split)
                        assert bk.get_option("cs_split") == split and bk.get_option("cs_dpp") == dpp
                        _CS_SPLITS.add(split)
                        _sweep(bk, member, (name, i, "dpp %d split %d" % (dpp, split)))


_COOP = []


@pytest.mark.parametrize("name", ["colsweep-g2-coop", "colsweep-g3-coop"])
def test_colsweep_cooperative_kernel(env, name):
    """K13 (csrc/kernels_colcoop.h, option cs_coop): the same plans, corner rows shared through LDS."""
    hjbdp = env[0]
    for member in _members(env, name):
        with hjbdp.Backup(member[0], variant=7) as bk:
            assert bk.info()["kernel_variant"] == 7 and bk.get_option("cs_coop") == 0
            _sweep(bk, member, (name, "plain"))
            bk.set_option("cs_coop", 1)
            assert bk.info()["kernel_variant"] == 7 and bk.get_option("cs_coop") == 1, ("not admitted", bk.get_option("cs_coop_why"))
            _COOP.append((name, bk.get_option("cs_coop"), bk.get_option("cs_coop_why")))
            _sweep(bk, member, (name, "coop"))


def test_colsweep_forms_were_reached():
    assert _COOP and all(on == 1 for _, on, _ in _COOP), _COOP
    assert _CS_SPLITS == {1, 3}, _CS_SPLITS


# ---- K9 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["local2d-f64-u4", "local2d-f64-u8", "local2d-f32-u4", "local2d-f32-u8", "local2d-tab64-u4"])
def test_tile2d_kernels(env, name):
    """K9 (csrc/kernels_tile2d.h): several stages per launch.  It applies from sixteen stages on and keeps no per-stage output, so
    the FINAL J and labels of sixteen stages (two launches of eight) are held to the exact reference; temporal = 2 makes hjb_solve
    fail unless K9 ran, temporal = 0 is one stage per launch.  Sixteen exact stages: float64 with half-cell moves, float32 (and
    float64 query tables) with whole-cell moves (tie_local2d_problem says why)."""
    hjbdp = env[0]
    for spec, term, ref, twin in _members(env, name):
        stages = ref["J_stages"].shape[1]
        assert stages == 16
        with hjbdp.Backup(spec) as bk:
            for temporal in (2, 0):
                bk.set_option("temporal", temporal)
                assert bk.get_option("temporal") == temporal
                out = bk.solve(stages, terminal=term)
                assert out["stages_done"] == stages
                _same(out["J"], out["idx"], ref, twin, 0, (name, temporal))


# ---- K24 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dist-%s-%s" % (mode, t) for mode in ("expect", "worst") for t in ("float32", "float64")])
def test_disturbed_kernel(env, name):
    """K24 k_backup_disturb (variant 8, csrc/kernels_disturb.h).  One zero node gives the undisturbed reference's labels and J.  Two
    nodes, whole-cell offsets: HJB_DIST_EXPECT with weights 1/2 against the exact restatement of the contract (acc = p_0 v_0, then
    fma(p_w, v_w, acc)), HJB_DIST_WORST against max_w - stage by stage from the exact reference's own J, both index forms.  Both
    cases hold ties between controls of different cost (assert_ties)."""
    import tie_problems as TP
    hjbdp = env[0]
    off, w, mode = TP.TIE_CASES[name].dist
    for spec, term, ref, _ in _members(env, name):
        stages = ref["J_stages"].shape[1]
        plain = TP.tie_reference(spec, term, 1)
        with hjbdp.Backup(spec) as bk:
            bk.set_disturbance(np.zeros((spec.D, 1)), None, "worst")
            assert bk.info()["kernel_variant"] == 8 and bk.info()["dist_nodes"] == 1
            J, idx = bk.backup_stage(term)
            _same(J, idx, plain, plain, 0, (name, "one zero node"))
            bk.set_disturbance(off, w, mode)
            assert bk.info()["kernel_variant"] == 8 and bk.info()["dist_nodes"] == 2 and bk.info()["dist_mode"] == mode
            for i32 in (1, 0):
                bk.set_option("dist_i32", i32)
                assert bk.get_option("dist_form") == i32
                for k in range(stages - 1, -1, -1):
                    J, idx = bk.backup_stage(term if k == stages - 1 else ref["J_stages"][:, k + 1])
                    _same(J, idx, ref, ref, k, (name, mode, i32))


# ---- slabs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("free-4-float32", 5), ("colsweep-g3-f32", 7)])
def test_three_slabs_with_ties_in_every_boundary_plane(env, name, variant):
    """Three slabs of the last axis ([0, 4), [4, 9), [9, 13)) of a K7 and of a K10 case, the first two stages of the sweep, each from
    the exact reference's own J: the owned planes equal the whole-grid exact reference.  In both stages every plane beside a cut
    (3, 4, 8, 9) holds a state with two or more minimisers of different stage cost - asserted from the reference (by the third stage
    the ties have thinned out to a handful of planes, so it is left to the whole-grid tests)."""
    hjbdp = env[0]
    spec, term, ref, twin = _members(env, name)[0]
    nl = spec.n[-1]
    inner = spec.nS // nl
    stages = ref["J_stages"].shape[1]
    g = ref["g"]
    with hjbdp.Backup(spec, variant=variant) as bk:
        need = bk.info()
    for k in (stages - 1, stages - 2):
        mask = ref["minimisers"][k]
        gmin = np.where(mask, g, np.inf).min(axis=1)
        gmax = np.where(mask, g, -np.inf).max(axis=1)
        mixed = (gmax > gmin).reshape(inner, nl, order="F")
        for plane in (3, 4, 8, 9):
            assert mixed[:, plane].any(), (name, k, plane)
    for b, e in ((0, 4), (4, 9), (9, 13)):
        lo, hi = min(need["halo_needed_lo"], b), min(need["halo_needed_hi"], nl - e)
        with hjbdp.Backup(spec, slab=(b, e, lo, hi), variant=variant) as bk:
            assert bk.info()["kernel_variant"] == variant
            for k in (stages - 1, stages - 2):
                Jn = (term if k == stages - 1 else ref["J_stages"][:, k + 1]).reshape(inner, nl, order="F")
                Jo, io = bk.backup_stage(np.asfortranarray(Jn[:, b - lo:e + hi]).reshape(-1, order="F"))
                got = np.ascontiguousarray(Jo.reshape(inner, -1, order="F")[:, lo:lo + e - b])
                want = np.ascontiguousarray(ref["J_stages"][:, k].reshape(inner, nl, order="F")[:, b:e])
                assert np.array_equal(_bits(got), _bits(want)), (name, b, e, k)
                wi = ref["idx_stages"][:, k].reshape(inner, nl, order="F")[:, b:e].reshape(-1, order="F")
                bad = np.flatnonzero(io.astype(np.int64) != wi)
                assert bad.size == 0, (name, b, e, k, bad.size, bad[:6].tolist())


# ---- hjb_solve_batch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [7, 5])
def test_batched_kernels(env, variant):
    """hjb_solve_batch (csrc/hjbdp_batch.hip): one launch per stage over two members of the column-sweep shape built from different
    seeds - the batched column sweep (variant 7) and the batched table kernel (variant 5); every member's final J and labels equal
    its own exact reference."""
    hjbdp, _abi, _ = env
    members = _members(env, "colsweep-g3-f32")[:2]
    assert not np.array_equal(members[0][2]["idx"], members[1][2]["idx"])
    bks = [hjbdp.Backup(m[0], variant=variant) for m in members]
    try:
        n = len(bks)
        optp, resp = (C.POINTER(_abi.hjb_solve_opts) * n)(), (C.POINTER(_abi.hjb_result) * n)()
        keep, outs = [], []
        for i, (bk, (spec, term, ref, twin)) in enumerate(zip(bks, members)):
            assert bk.info()["kernel_variant"] == variant
            o, r = _abi.hjb_solve_opts(), _abi.hjb_result()
            o.n_stages = ref["J_stages"].shape[1]
            t = np.ascontiguousarray(term, dtype=spec.j_dtype)
            o.terminal = t.ctypes.data
            J, idx = np.empty(spec.nS, dtype=spec.j_dtype), np.empty(spec.nS, dtype=spec.idx_np_dtype)
            o.J_final, o.idx_final = J.ctypes.data, idx.ctypes.data
            optp[i], resp[i] = C.pointer(o), C.pointer(r)
            keep += [o, r, t]
            outs.append((J, idx, r))
        hs = (C.c_void_p * n)(*[bk._h for bk in bks])
        st = bks[0].lib.hjb_solve_batch(n, hs, optp, resp)
        assert st == _abi.HJB_OK, bks[0].lib.hjb_last_error(bks[0]._h)
        for i, ((J, idx, r), (spec, term, ref, twin)) in enumerate(zip(outs, members)):
            assert r.stages_done == ref["J_stages"].shape[1]
            _same(J, idx, ref, twin, 0, ("batch", variant, i))
    finally:
        for bk in bks:
            bk.close()


# ---- K22 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["free-1-float64", "free-2-float32", "free-2-uneven", "free-2-tab64", "free-4-float64",
                                  "free-6-float32", "k5-c3"])
def test_evaluate_kernel_on_either_end_of_a_tie(env, name):
    """K22 k_evaluate (csrc/kernels_evaluate.h) decodes labels: evaluating the exact reference's FIRST-minimiser labels returns its
    J, and so does evaluating the labels of the LAST minimiser of every state - another control, another stage cost, other cells,
    the same total - bit for bit.  Both term sources where both exist (eval_tables 0 / 1) and both index widths (eval_i32)."""
    hjbdp, _abi, _ = env
    for spec, term, ref, twin in _members(env, name):
        stages = ref["J_stages"].shape[1]
        assert any(np.any(ref["idx_stages"][:, k] != ref["last_idx_stages"][:, k]) for k in range(stages))
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
                    for k in range(stages):
                        Jn = term if k == stages - 1 else ref["J_stages"][:, k + 1]
                        for which in ("idx_stages", "last_idx_stages"):
                            got = bk.evaluate_stage(Jn, ref[which][:, k].astype(spec.idx_np_dtype))
                            bad = np.flatnonzero(_bits(got) != _bits(ref["J_stages"][:, k]))
                            assert bad.size == 0, (name, src, i32, k, which, bad.size, bad[:6].tolist())
        assert 1 in ran and (0 in ran or spec.table_dtype is not None), ran
