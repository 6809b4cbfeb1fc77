"""GPU tests (-m gpu) of the disturbed backup (hjb_set_disturbance, kernel variant 8; csrc/kernels_disturb.h):
J_k(x) = min_u g + E_w / max_w F_{k+1}(x_next + d_w), and its fixed-label form behind hjb_evaluate*.

Bars, all bit for bit unless said otherwise: one zero node is the handle's own undisturbed backup under every typing; seeded node
sets equal tests/disturbance_refs.py (the contract of include/hjbdp.h restated in numpy); an affine cost-to-go gives the analytic
values; the fixed-label form returns the backup's J on its labels and the restatement on any; hjb_solve equals a host loop of
stages; the index forms and launch sizes agree.  The shapes are the smallest at which the thing tested can go wrong."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

from disturbance_refs import DisturbedRef

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi


def _retype(hjbdp, spec, **kw):
    args = dict(dtype=spec.dtype, index_base=spec.index_base, j_storage=None if spec.j_dtype == spec.dtype else spec.j_dtype,
                idx_dtype=spec.idx_dtype, table_dtype=spec.table_dtype, cost_dtype=spec.cost_dtype)
    args.update(kw)
    if args.get("table_dtype") is not None or args.get("cost_dtype") is not None:
        args["dtype"] = np.float32
    return hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, **args)


def _terminal(spec, seed):
    return np.random.default_rng(seed).random(spec.nS).astype(spec.j_dtype)


def _bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a


def _same(a, b):
    return a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _offsets(spec, axes, W, seed, cells=1.5):
    """W seeded nodes, up to `cells` mean cells of each listed axis either way; node 0 is NOT the nominal state."""
    rng = np.random.default_rng(seed)
    off = np.zeros((spec.D, W))
    for a in axes:
        h = (spec.knots[a][-1] - spec.knots[a][0]) / (spec.n[a] - 1)
        off[a] = cells * h * rng.uniform(-1.0, 1.0, W)
        off[a, rng.integers(0, W)] = cells * h * (1 if rng.random() < 0.5 else -1)       # the full reach, either side
    return off


def _weights(W, seed):
    w = np.random.default_rng(seed).uniform(0.2, 1.0, W)
    return w / w.sum()


# ---- 1. identity ---------------------------------------------------------------------------------------------------------------
GRIDS = [(7,), (7, 5), (6, 5, 4), (5, 4, 3, 3), (4, 3, 3, 3, 2), (3, 3, 3, 3, 3, 2)]
CONTROLS = [(5,), (3, 4), (3, 2, 2)]
IDX = [(np.int32, 0), (np.uint8, 1), (np.uint16, 0), (np.int32, 1), (np.uint8, 0), (np.uint16, 1)]


def _identity_case(env, spec, seed):
    """One zero node, both modes: the disturbed handle equals its own backup taken just before the setting, and again after
    clearing; kernel_variant reads 8 in between and the earlier variant afterwards."""
    hjbdp, _abi = env
    term = _terminal(spec, seed)
    with hjbdp.Backup(spec) as bk:
        J0, i0 = bk.backup_stage(term)
        v0 = bk.info()["kernel_variant"]
        assert v0 != 8 and bk.info()["dist_nodes"] == 0
        for mode, w in (("expect", None), ("expect", [1.0]), ("worst", None)):
            bk.set_disturbance(np.zeros((spec.D, 1)), w, mode)
            inf = bk.info()
            assert inf["kernel_variant"] == 8 and inf["dist_nodes"] == 1 and inf["dist_mode"] == mode and inf["dist_axes"] == 0
            J1, i1 = bk.backup_stage(term)
            assert _same(J1, J0) and _same(i1, i0), (mode, v0, int(np.sum(_bits(J1) != _bits(J0))), int(np.sum(i1 != i0)))
            assert _same(bk.evaluate_stage(term, i0), J0), mode
            bk.clear_disturbance()
            assert bk.info()["kernel_variant"] == v0 and bk.info()["dist_nodes"] == 0
            J2, i2 = bk.backup_stage(term)
            assert _same(J2, J0) and _same(i2, i0), mode
    return v0


@pytest.mark.parametrize("storage", ["f32", "f64", "f16"])
@pytest.mark.parametrize("case", range(len(GRIDS)))
def test_one_zero_node_is_the_undisturbed_backup(env, case, storage):
    hjbdp, _abi = env
    from problems import random_problem
    n = GRIDS[case]
    dtype = np.float64 if storage == "f64" else np.float32
    for k, nonuniform in enumerate((False, True)):
        sel = case + k + {"f32": 0, "f64": 1, "f16": 2}[storage]
        m = CONTROLS[sel % 3]
        idx_dtype, base = IDX[sel % len(IDX)]
        spec = random_problem(900 + 10 * case + k, n, m, dtype=dtype, nonuniform=nonuniform, index_base=base)
        spec = _retype(hjbdp, spec, j_storage=np.float16 if storage == "f16" else None, idx_dtype=idx_dtype)
        _identity_case(env, spec, seed=case)


def test_one_zero_node_under_float64_queries_and_costs(env):
    """HJB_TAB_F64 / HJB_COST_F64: the undisturbed handles run on the table-driven kernels (their tables are built in double);
    variant 8 forms the same queries from the float64 terms itself."""
    hjbdp, _abi = env
    from problems import colsweep_problem, pos_att_channel_spec, random_problem
    cs = colsweep_problem(1, (70, 9, 8, 11), nU=9, gax=3, cost="fast")
    seen = set()
    for spec in (_retype(hjbdp, cs, cost_dtype=np.float64), _retype(hjbdp, cs, table_dtype=np.float64, cost_dtype=np.float64),
                 _retype(hjbdp, cs, table_dtype=np.float64, j_storage=np.float16),
                 _retype(hjbdp, random_problem(31, (6, 5, 7), (3, 2), dtype=np.float32, nonuniform=True, index_base=1), table_dtype=np.float64,
                         idx_dtype=np.uint8),
                 pos_att_channel_spec("f64", n=12), pos_att_channel_spec("terms", n=12)):
        seen.add(_identity_case(env, spec, seed=5))
    assert seen & {5, 6, 7}, seen


# ---- 2. against the restatement ------------------------------------------------------------------------------------------------
# (storage / typing, n, m, nonuniform, offset axes or None = all, W, seed): every state of every grid; the seeds are the first from
# their case number (100 for two) at which the REFERENCE's queries meet the coverage condition the test asserts
REF_CASES = [
    ("f32", (9, 8, 7), (3, 2), True, (0, 2), 5, 11),
    ("f32", (6, 5, 4, 5), (4,), False, None, 9, 12),
    ("f32", (31,), (7,), True, None, 2, 13),
    ("f32", (4, 4, 4, 4, 3), (2, 3), False, (1, 4), 2, 14),
    ("f32", (4, 4, 4, 4, 4, 3), (2, 1, 2), False, (0, 5), 2, 100),
    ("f64", (12, 11), (5,), True, (1,), 2, 16),
    ("f64", (7, 6, 5), (2, 3), False, None, 9, 17),
    ("f16", (9, 8, 7), (4,), False, None, 5, 18),
    ("f16", (14, 13), (3, 3), True, (0,), 1, 100),
    ("tab64", (9, 8, 7), (3, 2), True, None, 5, 20),
    ("tab64+cost64", (14, 6, 5, 6), None, False, (2, 3), 9, 21),
    ("cost64", (14, 6, 5, 6), None, True, (0, 1), 5, 22),
    ("tab64+f16", (8, 7, 6), (4,), False, (2,), 2, 23),
]


def _ref_spec(hjbdp, typing, n, m, nonuniform, seed):
    from problems import colsweep_problem, random_problem
    if m is None:                                       # the column-sweep shape: float64 cost terms need a shape the tables fit
        spec = colsweep_problem(seed, n, nU=9, gax=3, cost="fast", nonuniform=nonuniform)
    else:
        spec = random_problem(seed, n, m, dtype=np.float64 if typing == "f64" else np.float32, nonuniform=nonuniform, index_base=seed % 2)
    kw = {}
    if "tab64" in typing:
        kw["table_dtype"] = np.float64
    if "cost64" in typing:
        kw["cost_dtype"] = np.float64
    if "f16" in typing:
        kw["j_storage"] = np.float16
    return _retype(hjbdp, spec, **kw)


@pytest.mark.parametrize("case", range(len(REF_CASES)))
def test_backup_equals_the_restatement(env, case):
    hjbdp, _abi = env
    typing, n, m, nonuniform, axes, W, seed = REF_CASES[case]
    spec = _ref_spec(hjbdp, typing, n, m, nonuniform, seed)
    axes = tuple(range(spec.D)) if axes is None else axes
    off = _offsets(spec, axes, W, seed)
    term = _terminal(spec, seed)
    with hjbdp.Backup(spec) as bk:
        for mode, w in (("expect", _weights(W, seed) if case % 2 else None), ("worst", None)):
            ref = DisturbedRef(spec, off, w, mode)
            assert ref.axes_mask == sum(1 << a for a in axes)
            if mode == "expect":
                # the inputs reach what can go wrong: extrapolation at both ends of every offset axis with >= 4 knots, and
                # (with more than one node) nodes of one (state, control) in different cells
                for a, (below, above, split) in ref.coverage().items():
                    assert (below and above) or spec.n[a] < 4, (a, below, above)
                    assert split or W == 1, a
            bk.set_disturbance(off, w, mode)
            assert bk.get_option("dist_axes") == ref.axes_mask and bk.get_option("dist_nodes") == W
            assert bk.get_option("dist_mode") == (_abi.HJB_DIST_WORST if mode == "worst" else _abi.HJB_DIST_EXPECT)
            J, idx = bk.backup_stage(term)
            Jr, ir = ref.backup(term)
            print("case %d %s: J differs at %d of %d states, labels at %d" % (case, mode, int(np.sum(_bits(J) != _bits(Jr))), spec.nS, int(np.sum(idx != ir))))
            assert _same(J, Jr), (mode, int(np.sum(_bits(J) != _bits(Jr))))
            assert _same(idx, ir), (mode, int(np.sum(idx != ir)))


# ---- 3. analytic ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_affine_cost_to_go_gives_the_analytic_values(env, dtype):
    """Independent of the restatement: integer knots, quarter-integer queries, integer slopes - every operation is exact."""
    hjbdp, _abi = env
    from test_disturbance_refs import affine_expected, affine_problem
    spec, J_next, slope = affine_problem(dtype)
    with hjbdp.Backup(spec) as bk:
        for axis in (0, 1):
            for mode in ("expect", "worst"):
                off = np.zeros((2, 2))
                off[axis] = (0.5, -0.5)
                bk.set_disturbance(off, (0.5, 0.5) if mode == "expect" else None, mode)
                want = affine_expected(spec, slope, axis, mode)
                J, idx = bk.backup_stage(J_next)
                assert np.array_equal(J.astype(np.float64), want.min(axis=1)), (axis, mode)
                assert np.array_equal(idx, np.argmin(want, axis=1) + spec.index_base), (axis, mode)
                for u in range(spec.nU):
                    got = bk.evaluate_stage(J_next.reshape(-1, order="F"), np.full(spec.nS, u + spec.index_base, dtype=spec.idx_np_dtype))
                    assert np.array_equal(got.astype(np.float64), want[:, u]), (axis, mode, u)


# ---- 4. ties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [(4,), (3, 2), (2, 3, 2)])
def test_ties_go_to_the_first_control(env, m):
    """Constant J_next and constant cost: every candidate is the same number, the first visited control wins under both modes -
    also through the cascade order of several control dims (label index_base = every dim's first level)."""
    hjbdp, _abi = env
    from problems import random_problem
    for base in (0, 1):
        r = random_problem(40, (6, 5, 4), m, dtype=np.float32, index_base=base)
        cost = [hjbdp.Term((0,), np.full(6, 0.75))] + [hjbdp.Term((3 + c,), np.full(m[c], 0.5)) for c in range(len(m))]
        spec = hjbdp.ProblemSpec(r.knots, m, r.next_terms, cost, dtype=np.float32, index_base=base)
        Jn = np.full(spec.nS, 2.5, dtype=np.float32)
        off = _offsets(spec, (0, 1, 2), 3, 41)
        with hjbdp.Backup(spec) as bk:
            for mode, w in (("expect", [0.25, 0.5, 0.25]), ("worst", None)):
                bk.set_disturbance(off, w, mode)
                J, idx = bk.backup_stage(Jn)
                assert (idx == base).all(), (mode, np.unique(idx))
                assert (J == np.float32(0.75 + 0.5 * len(m) + 2.5)).all(), mode      # (every operation exact: dyadic values and weights)


# ---- 5. fixed labels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typing", ["f32", "f64", "tab64+cost64"])
def test_fixed_labels_share_the_backups_candidates(env, typing):
    hjbdp, _abi = env
    n, m = ((14, 6, 5, 6), None) if "cost64" in typing else ((7, 6, 5), (3, 2))
    spec = _ref_spec(hjbdp, typing, n, m, True, 51)
    W = 5
    off = _offsets(spec, tuple(range(spec.D)), W, 52)
    term = _terminal(spec, 53)
    lab = np.random.default_rng(54).integers(spec.index_base, spec.index_base + spec.nU, spec.nS).astype(spec.idx_np_dtype)
    with hjbdp.Backup(spec) as bk:
        for mode, w in (("expect", _weights(W, 55)), ("worst", None)):
            bk.set_disturbance(off, w, mode)
            J, idx = bk.backup_stage(term)
            assert _same(bk.evaluate_stage(term, idx), J), mode                    # its own labels: its J
            got = bk.evaluate_stage(term, lab)
            assert _same(got, DisturbedRef(spec, off, w, mode).evaluate(term, lab)), mode
            assert (got >= J).all(), mode                                          # the same candidates: exact comparison
            # the sweep of a fixed policy goes through the same launch
            res = bk.evaluate(2, idx, terminal=term, keep_J=True)
            assert _same(res["J_stages"][:, 1], J)
            assert _same(res["J"], bk.evaluate_stage(J, idx))


def test_a_label_out_of_range_through_both_entries(env):
    hjbdp, _abi = env
    from problems import random_problem
    spec = random_problem(56, (7, 11, 13), (3, 2), dtype=np.float32, index_base=1)
    nS, nU = spec.nS, spec.nU
    term = _terminal(spec, 57)
    lab = np.random.default_rng(58).integers(1, nU + 1, nS).astype(np.int32)
    bad = lab.copy()
    bad[700] = nU + 1
    with hjbdp.Backup(spec) as bk:
        bk.set_disturbance(_offsets(spec, (0, 1, 2), 5, 59), None, "worst")
        want = bk.evaluate_stage(term, lab)
        for i32 in (1, 0):
            bk.set_option("dist_i32", i32)
            assert bk.get_option("dist_form") == i32
            with hjbdp.DeviceBuffer(term.nbytes) as dIn, hjbdp.DeviceBuffer(term.nbytes) as dOut, hjbdp.DeviceBuffer(bad.nbytes) as dL:
                dIn.upload(term)
                dL.upload(bad)
                dOut.upload(np.zeros(nS, dtype=np.float32))
                bk.evaluate_stage_device(dIn, dL, dOut)
                with pytest.raises(hjbdp.HjbError) as ei:
                    bk.check_device_status()
                assert ei.value.status == _abi.HJB_E_INVALID and "label" in str(ei.value)
                bk.check_device_status()                                       # once: HJB_OK afterwards
                got = dOut.download(np.float32)
                assert np.array_equal(np.flatnonzero(np.isnan(got)), [700])    # NaN at that state only
                keep = np.arange(nS) != 700
                assert np.array_equal(got[keep], want[keep])
        # the host entry looks first: refused, outputs untouched
        out = np.full(nS, -7.0, dtype=np.float32)
        st = bk.lib.hjb_evaluate_stage(bk._h, term.ctypes.data, bad.ctypes.data, out.ctypes.data)
        assert st == _abi.HJB_E_INVALID and (out == -7.0).all()
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.evaluate(2, bad)
        assert ei.value.status == _abi.HJB_E_INVALID
        assert np.array_equal(bk.evaluate_stage(term, lab), want)


# ---- 6. the sweep --------------------------------------------------------------------------------------------------------------
def _local_2d(hjbdp, n=(35, 20), dtype=np.float32):
    """A local 2-D problem (every query within one cell of its state): undisturbed, hjb_solve runs it several stages per launch."""
    rng = np.random.default_rng(n[0])
    kx, kv = np.linspace(-0.5, 0.5, n[0]), np.linspace(-0.4, 0.6, n[1])
    hx, hv = kx[1] - kx[0], kv[1] - kv[0]
    U = np.array([-0.26, 0.0, 0.13, 0.26])
    nxt = [[hjbdp.Term((0,), kx), hjbdp.Term((1,), 0.9 * hx * np.sin(3 * kv))],
           [hjbdp.Term((1,), kv), hjbdp.Term((0,), 0.4 * hv * np.cos(5 * kx)), hjbdp.Term((2,), 0.55 * hv * U / 0.26)]]
    cost = [hjbdp.Term((0,), 6 * kx ** 2), hjbdp.Term((1,), 3 * kv ** 2), hjbdp.Term((2,), 0.1 * U ** 2), hjbdp.Term((0, 1), 0.05 * rng.random(n))]
    return hjbdp.ProblemSpec([kx, kv], [len(U)], nxt, cost, dtype=dtype, index_base=1)


K_TILE = 8          # csrc/kernels_tile2d.h kTileK: stages per launch of the several-stages-per-launch path


@pytest.mark.parametrize("mode", ["expect", "worst"])
def test_solve_equals_a_host_loop_of_stages(env, mode):
    hjbdp, _abi = env
    spec = _local_2d(hjbdp)
    n_st = 2 * K_TILE + 1
    W = 5
    off = _offsets(spec, (0, 1), W, 61, cells=0.8)
    w = _weights(W, 62) if mode == "expect" else None
    with hjbdp.Backup(spec) as bk:
        bk.set_option("temporal", 2)
        nominal = bk.solve(n_st)                        # undisturbed, this problem takes the several-stages-per-launch path
        bk.set_option("temporal", 1)
        bk.set_disturbance(off, w, mode)
        out = bk.solve(n_st, keep_J=True, keep_idx=True)
        J = np.zeros(spec.nS, dtype=spec.j_dtype)
        sums = {}
        for k_s in range(n_st, 0, -1):                  # the host loop: stage k_s in column k_s - 1
            J, idx = bk.backup_stage(J)
            assert _same(out["J_stages"][:, k_s - 1], J) and _same(out["idx_stages"][:, k_s - 1], idx), k_s
            sums[k_s] = float(np.sum(J.astype(np.float64)))
        assert _same(out["J"], J) and _same(out["idx"], idx)
        assert not _same(nominal["J"], J)
        plain = bk.solve(n_st)                          # no per-stage outputs: what would have been tiled
        assert _same(plain["J"], J) and _same(plain["idx"], idx) and plain["stages_done"] == n_st
        for (Jr, ir), k_s in zip(DisturbedRef(spec, off, w, mode).sweep(n_st), range(n_st, 0, -1)):
            assert _same(out["J_stages"][:, k_s - 1], Jr) and _same(out["idx_stages"][:, k_s - 1], ir), k_s
        # several stages per launch, when required, is refused; when merely allowed it was silently not taken (above)
        bk.set_option("temporal", 2)
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.solve(n_st)
        assert ei.value.status == _abi.HJB_E_UNSUPPORTED
        bk.set_option("temporal", 1)
        # the monitor: stop at the monitor point the host loop's own sums say
        period = 4
        pts = [k for k in range(n_st, 0, -1) if k % period == 0]
        e, prev = [], 0.0
        for k in pts:
            e.append(abs(sums[k] - prev))
            prev = sums[k]
        order = np.argsort(e)
        assert e[order[1]] > e[order[0]] * (1 + 1e-6)
        tol = 0.5 * (e[order[0]] + e[order[1]])
        stop = next(k for k, ek in zip(pts, e) if ek < tol)
        mon = bk.solve(n_st, monitor_period=period, monitor_tol=tol)
        assert mon["stages_done"] == n_st - stop + 1 and mon["stopped_early"]
        # graph replay: an ordinary launch, captured and replayed
        long = 2 * 32 + 6
        bk.set_option("graph", 1)
        g1 = bk.solve(long)
        bk.set_option("graph", 0)
        g0 = bk.solve(long)
        assert _same(g1["J"], g0["J"]) and _same(g1["idx"], g0["idx"]) and g1["stages_done"] == long


# ---- 7. forms and launches -----------------------------------------------------------------------------------------------------
def test_index_forms_and_launch_sizes_give_the_same_bits(env):
    hjbdp, _abi = env
    from problems import random_problem
    spec = random_problem(71, (7, 6, 7, 7), (3,), dtype=np.float32, nonuniform=True, index_base=1)
    off = _offsets(spec, (0, 1, 2, 3), 5, 72)
    term = _terminal(spec, 73)
    with hjbdp.Backup(spec) as bk:
        bk.set_disturbance(off, _weights(5, 74), "expect")
        assert bk.get_option("dist_form") == 1 and bk.get_option("dist_i32") == 1
        J, idx = bk.backup_stage(term)
        auto_grid = bk.get_option("grid")
        assert auto_grid == -(-spec.nS // 256)
        for i32 in (0, 1):
            bk.set_option("dist_i32", i32)
            assert bk.get_option("dist_form") == i32
            for grid in (1, 3, auto_grid):
                bk.set_option("grid", grid)
                bk.set_option("eval_grid", 0 if grid == auto_grid else grid)
                assert bk.get_option("grid") == grid
                J1, i1 = bk.backup_stage(term)
                assert _same(J1, J) and _same(i1, idx), (i32, grid)
                assert _same(bk.evaluate_stage(term, idx), J), (i32, grid)
        bk.set_option("eval_i32", 0)                      # the predicate is the fixed-label stage's own: one statement of it
        assert bk.get_option("dist_form") == 0
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.set_option("dist_form", 1)
        assert ei.value.status == _abi.HJB_E_INVALID


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was(env):
    hjbdp, _abi = env
    from problems import random_problem
    spec = random_problem(81, (6, 5, 4), (3, 2), dtype=np.float32, index_base=1)
    D = spec.D
    term = _terminal(spec, 82)
    off = np.asfortranarray(_offsets(spec, (0, 2), 3, 83))
    dp = C.POINTER(C.c_double)
    good = off.ctypes.data_as(dp)
    nan_off = off.copy(order="F")
    nan_off[1, 2] = np.nan
    inf_off = off.copy(order="F")
    inf_off[0, 0] = np.inf
    w_ok = np.array([0.2, 0.3, 0.5])
    w_neg = np.array([0.6, -0.1, 0.5])
    w_nan = np.array([0.2, np.nan, 0.5])
    E, W_ = _abi.HJB_DIST_EXPECT, _abi.HJB_DIST_WORST
    invalid = [("mode", (2, 3, good, None)), ("mode", (-1, 3, good, None)), ("n_nodes", (E, -1, good, None)),
               ("n_nodes", (E, _abi.HJB_DIST_MAX_NODES + 1, good, None)), ("null offsets", (E, 3, None, None)),
               ("not finite", (E, 3, nan_off.ctypes.data_as(dp), None)), ("not finite", (W_, 3, inf_off.ctypes.data_as(dp), None)),
               ("weight", (E, 3, good, w_neg.ctypes.data_as(dp))), ("weight", (E, 3, good, w_nan.ctypes.data_as(dp))),
               ("no weights", (W_, 3, good, w_ok.ctypes.data_as(dp)))]
    with hjbdp.Backup(spec) as bk:
        lib = bk.lib
        assert lib.hjb_set_disturbance(None, E, 3, good, None) == _abi.HJB_E_INVALID
        for disturbed in (False, True):
            if disturbed:
                bk.set_disturbance(off, w_ok, "expect")
            J0, i0 = bk.backup_stage(term)
            inf0 = bk.info()
            for text, args in invalid:
                assert lib.hjb_set_disturbance(bk._h, *args) == _abi.HJB_E_INVALID, (text, args[:2])
                assert text.encode() in lib.hjb_last_error(bk._h), (text, lib.hjb_last_error(bk._h))
                assert bk.info() == inf0
                J1, i1 = bk.backup_stage(term)
                assert _same(J1, J0) and _same(i1, i0), text
        # while a disturbance is set: no other variant, no probe, no several-stages-per-launch on demand
        for v in range(8):
            with pytest.raises(hjbdp.HjbError) as ei:
                bk.set_option("variant", v)
            assert ei.value.status == _abi.HJB_E_UNSUPPORTED and "variant 8 only" in str(ei.value)
        probe = {"lo": (0,) * D, "hi": (2,) * D, "control": (0, 0), "want": ("g",)}
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.solve(3, probe=probe)
        assert ei.value.status == _abi.HJB_E_UNSUPPORTED and "probe" in str(ei.value)
        J1, i1 = bk.backup_stage(term)
        assert _same(J1, J0) and _same(i1, i0)
        bk.clear_disturbance()
        assert bk.solve(3, probe=probe)["probe"]["g"].shape == (2,) * D + (3,)
    # a slab handle and a handle with a state model take none
    with hjbdp.Backup(spec, slab=(1, 3, 1, 1)) as bk:
        inf0 = bk.info()
        assert bk.lib.hjb_set_disturbance(bk._h, E, 3, good, None) == _abi.HJB_E_UNSUPPORTED
        assert b"slab" in bk.lib.hjb_last_error(bk._h) and bk.info() == inf0 and inf0["kernel_variant"] != 8
    sa = hjbdp.Solver_attitude(n_mesh_w=9, n_mesh_q=4)
    sa.U_vector = np.linspace(-0.11, 0.11, 5)
    mspec = sa.build_spec_model()
    moff = np.asfortranarray(np.full((6, 2), 0.01))
    with hjbdp.Backup(mspec) as bk:
        assert bk.lib.hjb_set_disturbance(bk._h, W_, 2, moff.ctypes.data_as(dp), None) == _abi.HJB_E_UNSUPPORTED
        assert b"model" in bk.lib.hjb_last_error(bk._h) and bk.info()["kernel_variant"] == 4 and bk.info()["dist_nodes"] == 0


def test_solve_batch_refuses_a_disturbed_member_and_the_python_side_falls_back(env):
    hjbdp, _abi = env
    from problems import random_problem
    n_st = 5
    specs = [random_problem(85 + i, (9, 8, 7), (3,), dtype=np.float32, index_base=1) for i in range(2)]
    off = _offsets(specs[0], (0, 1), 3, 86)
    bks = [hjbdp.Backup(s) for s in specs]
    try:
        for bk in bks:
            bk.set_option("variant", 5)                  # the table kernel's 32-bit form: a group hjb_solve_batch takes
        keep, optp, resp = [], (C.POINTER(_abi.hjb_solve_opts) * 2)(), (C.POINTER(_abi.hjb_result) * 2)()
        outs = []
        for k, s in enumerate(specs):
            o, r = _abi.hjb_solve_opts(), _abi.hjb_result()
            o.n_stages = n_st
            J, idx = np.empty(s.nS, dtype=s.j_dtype), np.empty(s.nS, dtype=s.idx_np_dtype)
            o.J_final, o.idx_final = J.ctypes.data, idx.ctypes.data
            keep += [o, r]
            outs.append((J, idx))
            optp[k], resp[k] = C.pointer(o), C.pointer(r)
        hs = (C.c_void_p * 2)(*[bk._h for bk in bks])
        lib = bks[0].lib
        assert lib.hjb_solve_batch(2, hs, optp, resp) == _abi.HJB_OK
        plain = [bk.solve(n_st) for bk in bks]
        assert all(_same(J, p["J"]) and _same(idx, p["idx"]) for (J, idx), p in zip(outs, plain))
        bks[1].set_disturbance(off, None, "worst")
        assert lib.hjb_solve_batch(2, hs, optp, resp) == _abi.HJB_E_UNSUPPORTED
        assert b"disturbance" in lib.hjb_last_error(bks[1]._h)
        want = [bks[0].solve(n_st), bks[1].solve(n_st)]
    finally:
        for bk in bks:
            bk.close()
    dspecs = [specs[0], _retype(hjbdp, specs[1], disturbance=(off, None, "worst"))]
    got, _, variants, sizes = hjbdp.solve_batch(dspecs, n_st)
    assert variants[1] == 8 and sizes == [1, 1]
    assert all(_same(g["J"], w["J"]) and _same(g["idx"], w["idx"]) for g, w in zip(got, want))
    assert not _same(want[1]["J"], plain[1]["J"])


# ---- 9. mirrors ----------------------------------------------------------------------------------------------------------------
def test_dynamic_solver_runs_and_judges_its_policy_under_the_disturbance(env):
    hjbdp, _abi = env

    def solver(dist):
        ds = hjbdp.Dynamic_Solver(precision="double")
        ds.N, ds.dx, ds.du = 9, 21, 40
        ds.disturbance = dist
        return ds.run()
    off, w = hjbdp.gaussian_nodes([0.08, 0.12], order=3)
    ds = solver((off, w, "expect"))
    pc = ds.policy_cost()
    assert pc.shape == (21, 21, 8) and np.array_equal(pc, ds.J_star[:, :, :8])      # the stored per-stage labels: the run's own J
    nominal = solver(None)
    assert not np.array_equal(nominal.J_star, ds.J_star)
    assert np.array_equal(nominal.policy_cost(), nominal.J_star[:, :, :8])
    ds.disturbance = None                               # the same labels judged on the nominal plant: another cost
    assert not np.array_equal(ds.policy_cost(), pc)


def test_pos_att_relabelling_permutes_the_offset_rows(env):
    """One channel at n = 12, offsets on the v axis only (rows (x, v, theta, w)), worst case.  axis_order "auto" runs the channel
    as (x, theta, w, v): bit-equal to a handle built in that order with the rows permuted BY HAND, and equal to the run in the
    reference's own order up to the order of the 1-D lerps - a few float32 ulp per stage (3 stages here:
    bound 1e-5 of max J, three orders above that and three below what a row on the wrong axis changes, asserted too)."""
    hjbdp, _abi = env
    n_st = 3

    def channel(order, dist):
        pa = hjbdp.Solver_pos_att()
        pa.n_mesh_x = pa.n_mesh_v = pa.n_mesh_t = pa.n_mesh_w = 12
        pa.axis_order = order
        pa.disturbance = dist
        sx, sv, st, sw = pa.grids()
        args = (sx, sv, st[0], sw, pa.F_Thr0, pa.F_Thr1, pa.F_Thr6, pa.F_Thr7, pa.Qx1, pa.Qv1, pa.Qt1, pa.Qw1, pa.R1, pa.J2)
        ctl = pa.calculate_one_channel_U_Opt(*args, "controller_x", n_stages=n_st)
        return pa, args, ctl["F_gI_Values"], ctl["U_Optimal_id"]
    pa0 = hjbdp.Solver_pos_att()
    pa0.n_mesh_x = pa0.n_mesh_v = pa0.n_mesh_t = pa0.n_mesh_w = 12
    sv = pa0.grids()[1]
    hv = sv[1] - sv[0]
    off = np.zeros((4, 3))
    off[1] = (0.0, 0.9 * hv, -0.9 * hv)
    dist = (off, None, "worst")
    pa, args, J_auto, U_auto = channel("auto", dist)
    spec, _ = pa.build_channel_spec(*args)
    order = hjbdp.suggest_axis_order(spec)
    assert order is not None and tuple(order) != (0, 1, 2, 3)
    # by hand: the undisturbed spec relabelled, then the rows listed in the new order
    bare = _retype(hjbdp, spec, disturbance=None)
    pspec, to_old = hjbdp.permute_state_axes(bare, order)
    hand = _retype(hjbdp, pspec, disturbance=(off[list(order)], None, "worst"))
    with hjbdp.Backup(hand) as bk:
        assert bk.get_option("dist_axes") == 1 << list(order).index(1)
        out = bk.solve(n_st, monitor_period=pa.monitor_period, monitor_tol=pa.monitor_tol, monitor_single=pa.monitor_single)
    assert np.array_equal(to_old(out["J"]).reshape(spec.n, order="F"), J_auto)
    assert np.array_equal(to_old(out["idx"]).reshape(spec.n, order="F"), U_auto)
    _, _, J_ref, _ = channel(None, dist)
    scale = float(np.abs(J_ref).max())
    assert np.abs(J_auto - J_ref).max() <= 1e-5 * scale
    wrong = np.zeros((4, 3))
    wrong[3] = off[1]                                  # the same numbers on the w axis
    _, _, J_wrong, _ = channel(None, (wrong, None, "worst"))
    assert np.abs(J_wrong - J_ref).max() > 1e-2 * scale


# ---- 10. budget ----------------------------------------------------------------------------------------------------------------
def test_no_scratch_and_no_lds_in_the_built_kernels(built, tmp_path):
    """Read from the code objects inside the built library (llvm-objdump --offloading, llvm-readelf --notes): every
    k_backup_disturb instantiation - 5 typings x D 1..6 x 2 index forms x 2 label forms - without LDS; none at D <= 4 with scratch."""
    tools = "/opt/rocm/lib/llvm/bin"
    objdump = shutil.which("llvm-objdump", path=tools) or shutil.which("llvm-objdump")
    readelf = shutil.which("llvm-readelf", path=tools) or shutil.which("llvm-readelf")
    assert objdump and readelf, "llvm-objdump / llvm-readelf of the ROCm toolchain not found"
    lib = tmp_path / "libhjbdp.so"
    shutil.copy(built.LIB, lib)
    r = subprocess.run([objdump, "--offloading", lib.name], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    for co in sorted(tmp_path.glob("libhjbdp.so.*gfx950*")):
        notes = subprocess.run([readelf, "--notes", co.name], cwd=tmp_path, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:                     # one block per kernel of the code object
            m = re.search(r"\.name:\s+(\S*k_backup_disturb\S*)", blk)
            if m:
                found[m.group(1)] = (int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)),
                                     int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    assert len(found) == 5 * 6 * 2 * 2, len(found)
    for name, (lds, scratch) in found.items():
        D = int(re.search(r"Li(\d)E", name).group(1))
        assert lds == 0, (name, lds)
        assert scratch == 0 or D > 4, (name, scratch)
