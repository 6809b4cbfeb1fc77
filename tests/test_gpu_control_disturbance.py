"""GPU tests (-m gpu) of the backup under a control-dependent disturbance (hjb_set_control_disturbance, kernel variant 8 in its
per-control form; csrc/kernels_ctrldist.h):  J_k(x) = min_u g + E_w / max_w F_{k+1}(x_next + d_w(u)), and its fixed-label form.

Every comparison is bit for bit.  A table constant along the control is the additive disturbance (hjb_set_disturbance) on the same
handle under every typing; seeded tables that differ along every control dim equal tests/control_disturbance_refs.py (the contract
of include/hjbdp.h restated in numpy); every slice of a table is that label's node set; an affine cost-to-go gives the analytic
values; the fixed-label form shares the min form's candidates; hjb_solve equals a host loop of stages; the index forms and launch
sizes agree; switching between the two settings, growing and shrinking tables and every refusal leave the handle's bits as they
were.  Shapes are those of tests/test_gpu_disturbance.py: the smallest at which the thing tested can go wrong."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

from control_disturbance_refs import ControlDisturbedRef
from test_gpu_disturbance import CONTROLS, GRIDS, IDX, K_TILE, _bits, _local_2d, _offsets, _ref_spec, _retype, _same, _terminal, _weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi


def _table(spec, axes, W, seed, cells=1.5):
    """A seeded [D, W, nU] table, up to `cells` mean cells of each listed axis either way, different for every (node, control);
    the full reach is met on either side at some (node, control)."""
    rng = np.random.default_rng(seed)
    off = np.zeros((spec.D, W, spec.nU))
    for a in axes:
        h = (spec.knots[a][-1] - spec.knots[a][0]) / (spec.n[a] - 1)
        off[a] = cells * h * rng.uniform(-1.0, 1.0, (W, spec.nU))
        for sign in (1.0, -1.0):
            off[a, rng.integers(0, W), rng.integers(0, spec.nU)] = sign * cells * h
    return off


def _misread_tables(spec, off):
    """The tables a decode mix-up would read: entry l taken from the VISITING index of label l (control dim 0 slowest) instead, and
    from the label with two equally long control dims swapped.  Empty with one control dim."""
    if spec.C == 1:
        return []
    sub = np.unravel_index(np.arange(spec.nU), spec.m, order="F")            # label -> per-dim indices
    out = [off[:, :, np.ravel_multi_index(sub, spec.m, order="C")]]           # ... -> its visiting index
    for c0 in range(spec.C):
        for c1 in range(c0 + 1, spec.C):
            if spec.m[c0] == spec.m[c1]:
                sw = list(sub)
                sw[c0], sw[c1] = sw[c1], sw[c0]
                out.append(off[:, :, np.ravel_multi_index(sw, spec.m, order="F")])
    return out


TYPINGS = ["f32", "f64", "f16", "tab64", "tab64+cost64", "cost64", "tab64+f16"]


def _typed(hjbdp, spec, typing):
    kw = {}
    if "tab64" in typing:
        kw["table_dtype"] = np.float64
    if "cost64" in typing:
        kw["cost_dtype"] = np.float64
    if "f16" in typing:
        kw["j_storage"] = np.float16
    return _retype(hjbdp, spec, **kw)


# ---- 1. a table constant along the control is the additive disturbance ------------------------------------------------------------------
@pytest.mark.parametrize("typing", TYPINGS)
@pytest.mark.parametrize("case", range(len(GRIDS)))
def test_a_constant_table_is_the_additive_disturbance(env, case, typing):
    hjbdp, _abi = env
    from problems import random_problem
    n = GRIDS[case]
    sel = case + TYPINGS.index(typing)
    m = CONTROLS[sel % 3]
    idx_dtype, base = IDX[sel % len(IDX)]
    spec = random_problem(1900 + 10 * case, n, m, dtype=np.float64 if typing == "f64" else np.float32, nonuniform=bool(sel % 2), index_base=base)
    spec = _typed(hjbdp, _retype(hjbdp, spec, idx_dtype=idx_dtype), typing)
    D, W = spec.D, 3
    term = _terminal(spec, case)
    off = _offsets(spec, tuple(range(0, D, 2)), W, 1000 + case)
    const = np.repeat(off[:, :, None], spec.nU, axis=2)
    with hjbdp.Backup(spec) as bk:
        J0, i0 = bk.backup_stage(term)
        v0 = bk.info()["kernel_variant"]
        for mode, w in (("expect", _weights(W, case)), ("worst", None)):
            bk.set_disturbance(off, w, mode)
            inf = bk.info()
            assert inf["kernel_variant"] == 8 and not inf["dist_ctrl"]
            Ja, ia = bk.backup_stage(term)
            bk.set_control_disturbance(const, w, mode)
            inf = bk.info()
            assert inf["kernel_variant"] == 8 and inf["dist_ctrl"] and inf["dist_nodes"] == W and inf["dist_mode"] == mode
            assert inf["dist_axes"] == sum(1 << a for a in range(0, D, 2))
            Jc, ic = bk.backup_stage(term)
            assert _same(Jc, Ja) and _same(ic, ia), (mode, int(np.sum(_bits(Jc) != _bits(Ja))), int(np.sum(ic != ia)))
            assert _same(bk.evaluate_stage(term, ia), Ja), mode
            assert not _same(Ja, J0)
            # one zero node, for every control: the undisturbed backup; and again after clearing
            bk.set_control_disturbance(np.zeros((D, 1, spec.nU)), [1.0] if mode == "expect" else None, mode)
            assert bk.info()["kernel_variant"] == 8 and bk.get_option("dist_ctrl") == 1 and bk.get_option("dist_axes") == 0
            J1, i1 = bk.backup_stage(term)
            assert _same(J1, J0) and _same(i1, i0), (mode, v0)
            assert _same(bk.evaluate_stage(term, i0), J0), mode
            bk.clear_disturbance()
            inf = bk.info()
            assert inf["kernel_variant"] == v0 and inf["dist_nodes"] == 0 and not inf["dist_ctrl"]
            J2, i2 = bk.backup_stage(term)
            assert _same(J2, J0) and _same(i2, i0), mode


# ---- 2. against the restatement ------------------------------------------------------------------------------------------------
# (typing, n, m (None: the column-sweep shape, 9 controls), nonuniform, offset axes or None = all, W, seed): every state of every grid.
# The seed of a case is its number: at each the REFERENCE alone meets the conditions the test asserts (reference_conditions) -
# checked on the CPU, before any kernel ran
REF_CASES = [
    ("f32", (9, 8, 7), (3, 2), True, (0, 2), 5, 0),
    ("f32", (6, 5, 4, 5), (4,), False, None, 9, 1),
    ("f32", (31,), (7,), True, None, 2, 2),
    ("f32", (4, 4, 4, 4, 3), (2, 3), False, (1, 4), 2, 3),
    ("f32", (4, 4, 4, 4, 4, 3), (2, 3, 2), False, (0, 5), 2, 4),
    ("f64", (12, 11), (5,), True, (1,), 1, 5),
    ("f64", (7, 6, 5), (2, 3, 2), False, None, 9, 6),
    ("f16", (9, 8, 7), (2, 3, 2), True, None, 5, 7),
    ("f16", (14, 13), (3, 2), True, (0,), 1, 8),
    ("tab64", (9, 8, 7), (3, 2), True, None, 5, 9),
    ("tab64+cost64", (14, 6, 5, 6), None, False, (2, 3), 9, 10),
    ("cost64", (14, 6, 5, 6), None, True, (0, 1), 5, 11),
    ("tab64+f16", (8, 7, 6), (2, 3, 2), False, (2,), 2, 12),
]


def restatement_case(hjbdp, case):
    typing, n, m, nonuniform, axes, W, seed = REF_CASES[case]
    spec = _ref_spec(hjbdp, typing, n, m, nonuniform, seed)
    axes = tuple(range(spec.D)) if axes is None else axes
    return spec, axes, W, _table(spec, axes, W, seed), _terminal(spec, seed), (_weights(W, seed) if case % 2 else None)


def reference_conditions(spec, axes, W, off, term, w):
    """What the REFERENCE must show for a case to be worth running: {name: bool}."""
    ref = ControlDisturbedRef(spec, off, w, "expect")
    cov = ref.coverage()
    out = {"mask": ref.axes_mask == sum(1 << a for a in axes),
           "both ends": all((below and above) or spec.n[a] < 4 for a, (below, above, _) in cov.items()),
           "split": W == 1 or all(split for _, _, split in cov.values())}
    Jr = ref.backup(term)[0]
    out["decode"] = all(not _same(ControlDisturbedRef(spec, bad, w, "expect").backup(term)[0], Jr) for bad in _misread_tables(spec, off))
    return out


@pytest.mark.parametrize("case", range(len(REF_CASES)))
def test_backup_equals_the_restatement(env, case):
    hjbdp, _abi = env
    spec, axes, W, off, term, w = restatement_case(hjbdp, case)
    cond = reference_conditions(spec, axes, W, off, term, w)
    assert all(cond.values()), cond
    with hjbdp.Backup(spec) as bk:
        for mode, wm in (("expect", w), ("worst", None)):
            ref = ControlDisturbedRef(spec, off, wm, mode)
            bk.set_control_disturbance(off.reshape((spec.D, W) + spec.m, order="F") if case % 3 == 0 else off, wm, mode)
            assert bk.get_option("dist_axes") == ref.axes_mask and bk.get_option("dist_nodes") == W and bk.get_option("dist_ctrl") == 1
            J, idx = bk.backup_stage(term)
            Jr, ir = ref.backup(term)
            print("case %d %s: J differs at %d of %d states, labels at %d" % (case, mode, int(np.sum(_bits(J) != _bits(Jr))), spec.nS, int(np.sum(idx != ir))))
            assert _same(J, Jr), (mode, int(np.sum(_bits(J) != _bits(Jr))))
            assert _same(idx, ir), (mode, int(np.sum(idx != ir)))


# ---- 3. slices -----------------------------------------------------------------------------------------------------------------
def test_every_slice_is_that_labels_node_set(env):
    hjbdp, _abi = env
    from problems import random_problem
    spec = random_problem(131, (6, 5, 4), (3, 2), dtype=np.float32, nonuniform=True, index_base=1)
    W = 5
    off = _table(spec, (0, 1, 2), W, 132)
    term = _terminal(spec, 133)
    w = _weights(W, 134)
    with hjbdp.Backup(spec) as bk:
        for mode, wm in (("expect", w), ("worst", None)):
            bk.set_control_disturbance(off, wm, mode)
            got = [bk.evaluate_stage(term, np.full(spec.nS, l0 + 1, dtype=np.int32)) for l0 in range(spec.nU)]
            for l0 in range(spec.nU):
                bk.set_disturbance(off[:, :, l0], wm, mode)
                assert _same(got[l0], bk.evaluate_stage(term, np.full(spec.nS, l0 + 1, dtype=np.int32))), (mode, l0)


# ---- 4. analytic ---------------------------------------------------------------------------------------------------------------
def analytic_table():
    """Quarter-integer offsets [2, 3, 5] on both axes: the large controls (labels 0 and 4 of affine_problem's u) are the uncertain
    ones, u = 0 (label 2) is noise-free.  Weights 0.5, 0.25, 0.25: every product and sum of the contract is exact."""
    scale = np.array([8.0, 1.0, 0.0, 1.0, 8.0])                   # per control: enough at the ends to make the nominal argmin (label 0) lose
    node = np.array([[1.0, -0.5, 0.25], [-0.75, 0.5, 1.0]])       # per axis and node
    return node[:, :, None] * scale[None, None, :], np.array([0.5, 0.25, 0.25])


def analytic_expected(spec, slope, off, p, mode):
    """[nS, nU] in exact arithmetic: the nominal candidate plus a . sum_w p_w d_w(l) (expect) or max_w a . d_w(l) (worst)."""
    from test_disturbance_refs import affine_expected
    nominal = affine_expected(spec, slope, 0, "expect")
    ad = slope[0] * off[0] + slope[1] * off[1]                    # a . d_w(l): [W, nU]
    return nominal + ((p[:, None] * ad).sum(axis=0) if mode == "expect" else ad.max(axis=0))[None, :]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_affine_cost_to_go_gives_the_analytic_values(env, dtype):
    hjbdp, _abi = env
    from test_disturbance_refs import affine_problem
    spec, J_next, slope = affine_problem(dtype)
    off, p = analytic_table()
    with hjbdp.Backup(spec) as bk:
        for mode in ("expect", "worst"):
            bk.set_control_disturbance(off, p if mode == "expect" else None, mode)
            want = analytic_expected(spec, slope, off, p, mode)
            J, idx = bk.backup_stage(J_next)
            assert np.array_equal(J.astype(np.float64), want.min(axis=1)), mode
            assert np.array_equal(idx, np.argmin(want, axis=1) + spec.index_base), mode
            for u in range(spec.nU):
                got = bk.evaluate_stage(J_next.reshape(-1, order="F"), np.full(spec.nS, u + spec.index_base, dtype=spec.idx_np_dtype))
                assert np.array_equal(got.astype(np.float64), want[:, u]), (mode, u)
            # the noise depends on the control: the same nodes averaged over the controls choose another control somewhere
            avg = np.repeat(off.mean(axis=2, keepdims=True), spec.nU, axis=2)
            assert (np.argmin(analytic_expected(spec, slope, avg, p, mode), axis=1) != np.argmin(want, axis=1)).any(), mode


# ---- 5. fixed labels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typing", ["f32", "f64", "tab64+cost64"])
def test_fixed_labels_share_the_backups_candidates(env, typing):
    hjbdp, _abi = env
    n, m = ((14, 6, 5, 6), None) if "cost64" in typing else ((7, 6, 5), (3, 2))
    spec = _ref_spec(hjbdp, typing, n, m, True, 151)
    W = 5
    off = _table(spec, tuple(range(spec.D)), W, 152)
    term = _terminal(spec, 153)
    rng = np.random.default_rng(154)
    lab = rng.integers(spec.index_base, spec.index_base + spec.nU, spec.nS).astype(spec.idx_np_dtype)
    n_st = 3
    labs = np.asfortranarray(rng.integers(spec.index_base, spec.index_base + spec.nU, (spec.nS, n_st)).astype(spec.idx_np_dtype))
    with hjbdp.Backup(spec) as bk:
        for mode, w in (("expect", _weights(W, 155)), ("worst", None)):
            bk.set_control_disturbance(off, w, mode)
            J, idx = bk.backup_stage(term)
            assert _same(bk.evaluate_stage(term, idx), J), mode                    # its own labels: its J
            got = bk.evaluate_stage(term, lab)
            assert _same(got, ControlDisturbedRef(spec, off, w, mode).evaluate(term, lab)), mode
            assert (got >= J).all(), mode                                          # the same candidates: exact comparison
            # the sweep of per-stage labels is a host loop of stages (the stage with index k_s reads column k_s - 1)
            res = bk.evaluate(n_st, labs, terminal=term, keep_J=True)
            Jk = term
            for k_s in range(n_st, 0, -1):
                Jk = bk.evaluate_stage(Jk, labs[:, k_s - 1])
                assert _same(res["J_stages"][:, k_s - 1], Jk), (mode, k_s)
            assert _same(res["J"], Jk)


def test_a_label_out_of_range_through_both_entries(env):
    hjbdp, _abi = env
    from problems import random_problem
    spec = random_problem(156, (7, 11, 13), (3, 2), dtype=np.float32, index_base=1)
    nS, nU = spec.nS, spec.nU
    term = _terminal(spec, 157)
    lab = np.random.default_rng(158).integers(1, nU + 1, nS).astype(np.int32)
    bad = lab.copy()
    bad[700], bad[3] = nU + 1, 0                                # one past the table's last row, and one before its first
    with hjbdp.Backup(spec) as bk:
        bk.set_control_disturbance(_table(spec, (0, 1, 2), 5, 159), None, "worst")
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
                assert np.array_equal(np.flatnonzero(np.isnan(got)), [3, 700])  # NaN at those states only
                keep = ~np.isin(np.arange(nS), [3, 700])
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
@pytest.mark.parametrize("mode", ["expect", "worst"])
def test_solve_equals_a_host_loop_of_stages(env, mode):
    hjbdp, _abi = env
    spec = _local_2d(hjbdp)
    n_st = 2 * K_TILE + 1
    W = 5
    off = _table(spec, (0, 1), W, 161, cells=0.8)
    w = _weights(W, 162) if mode == "expect" else None
    with hjbdp.Backup(spec) as bk:
        bk.set_option("temporal", 2)
        nominal = bk.solve(n_st)                        # undisturbed, this problem takes the several-stages-per-launch path
        bk.set_option("temporal", 1)
        bk.set_control_disturbance(off, w, mode)
        outs = {}
        for graph in (0, 1):
            bk.set_option("graph", graph)
            outs[graph] = bk.solve(n_st, keep_J=True, keep_idx=True)
        out = outs[1]
        assert _same(outs[0]["J_stages"], out["J_stages"]) and _same(outs[0]["idx_stages"], out["idx_stages"])
        J = np.zeros(spec.nS, dtype=spec.j_dtype)
        for k_s in range(n_st, 0, -1):                  # the host loop: stage k_s in column k_s - 1
            J, idx = bk.backup_stage(J)
            assert _same(out["J_stages"][:, k_s - 1], J) and _same(out["idx_stages"][:, k_s - 1], idx), k_s
        assert _same(out["J"], J) and _same(out["idx"], idx)
        assert not _same(nominal["J"], J)
        for (Jr, ir), k_s in zip(ControlDisturbedRef(spec, off, w, mode).sweep(3), range(n_st, n_st - 3, -1)):
            assert _same(out["J_stages"][:, k_s - 1], Jr) and _same(out["idx_stages"][:, k_s - 1], ir), k_s
        # no per-stage outputs (what would have been tiled), ordinary launches and a captured, replayed stage loop
        long = 2 * 32 + 6
        for graph in (0, 1):
            bk.set_option("graph", graph)
            plain = bk.solve(n_st)
            assert _same(plain["J"], J) and _same(plain["idx"], idx) and plain["stages_done"] == n_st
            outs[graph] = bk.solve(long)
        assert _same(outs[0]["J"], outs[1]["J"]) and _same(outs[0]["idx"], outs[1]["idx"]) and outs[1]["stages_done"] == long
        # several stages per launch, when required, is refused; when merely allowed it was silently not taken (above)
        bk.set_option("temporal", 2)
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.solve(n_st)
        assert ei.value.status == _abi.HJB_E_UNSUPPORTED
        bk.set_option("temporal", 1)
        assert _same(bk.solve(n_st)["J"], J)


# ---- 7. forms and launches -----------------------------------------------------------------------------------------------------
def test_index_forms_and_launch_sizes_give_the_same_bits(env):
    hjbdp, _abi = env
    from problems import random_problem
    spec = random_problem(171, (7, 6, 7, 7), (3, 2), dtype=np.float32, nonuniform=True, index_base=1)
    assert spec.nS > 3 * 256
    off = _table(spec, (0, 1, 2, 3), 5, 172)
    term = _terminal(spec, 173)
    with hjbdp.Backup(spec) as bk:
        bk.set_control_disturbance(off, _weights(5, 174), "expect")
        assert bk.get_option("dist_form") == 1 and bk.get_option("dist_i32") == 1
        J, idx = bk.backup_stage(term)
        auto_grid = bk.get_option("grid")
        assert auto_grid == -(-spec.nS // 256)
        for i32 in (0, 1):
            bk.set_option("dist_i32", i32)
            assert bk.get_option("dist_form") == i32
            for grid in (1, 2, 3, auto_grid):
                for block in (256, 64):
                    bk.set_option("grid", grid)
                    bk.set_option("block", block)
                    bk.set_option("eval_grid", 0 if grid == auto_grid else grid)
                    assert bk.get_option("grid") == grid and bk.info()["block"] == block
                    J1, i1 = bk.backup_stage(term)
                    assert _same(J1, J) and _same(i1, idx), (i32, grid, block)
                    assert _same(bk.evaluate_stage(term, idx), J), (i32, grid, block)


# ---- 8. switching and refusals -------------------------------------------------------------------------------------------------
def test_switching_growing_and_refusals_leave_the_bits_as_they_were(env):
    hjbdp, _abi = env
    from problems import random_problem
    spec = random_problem(181, (6, 5, 4), (3, 2), dtype=np.float32, index_base=1)
    D, nU = spec.D, spec.nU
    term = _terminal(spec, 182)
    add = _offsets(spec, (0, 2), 3, 183)
    t2, t9, t3 = _table(spec, (0, 1), 2, 184), _table(spec, (0, 1, 2), 9, 185), _table(spec, (1,), 3, 186)
    w3 = np.array([0.2, 0.3, 0.5])
    dp = C.POINTER(C.c_double)
    E, W_ = _abi.HJB_DIST_EXPECT, _abi.HJB_DIST_WORST
    t3f = np.asfortranarray(t3)                                  # (kept alive: the calls below take its address)
    good = t3f.ctypes.data_as(dp)
    with hjbdp.Backup(spec) as bk:
        lib = bk.lib
        J0, i0 = bk.backup_stage(term)
        # K24 -> K32 -> K24; a table that grows (W 2 -> 9) and shrinks; each setting gives its own bits again
        want = {}
        for name, setit in (("add", lambda: bk.set_disturbance(add, w3, "expect")), ("t2", lambda: bk.set_control_disturbance(t2, None, "worst")),
                            ("t9", lambda: bk.set_control_disturbance(t9, _weights(9, 187), "expect")),
                            ("t3", lambda: bk.set_control_disturbance(t3, w3, "expect"))):
            setit()
            want[name] = bk.backup_stage(term)
            assert bk.info()["dist_ctrl"] == (name != "add")
        for name, ref in (("t2", ControlDisturbedRef(spec, t2, None, "worst")), ("t9", ControlDisturbedRef(spec, t9, _weights(9, 187), "expect")),
                          ("t3", ControlDisturbedRef(spec, t3, w3, "expect"))):
            Jr, ir = ref.backup(term)
            assert _same(want[name][0], Jr) and _same(want[name][1], ir), name
        bk.set_control_disturbance(t2, None, "worst")
        assert all(_same(a, b) for a, b in zip(bk.backup_stage(term), want["t2"]))
        bk.set_disturbance(add, w3, "expect")
        assert all(_same(a, b) for a, b in zip(bk.backup_stage(term), want["add"]))
        bk.clear_disturbance()
        assert all(_same(a, b) for a, b in zip(bk.backup_stage(term), (J0, i0)))
        # refusals, on the bare handle, under the additive setting and under a table: status, text, info and bits
        nan_t = t3f.copy(order="F")
        nan_t[1, 2, nU - 1] = np.nan
        keep = [nan_t, t3f, np.array([0.6, -0.1, 0.5]), np.zeros((D, 129, 1))]
        refused = [("n_controls", _abi.HJB_E_INVALID, (E, 3, nU - 1, good, None)), ("n_controls", _abi.HJB_E_INVALID, (E, 3, nU + 1, good, None)),
                   ("n_controls", _abi.HJB_E_INVALID, (E, 3, -1, good, None)),
                   ("not finite", _abi.HJB_E_INVALID, (E, 3, nU, keep[0].ctypes.data_as(dp), None)),
                   ("no weights", _abi.HJB_E_INVALID, (W_, 3, nU, good, w3.ctypes.data_as(dp))),
                   ("weight", _abi.HJB_E_INVALID, (E, 3, nU, good, keep[2].ctypes.data_as(dp))),
                   ("n_nodes", _abi.HJB_E_INVALID, (E, _abi.HJB_DIST_MAX_NODES + 1, nU, keep[3].ctypes.data_as(dp), None)),
                   ("null offsets", _abi.HJB_E_INVALID, (E, 3, nU, None, None)), ("mode", _abi.HJB_E_INVALID, (2, 3, nU, good, None))]
        assert lib.hjb_set_control_disturbance(None, E, 3, nU, good, None) == _abi.HJB_E_INVALID
        for state in ("bare", "add", "t3"):
            if state == "add":
                bk.set_disturbance(add, w3, "expect")
            elif state == "t3":
                bk.set_control_disturbance(t3, w3, "expect")
            Jb, ib = bk.backup_stage(term)
            inf0 = bk.info()
            for text, status, args in refused:
                assert lib.hjb_set_control_disturbance(bk._h, *args) == status, (state, text, args[:3])
                assert text.encode() in lib.hjb_last_error(bk._h), (text, lib.hjb_last_error(bk._h))
                assert bk.info() == inf0
                J1, i1 = bk.backup_stage(term)
                assert _same(J1, Jb) and _same(i1, ib), (state, text)
        # while a table is set: the read-only option, no other variant, no probe ("temporal" = 2: the sweep's test)
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.set_option("dist_ctrl", 0)
        assert ei.value.status == _abi.HJB_E_INVALID and "read-only" in str(ei.value)
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.set_option("variant", 5)
        assert ei.value.status == _abi.HJB_E_UNSUPPORTED and "variant 8 only" in str(ei.value)
        probe = {"lo": (0,) * D, "hi": (2,) * D, "control": (0, 0), "want": ("g",)}
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.solve(3, probe=probe)
        assert ei.value.status == _abi.HJB_E_UNSUPPORTED and "probe" in str(ei.value)
        J1, i1 = bk.backup_stage(term)
        assert _same(J1, want["t3"][0]) and _same(i1, want["t3"][1])
        bk.clear_disturbance()
        assert bk.solve(3, probe=probe)["probe"]["g"].shape == (2,) * D + (3,)
    # a table of more than 2^26 entries: refused by its size, before a byte of it is read
    big = random_problem(188, (3, 3, 3), (500, 400), dtype=np.float32)
    assert big.D * 128 * big.nU > _abi.HJB_CTRL_DIST_MAX_ENTRIES
    small = np.zeros(8)
    with hjbdp.Backup(big) as bk:
        inf0 = bk.info()
        assert bk.lib.hjb_set_control_disturbance(bk._h, W_, 128, big.nU, small.ctypes.data_as(dp), None) == _abi.HJB_E_UNSUPPORTED
        assert b"2^26" in bk.lib.hjb_last_error(bk._h) and bk.info() == inf0 and inf0["kernel_variant"] != 8
    # a slab handle and a handle with a state model take none
    with hjbdp.Backup(spec, slab=(1, 3, 1, 1)) as bk:
        inf0 = bk.info()
        assert bk.lib.hjb_set_control_disturbance(bk._h, E, 3, nU, good, None) == _abi.HJB_E_UNSUPPORTED
        assert b"slab" in bk.lib.hjb_last_error(bk._h) and bk.info() == inf0 and inf0["kernel_variant"] != 8
    sa = hjbdp.Solver_attitude(n_mesh_w=9, n_mesh_q=4)
    sa.U_vector = np.linspace(-0.11, 0.11, 5)
    mspec = sa.build_spec_model()
    moff = np.asfortranarray(np.full((6, 2, mspec.nU), 0.01))
    with hjbdp.Backup(mspec) as bk:
        assert bk.lib.hjb_set_control_disturbance(bk._h, W_, 2, mspec.nU, moff.ctypes.data_as(dp), None) == _abi.HJB_E_UNSUPPORTED
        assert b"model" in bk.lib.hjb_last_error(bk._h) and bk.info()["kernel_variant"] == 4 and bk.info()["dist_nodes"] == 0


def test_solve_batch_refuses_a_member_with_a_table_and_the_python_side_falls_back(env):
    hjbdp, _abi = env
    from problems import random_problem
    n_st = 5
    specs = [random_problem(185 + i, (9, 8, 7), (3,), dtype=np.float32, index_base=1) for i in range(2)]
    off = _table(specs[1], (0, 1), 3, 186)
    bks = [hjbdp.Backup(s) for s in specs]
    try:
        for bk in bks:
            bk.set_option("variant", 5)                  # the table kernel's 32-bit form: a group hjb_solve_batch takes
        keep, optp, resp = [], (C.POINTER(_abi.hjb_solve_opts) * 2)(), (C.POINTER(_abi.hjb_result) * 2)()
        for k, s in enumerate(specs):
            o, r = _abi.hjb_solve_opts(), _abi.hjb_result()
            o.n_stages = n_st
            J, idx = np.empty(s.nS, dtype=s.j_dtype), np.empty(s.nS, dtype=s.idx_np_dtype)
            o.J_final, o.idx_final = J.ctypes.data, idx.ctypes.data
            keep += [o, r, J, idx]
            optp[k], resp[k] = C.pointer(o), C.pointer(r)
        hs = (C.c_void_p * 2)(*[bk._h for bk in bks])
        lib = bks[0].lib
        assert lib.hjb_solve_batch(2, hs, optp, resp) == _abi.HJB_OK
        plain = bks[1].solve(n_st)
        bks[1].set_control_disturbance(off, None, "worst")
        assert lib.hjb_solve_batch(2, hs, optp, resp) == _abi.HJB_E_UNSUPPORTED
        assert b"disturbance" in lib.hjb_last_error(bks[1]._h)
        want = [bks[0].solve(n_st), bks[1].solve(n_st)]
    finally:
        for bk in bks:
            bk.close()
    dspecs = [specs[0], _retype(hjbdp, specs[1], control_disturbance=(off, None, "worst"))]
    got, _, variants, sizes = hjbdp.solve_batch(dspecs, n_st)
    assert variants[1] == 8 and sizes == [1, 1]
    assert all(_same(g["J"], w["J"]) and _same(g["idx"], w["idx"]) for g, w in zip(got, want))
    assert not _same(want[1]["J"], plain["J"])


# ---- 9. the mirror -------------------------------------------------------------------------------------------------------------
def test_dynamic_solver_designs_and_prices_under_actuator_noise(env):
    hjbdp, _abi = env

    def solver(noise):
        ds = hjbdp.Dynamic_Solver(precision="double")
        ds.N, ds.dx, ds.du = 6, 35, 100
        ds.actuator_noise = noise
        return ds
    nominal = solver(None).run()
    zero = solver(([0.0], None, "expect")).run()
    assert np.array_equal(zero.J_star, nominal.J_star) and np.array_equal(zero.u_star_idxs, nominal.u_star_idxs)
    eps, w = [-0.2, 0.0, 0.2], [0.25, 0.5, 0.25]
    ds = solver((eps, w, "expect")).run()
    assert not np.array_equal(ds.J_star, nominal.J_star)
    # by hand: the table from the solver's own B and control mesh, on the spec the solver builds without it
    bare = solver(None).build_spec()
    U = np.asarray(ds._U_mesh, dtype=np.float64)
    off = np.stack([np.outer(np.asarray(eps), ds.B[a, 0] * U) for a in range(2)])            # [2, W, nU]: B U_mesh[l] eps[w]
    hand = _retype(hjbdp, bare, control_disturbance=(off, w, "expect"))
    with hjbdp.Backup(hand) as bk:
        out = bk.solve(ds.N - 1, keep_J=True, keep_idx=True)
    assert np.array_equal(out["J_stages"].reshape((35, 35, 5), order="F"), ds.J_star[:, :, :5])
    assert np.array_equal(out["idx_stages"].reshape((35, 35, 5), order="F"), ds.u_star_idxs)
    pc = ds.policy_cost()
    assert pc.shape == (35, 35, 5) and np.array_equal(pc, ds.J_star[:, :, :5])
    assert np.array_equal(nominal.policy_cost(), nominal.J_star[:, :, :5])
    for fly in (lambda: ds.get_noisy_paths(np.array([[2.0], [1.0]]), 4), lambda: ds.get_lookahead_paths(np.array([[2.0], [1.0]])),
                lambda: ds.get_noisy_cost_statistics(np.array([[2.0], [1.0]]), 4)):
        with pytest.raises(RuntimeError, match="control-dependent noise"):
            fly()
    X, _ = ds.get_optimal_paths(np.array([[2.0], [1.0]]))        # the nominal flight of the stored policy needs no node set
    assert X.shape == (2, 6, 1)


# ---- 10. budget ----------------------------------------------------------------------------------------------------------------
def test_no_scratch_and_no_lds_in_the_built_kernels(built, tmp_path):
    """Read from the code objects inside the built library (llvm-objdump --offloading, llvm-readelf --notes): every
    k_backup_ctrldist instantiation - 5 typings x D 1..6 x 2 index forms x 2 label forms - without LDS; none at D <= 4 with scratch."""
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
            m = re.search(r"\.name:\s+(\S*k_backup_ctrldist\S*)", blk)
            if m:
                found[m.group(1)] = (int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)),
                                     int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    assert len(found) == 5 * 6 * 2 * 2, len(found)
    for name, (lds, scratch) in found.items():
        D = int(re.search(r"Li(\d)E", name).group(1))
        assert lds == 0, (name, lds)
        assert scratch == 0 or D > 4, (name, scratch)
