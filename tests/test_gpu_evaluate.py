"""GPU tests (-m gpu) of the fixed-label stage and its sweep (hjb_evaluate_stage, hjb_evaluate_stage_device, hjb_evaluate;
csrc/kernels_evaluate.h): J(x) = g(x, u(x)) + F(x_next(x, u(x))) for GIVEN labels.

Bars, all bit for bit: on the backup's own labels the backup's J, under every typing, label width, stage-kernel variant and
source of cells and weights; on arbitrary labels tests/evaluate_refs.py::evaluate_ref in its canonical (fma) form, which
tests/test_evaluate_abi.py holds to the C twin, and - for the float64-typed tables and costs no host reference restates - the
library's own backups of the problem restricted to one control.  The shapes are the smallest at which the thing tested can go
wrong; none is a workload size."""
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


def _retype(hjbdp, spec, j_storage=None, idx_dtype=None, index_base=None):
    return hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, dtype=spec.dtype,
                             index_base=spec.index_base if index_base is None else index_base, j_storage=j_storage,
                             idx_dtype=spec.idx_dtype if idx_dtype is None else idx_dtype, table_dtype=spec.table_dtype,
                             cost_dtype=spec.cost_dtype)


def _terminal(spec, seed):
    """A random terminal cost in the J storage type (binary16 values for HJB_F16S)."""
    rng = np.random.default_rng(seed)
    return rng.random(spec.nS).astype(spec.j_dtype)


def _sources(hjbdp, _abi, bk):
    """The sources of cells and weights this handle can evaluate from: option eval_tables 0 (terms) and / or 1 (tables)."""
    out = []
    for s in (0, 1):
        try:
            bk.set_option("eval_tables", s)
            out.append(s)
        except hjbdp.HjbError as e:
            assert e.status == _abi.HJB_E_UNSUPPORTED
    bk.set_option("eval_tables", -1)
    assert out
    return out


# one shape per D; unequal control sizes (a transposed label decode gathers another control's value)
SHAPES = [((7,), (5,)), ((6, 5), (3, 4)), ((5, 4, 6), (3, 4, 2)), ((5, 4, 3, 4), (4,)), ((4, 3, 4, 3, 3), (2, 3)),
          ((3, 3, 3, 3, 3, 4), (3, 2, 2))]
IDX = [(np.int32, 0), (np.uint8, 1), (np.uint16, 0), (np.int32, 1), (np.uint8, 0), (np.uint16, 1)]


# the kernel's index forms: 32-bit with 24-bit products (what these sizes run by default), 32-bit with 32-bit products, 64-bit
FORMS = [(1, 1), (1, 0), (0, 1)]
EVAL_FORM = {(1, 1): 2, (1, 0): 1, (0, 1): 0}        # get_option("eval_form"): the form the next launch runs


def _own_labels_case(env, spec, variants=(None, 0, 5), seed=3):
    """evaluate_stage(J_next, backup_stage(J_next).idx) == backup_stage(J_next).J for every variant that serves and every source."""
    hjbdp, _abi, _ = env
    term = _terminal(spec, seed)
    ran, srcs_seen = [], set()
    for v in variants:
        try:
            bk = hjbdp.Backup(spec, variant=v)
        except hjbdp.HjbError as e:
            assert v is not None and e.status == _abi.HJB_E_UNSUPPORTED, (v, e)
            continue
        with bk:
            J, idx = bk.backup_stage(term)
            assert idx.dtype == spec.idx_np_dtype and J.dtype == spec.j_dtype
            for s in _sources(hjbdp, _abi, bk):
                bk.set_option("eval_tables", s)
                for i32, m24 in FORMS:
                    bk.set_option("eval_i32", i32)
                    bk.set_option("eval_m24", m24)
                    assert bk.get_option("eval_i32") == i32 and bk.get_option("eval_m24") == m24
                    assert bk.get_option("eval_form") == EVAL_FORM[(i32, m24)], (v, s, i32, m24)
                    got = bk.evaluate_stage(term, idx)
                    assert got.dtype == J.dtype
                    assert np.array_equal(got, J), (v, s, i32, m24, int(np.sum(got != J)))
                srcs_seen.add(s)
            ran.append(bk.info()["kernel_variant"])
    assert ran
    return ran, srcs_seen


@pytest.mark.parametrize("storage", ["f32", "f64", "f16"])
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_own_labels_give_the_backups_J(env, case, storage):
    hjbdp, _abi, _ = env
    from problems import random_problem
    n, m = SHAPES[case]
    dtype = np.float64 if storage == "f64" else np.float32
    for nonuniform in (False, True):
        idx_dtype, base = IDX[(case + (3 if nonuniform else 0) + {"f32": 0, "f64": 1, "f16": 2}[storage]) % len(IDX)]
        spec = random_problem(500 + 10 * case + nonuniform, n, m, dtype=dtype, nonuniform=nonuniform, index_base=base)
        spec = _retype(hjbdp, spec, j_storage=np.float16 if storage == "f16" else None, idx_dtype=idx_dtype)
        ran, srcs = _own_labels_case(env, spec)
        assert 0 in ran and srcs == {0, 1}, (ran, srcs)        # the generic kernel serves every one of these; both sources exist


def test_own_labels_pos_att_typing_and_colsweep_shape(env):
    """The reference's pos-att typing (float64-built tables, float64-summed cost, uint8 labels: evaluated from the tables only)
    and the column-sweep kernel's shape at its smallest size (variant 7 writes the labels)."""
    hjbdp, _abi, _ = env
    from problems import colsweep_problem, pos_att_channel_spec
    spec = pos_att_channel_spec("f64", n=12)
    ran, srcs = _own_labels_case(env, spec)
    assert srcs == {1} and 5 in ran, (ran, srcs)
    spec = pos_att_channel_spec("terms", n=12)                   # float64 tables, float32 cost terms
    ran, srcs = _own_labels_case(env, spec)
    assert srcs == {1}, (ran, srcs)
    for cs in (colsweep_problem(1, (70, 9, 8, 11), nU=9, gax=3, cost="fast"),
               colsweep_problem(3, (70, 9, 8, 11), nU=9, gax=3, cost="multi"),
               colsweep_problem(1, (70, 9, 8, 11), nU=9, gax=3, cost="fast", j_storage=np.float16)):
        ran, srcs = _own_labels_case(env, cs, variants=(None, 0, 5, 7))
        assert 7 in ran and srcs == {0, 1}, (ran, srcs)


RANDOM_CASES = [("f32", (7, 11, 13), (3, 2), True), ("f64", (7, 11, 13), (2, 3), False), ("f16", (9, 7, 6), (4,), False),
                ("f64", (301,), (5,), True), ("f32", (5, 4, 3, 4), (3, 4, 2), False), ("f32", (3, 3, 3, 3, 3, 4), (2, 3, 2), True)]


@pytest.mark.parametrize("storage,n,m,nonuniform", RANDOM_CASES)
def test_random_labels_equal_the_reference(env, storage, n, m, nonuniform):
    """Seeded random labels, every source, the automatic launch and one smaller than the work (7 * 11 * 13 = 1001 states: four
    workgroups, the last one partly filled; eval_grid 2 makes every workgroup stride), in both index forms of the kernel."""
    hjbdp, _abi, _ = env
    from evaluate_refs import evaluate_ref, oracle_problem
    from problems import random_problem
    dtype = np.float64 if storage == "f64" else np.float32
    spec = random_problem(900 + len(n), n, m, dtype=dtype, nonuniform=nonuniform, index_base=1)
    spec = _retype(hjbdp, spec, j_storage=np.float16 if storage == "f16" else None, idx_dtype="auto")
    rng = np.random.default_rng(77)
    term = _terminal(spec, 9)
    lab0 = rng.integers(0, spec.nU, spec.nS)
    ref = evaluate_ref(oracle_problem(spec), term.astype(dtype), lab0, lerp="fma").reshape(-1, order="F").astype(spec.j_dtype)
    labels = (lab0 + 1).astype(spec.idx_np_dtype)
    with hjbdp.Backup(spec) as bk:
        for s in _sources(hjbdp, _abi, bk):
            bk.set_option("eval_tables", s)
            for grid, (i32, m24) in [(g, f) for f in FORMS for g in (0, 2)] + [(1, FORMS[0])]:     # launch size x index form
                bk.set_option("eval_grid", grid)
                bk.set_option("eval_i32", i32)
                bk.set_option("eval_m24", m24)
                assert bk.get_option("eval_grid") == grid and bk.get_option("eval_i32") == i32
                assert bk.get_option("eval_form") == EVAL_FORM[(i32, m24)], (s, grid, i32, m24)
                got = bk.evaluate_stage(term, labels)
                assert np.array_equal(got, ref), (s, grid, i32, m24, int(np.sum(got != ref)))
        bk.set_option("eval_grid", 0)
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.set_option("eval_grid", -1)
        assert ei.value.status == _abi.HJB_E_INVALID


def _restrict_to_control(hjbdp, spec, u):
    """The problem with its one control dim sliced to control u alone (size 1): its backup IS that control's candidate value."""
    assert spec.C == 1
    D = spec.D

    def cut(t):
        if D not in t.dims:
            return hjbdp.Term(t.dims, t.data)
        ax = t.dims.index(D)
        return hjbdp.Term(t.dims, np.take(t.data, [u], axis=ax))
    return hjbdp.ProblemSpec(spec.knots, [1], [[cut(t) for t in ts] for ts in spec.next_terms], [cut(t) for t in spec.cost_terms],
                             dtype=spec.dtype, index_base=spec.index_base, j_storage=None if spec.j_dtype == spec.dtype else spec.j_dtype,
                             idx_dtype=spec.idx_dtype, table_dtype=spec.table_dtype, cost_dtype=spec.cost_dtype)


def test_float64_typed_labels_against_single_control_backups(env):
    """HJB_TAB_F64 / HJB_COST_F64: the per-control reference is the library's own trusted backup of the problem restricted to
    that one control - nine small handles for nU = 9.  Constant labels equal that handle's J; random labels the per-state
    selection among the nine planes."""
    hjbdp, _abi, _ = env
    from problems import pos_att_channel_spec
    spec = pos_att_channel_spec("f64", n=12)
    assert spec.nU == 9 and spec.table_dtype == np.float64 and spec.cost_dtype == np.float64
    term = _terminal(spec, 21)
    planes = []
    for u in range(spec.nU):
        with hjbdp.Backup(_restrict_to_control(hjbdp, spec, u)) as b1:
            inf = b1.info()
            assert inf["table_dtype"] == _abi.HJB_TAB_F64 and inf["cost_dtype"] == _abi.HJB_COST_F64
            planes.append(b1.backup_stage(term)[0])
    planes = np.stack(planes, axis=1)                                   # [nS, nU]
    assert len({planes[:, u].tobytes() for u in range(spec.nU)}) == spec.nU
    rng = np.random.default_rng(5)
    lab0 = rng.integers(0, spec.nU, spec.nS)
    with hjbdp.Backup(spec) as bk:
        for u in range(spec.nU):
            got = bk.evaluate_stage(term, np.full(spec.nS, u + 1, dtype=spec.idx_np_dtype))
            assert np.array_equal(got, planes[:, u]), u
        got = bk.evaluate_stage(term, (lab0 + 1).astype(spec.idx_np_dtype))
        assert np.array_equal(got, planes[np.arange(spec.nS), lab0])
        with pytest.raises(hjbdp.HjbError) as ei:                       # its float32 terms are copies for the host's analysis
            bk.set_option("eval_tables", 0)
        assert ei.value.status == _abi.HJB_E_UNSUPPORTED


def _sweep_specs(hjbdp):
    from problems import random_problem
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N, ds.dx, ds.du = 9, 21, 40                                      # the Kirk fixture's problem at a reduced size
    return [ds.build_spec(), random_problem(61, (9, 7, 6), (3, 2), dtype=np.float32, index_base=1)]


@pytest.mark.parametrize("which", [0, 1])
def test_sweep_with_per_stage_labels_reproduces_the_solve(env, which):
    hjbdp, _abi, _ = env
    spec = _sweep_specs(hjbdp)[which]
    term = _terminal(spec, 31)
    with hjbdp.Backup(spec) as bk:
        out = bk.solve(8, terminal=term, keep_J=True, keep_idx=True)
        ev = bk.evaluate(8, out["idx_stages"], terminal=term, keep_J=True)
        assert ev["sweep_ms"] > 0
        for k in range(8):
            assert np.array_equal(ev["J_stages"][:, k], out["J_stages"][:, k]), k
        assert np.array_equal(ev["J"], out["J"])
        ev2 = bk.evaluate(8, out["idx_stages"], terminal=term)            # ping-pong buffers instead of stage planes
        assert ev2["J_stages"] is None and np.array_equal(ev2["J"], out["J"])


@pytest.mark.parametrize("which", [0, 1])
def test_sweep_with_stationary_labels_equals_a_host_loop(env, which):
    hjbdp, _abi, _ = env
    spec = _sweep_specs(hjbdp)[which]
    term = _terminal(spec, 32)
    with hjbdp.Backup(spec) as bk:
        J1, idx = bk.backup_stage(term)
        one = bk.evaluate(1, idx, terminal=term, keep_J=True)
        assert np.array_equal(one["J"], J1) and np.array_equal(one["J_stages"][:, 0], J1)
        ev = bk.evaluate(8, idx, terminal=term, keep_J=True)
        J = term
        for k_s in range(8, 0, -1):
            J = bk.evaluate_stage(J, idx)
            assert np.array_equal(ev["J_stages"][:, k_s - 1], J), k_s
        assert np.array_equal(ev["J"], J)
        zero = bk.evaluate(3, idx)                                      # terminal None = zeros
        assert np.array_equal(zero["J"], bk.evaluate(3, idx, terminal=np.zeros(spec.nS))["J"])


def test_slab_with_halo_evaluates_to_the_whole_grid_result(env):
    hjbdp, _abi, _ = env
    from problems import random_problem
    spec = random_problem(99, (9, 8, 12), (4, 3), dtype=np.float32, spread=0.08)
    term = _terminal(spec, 3)
    rng = np.random.default_rng(8)
    labels = rng.integers(0, spec.nU, spec.nS).astype(spec.idx_np_dtype)
    with hjbdp.Backup(spec) as bk:
        Jw = bk.evaluate_stage(term, labels)
        need = bk.info()
    inner = 9 * 8
    Jw3, L3, T3 = (x.reshape(inner, 12, order="F") for x in (Jw, labels, term))
    hl, hh = need["halo_needed_lo"], need["halo_needed_hi"]
    assert hl + hh < 12
    for (b, e) in [(0, 5), (5, 9), (9, 12)]:
        lo, hi = min(hl, b), min(hh, 12 - e)
        with hjbdp.Backup(spec, slab=(b, e, lo, hi)) as bk:
            Jin = np.asfortranarray(T3[:, b - lo:e + hi]).reshape(-1, order="F")
            lab = np.asfortranarray(L3[:, b:e]).reshape(-1, order="F")
            for s in _sources(hjbdp, _abi, bk):
                bk.set_option("eval_tables", s)
                Jo = bk.evaluate_stage(Jin, lab).reshape(inner, e + hi - b + lo, order="F")
                assert np.array_equal(Jo[:, lo:lo + e - b], Jw3[:, b:e]), (b, e, s)
                assert np.array_equal(Jo[:, :lo], T3[:, b - lo:b]) and np.array_equal(Jo[:, lo + e - b:], T3[:, e:e + hi])


def test_too_small_halo_is_reported_as_a_left_slab(env):
    """The existing status word: the kernel clamps the cell and raises it, check_device_status reports HJB_E_HALO."""
    hjbdp, _abi, _ = env
    from problems import random_problem
    spec = random_problem(5, (6, 5, 16), (3,), dtype=np.float32, spread=0.6)
    term = _terminal(spec, 1)
    Jin = term.reshape(30, 16, order="F")[:, 6:10].reshape(-1, order="F")
    with hjbdp.Backup(spec, slab=(6, 10, 0, 0)) as bk:
        idx = np.zeros(30 * 4, dtype=spec.idx_np_dtype)                    # (index_base 0: control 0 everywhere)
        for s in _sources(hjbdp, _abi, bk):
            bk.set_option("eval_tables", s)
            with pytest.raises(hjbdp.HjbError) as ei:
                bk.evaluate_stage(Jin, idx)
            assert ei.value.status == _abi.HJB_E_HALO, s
            bk.check_device_status()                                     # reported once: cleared
        with hjbdp.DeviceBuffer(Jin.nbytes) as dIn, hjbdp.DeviceBuffer(Jin.nbytes) as dOut, hjbdp.DeviceBuffer(idx.nbytes) as dL:
            dIn.upload(Jin)
            dL.upload(idx)
            bk.evaluate_stage_device(dIn, dL, dOut)
            with pytest.raises(hjbdp.HjbError) as ei:
                bk.check_device_status()
            assert ei.value.status == _abi.HJB_E_HALO
            bk.check_device_status()
            assert np.isfinite(dOut.download(spec.j_dtype)).all()        # clamped, not out of bounds


def _raw_stage(bk, Jn, labels, Jo):
    return bk.lib.hjb_evaluate_stage(bk._h, Jn.ctypes.data, labels.ctypes.data, Jo.ctypes.data)


@pytest.mark.parametrize("idx_dtype,base", [(np.int32, 1), (np.uint8, 0), (np.uint16, 1)])
def test_host_entries_refuse_bad_labels_and_touch_nothing(env, idx_dtype, base):
    hjbdp, _abi, _ = env
    from problems import random_problem
    spec = _retype(hjbdp, random_problem(71, (6, 5, 4), (3, 2), dtype=np.float32, index_base=base), idx_dtype=idx_dtype)
    nS, nU = spec.nS, spec.nU
    term = _terminal(spec, 2)
    good = np.full(nS, base, dtype=idx_dtype)
    sentinel = np.float32(-777.25)
    bads = [(nS - 1, base + nU)]                                         # one past the largest label, at the last state
    if base == 1 or idx_dtype == np.int32:
        bads.append((nS // 2, base - 1))                                 # one below index_base (0 for base 1, -1 for int32 base 0)
    with hjbdp.Backup(spec) as bk:
        for where, value in bads:
            lab = good.copy()
            lab[where] = value
            Jo = np.full(nS, sentinel, dtype=np.float32)
            assert _raw_stage(bk, term, lab, Jo) == _abi.HJB_E_INVALID
            assert b"label" in bk.lib.hjb_last_error(bk._h) and (Jo == sentinel).all()
            with pytest.raises(hjbdp.HjbError) as ei:
                bk.evaluate(3, lab, terminal=term)
            assert ei.value.status == _abi.HJB_E_INVALID
        # a bad label only in the last plane of a per-stage array
        lab = np.full((nS, 4), base, dtype=idx_dtype, order="F")
        lab[nS - 1, 3] = base + nU
        Jf = np.full(nS, sentinel, dtype=np.float32)
        Js = np.full(nS * 4, sentinel, dtype=np.float32)
        ms = C.c_double(-1.0)
        st = bk.lib.hjb_evaluate(bk._h, 4, term.ctypes.data, lab.ctypes.data, 1, Jf.ctypes.data, Js.ctypes.data, C.byref(ms))
        assert st == _abi.HJB_E_INVALID and (Jf == sentinel).all() and (Js == sentinel).all() and ms.value == -1.0
        assert b"plane 3" in bk.lib.hjb_last_error(bk._h)
        # the other refusals of a live handle, before any device work
        p = term.ctypes.data
        assert bk.lib.hjb_evaluate(bk._h, 0, p, good.ctypes.data, 0, Jf.ctypes.data, None, None) == _abi.HJB_E_INVALID
        assert bk.lib.hjb_evaluate(bk._h, 3, p, good.ctypes.data, 2, Jf.ctypes.data, None, None) == _abi.HJB_E_INVALID
        assert bk.lib.hjb_evaluate(bk._h, 3, p, None, 0, Jf.ctypes.data, None, None) == _abi.HJB_E_INVALID
        for args in [(None, good.ctypes.data, Jf.ctypes.data), (p, None, Jf.ctypes.data), (p, good.ctypes.data, None)]:
            assert bk.lib.hjb_evaluate_stage(bk._h, *args) == _abi.HJB_E_INVALID
            assert bk.lib.hjb_evaluate_stage_device(bk._h, *args, None) == _abi.HJB_E_INVALID
        assert (Jf == sentinel).all()
        # ... and the handle still works
        assert np.isfinite(bk.evaluate_stage(term, good)).all()


def test_device_entry_marks_bad_labels_with_nan_and_reports_once(env):
    hjbdp, _abi, _ = env
    from problems import random_problem
    spec = random_problem(72, (7, 11, 13), (3, 2), dtype=np.float32, index_base=1)
    nS, nU = spec.nS, spec.nU
    term = _terminal(spec, 4)
    rng = np.random.default_rng(6)
    lab = rng.integers(1, nU + 1, nS).astype(np.int32)
    bad_at = np.array([0, 63, 64, 255, 256, 700, nS - 1])
    bad = lab.copy()
    bad[bad_at] = [0, nU + 1, -5, 2 ** 31 - 1, -2 ** 31, nU + 1, 0]
    with hjbdp.Backup(spec) as bk:
        want = bk.evaluate_stage(term, lab)
        for s, (i32, m24) in [(s, f) for s in _sources(hjbdp, _abi, bk) for f in FORMS]:
            bk.set_option("eval_tables", s)
            bk.set_option("eval_i32", i32)
            bk.set_option("eval_m24", m24)
            with hjbdp.DeviceBuffer(term.nbytes) as dIn, hjbdp.DeviceBuffer(term.nbytes) as dOut, hjbdp.DeviceBuffer(bad.nbytes) as dL:
                dIn.upload(term)
                dL.upload(bad)
                dOut.upload(np.zeros(nS, dtype=np.float32))
                bk.evaluate_stage_device(dIn, dL, dOut)
                with pytest.raises(hjbdp.HjbError) as ei:
                    bk.check_device_status()
                assert ei.value.status == _abi.HJB_E_INVALID and "label" in str(ei.value)
                bk.check_device_status()                                 # once: HJB_OK afterwards
                got = dOut.download(np.float32)
                assert np.array_equal(np.flatnonzero(np.isnan(got)), np.sort(bad_at))
                keep = np.ones(nS, dtype=bool)
                keep[bad_at] = False
                assert np.array_equal(got[keep], want[keep])
                dL.upload(lab)                                           # good labels: no flag, the full result
                bk.evaluate_stage_device(dIn, dL, dOut)
                bk.check_device_status()
                assert np.array_equal(dOut.download(np.float32), want)


def test_device_entry_on_a_stream_equals_the_host_entry_and_a_model_is_refused(env):
    hjbdp, _abi, _ = env
    from problems import random_problem
    from test_gpu_streams import _Hip
    spec = _retype(hjbdp, random_problem(73, (5, 4, 3, 4), (3, 4), dtype=np.float32, nonuniform=True, index_base=1), idx_dtype=np.uint8)
    term = _terminal(spec, 5)
    with hjbdp.Backup(spec) as bk:
        J, idx = bk.backup_stage(term)
        want = bk.evaluate_stage(term, idx)
        hip = _Hip()
        s = hip.stream()
        try:
            with hjbdp.DeviceBuffer(term.nbytes) as dIn, hjbdp.DeviceBuffer(term.nbytes) as dOut, hjbdp.DeviceBuffer(idx.nbytes) as dL:
                dIn.upload(term)
                dL.upload(idx)
                bk.evaluate_stage_device(dIn, dL, dOut, stream=s)
                bk.check_device_status(stream=s)
                got = dOut.download(np.float32)
                with pytest.raises(hjbdp.HjbError) as ei:                # in place is refused, as for the backup
                    bk.evaluate_stage_device(dIn, dL, dIn, stream=s)
                assert ei.value.status == _abi.HJB_E_INVALID
        finally:
            hip.destroy(s)
        assert np.array_equal(got, want) and np.array_equal(got, J)
    sa = hjbdp.Solver_attitude(n_mesh_w=9, n_mesh_q=4)
    sa.U_vector = np.linspace(-0.11, 0.11, 5)
    mspec = sa.build_spec_model()
    with hjbdp.Backup(mspec) as bk:
        labels = np.ones(mspec.nS, dtype=mspec.idx_np_dtype)
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.evaluate_stage(np.zeros(mspec.nS, dtype=mspec.j_dtype), labels)
        assert ei.value.status == _abi.HJB_E_UNSUPPORTED and "model" in str(ei.value)
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.evaluate(2, labels)
        assert ei.value.status == _abi.HJB_E_UNSUPPORTED
        with hjbdp.DeviceBuffer(mspec.nS * 4) as dIn, hjbdp.DeviceBuffer(mspec.nS * 4) as dOut, hjbdp.DeviceBuffer(labels.nbytes) as dL:
            with pytest.raises(hjbdp.HjbError) as ei:
                bk.evaluate_stage_device(dIn, dL, dOut)
            assert ei.value.status == _abi.HJB_E_UNSUPPORTED


def test_dynamic_solver_policy_cost_is_the_runs_J(env):
    hjbdp, _abi, _ = env
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N, ds.dx, ds.du = 9, 21, 40
    ds.run()
    pc = ds.policy_cost()
    assert pc.shape == (21, 21, 8) and pc.dtype == ds.J_star.dtype
    assert np.array_equal(pc, ds.J_star[:, :, :8])
    ds.u_star_idxs = np.repeat(ds.u_star_idxs[:, :, 7:], 8, axis=2)      # another policy: the first stage's labels at every stage
    stat = ds.policy_cost()
    assert np.array_equal(stat[:, :, 7], ds.J_star[:, :, 7]) and not np.array_equal(stat[:, :, 0], ds.J_star[:, :, 0])


def _channel_checks(hjbdp, solver, run, cost, build):
    K = 6
    run(n_stages=K, keep_policy=True)
    pcs = cost(n_stages=K)
    assert len(pcs) == 3
    for ch in range(3):
        spec = build(ch)[0]
        lab = np.asarray(solver.U_idx[ch]).reshape(-1, order="F").astype(spec.idx_np_dtype)
        with hjbdp.Backup(spec) as bk:
            direct = bk.evaluate(K, lab)["J"]
        assert pcs[ch].shape == spec.n and np.array_equal(pcs[ch].reshape(-1, order="F"), direct), ch
    per_stage = cost(stationary=False)                                   # the kept per-stage labels reproduce F_values
    for ch in range(3):
        assert np.array_equal(per_stage[ch], solver.F_values[ch]), ch
    with pytest.raises(ValueError):
        cost(n_stages=K + 1, stationary=False)
    run(n_stages=1)
    one = cost(n_stages=1)
    for ch in range(3):
        assert np.array_equal(one[ch], solver.F_values[ch]), ch
    with pytest.raises(RuntimeError):
        cost(stationary=False)                                           # this run kept no per-stage policy


def test_solver_position_policy_cost(env):
    hjbdp, _abi, _ = env
    sp = hjbdp.Solver_position()
    sp.n_mesh_x = sp.n_mesh_v = 21
    with pytest.raises(RuntimeError):
        sp.policy_cost(n_stages=2)
    # (sym_linspace grows the mesh on every build: the spec is rebuilt on the grid vectors the run left)
    _channel_checks(hjbdp, sp, sp.simplified_run, sp.policy_cost, lambda ch: sp.build_spec(ch, grid=sp.U1_Opt.GridVectors))


def test_solver_attitude_policy_cost_simplified(env):
    hjbdp, _abi, _ = env
    sa = hjbdp.Solver_attitude()
    sa.n_mesh_w_simplified = sa.n_mesh_t = 21
    with pytest.raises(RuntimeError):
        sa.policy_cost_simplified(n_stages=2)
    _channel_checks(hjbdp, sa, sa.simplified_run, sa.policy_cost_simplified, sa.build_spec_simplified)
