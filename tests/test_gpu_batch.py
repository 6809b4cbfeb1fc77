"""GPU tests (-m gpu) of hjb_solve_batch (csrc/hjbdp_batch.hip): several sweeps of one kernel shape, one launch per stage.

It launches two kernels nothing else launches - k_backup_tabled32_batch<T, TJ, D> (3 storage types x D = 1..4) and
k_backup_colsweep_batch<float, float, GAX, NG, true, true, C64> (2 group axes x NG = 1..6 x 2 cost typings) - and the column
sweep's NG is the LARGEST group count of the batch: a member whose own plan has fewer groups runs under array extents, pipeline
halves and wait counts its own hjb_solve never uses.  Here every instantiation is launched (sections 1 and 3, closed by section 6)
and the host loop is walked at its edges (sections 2 and 4), all through ctypes on handles made with hjbdp.Backup, so that a
refusal fails the test instead of falling back to threads, and terminal, monitor_tol, monitor_single, progress and null outputs
are per problem.

The bar, everywhere: J (float16 by bits), labels, stages_done, stopped_early, last_e and last_e2 of every member equal, with no
tolerance, BOTH oracle/c_oracle.sweep of the same spec AND the same handle's own hjb_solve run before and again after the batch.

Column-sweep plans.  problems.colsweep_problem(3000 + 10 * levels + nU + n[0], n, nU=nU, gax=g, big=big, levels=levels,
cost="fast") with n = (45, 9, 8, 8), (60, 8, 7, 8), (61, 7, 8, 8) or (120, 6, 6, 6); option "cs_groups" as read on an MI355X
(the same with cost_dtype float64; the plan of ensure_colsweep picks the group axis itself, and it is the generator's `gax` for
the rows kept here - for others, e.g. levels 6, nU 16 at n[0] = 61, it is not, which is why the tests read "cs_group_axis" too):

    (levels, big, nU)   cs_groups at n[0] = 45, 60, 61, 120 (gax 2 and gax 3 alike)
    (1, 2.7,  3)        1  1  1  1
    (1, 2.7,  6)        2  2  2  2        (one cell of the group axis: a group splits when a window cell's three slots are full)
    (1, 2.7,  9)        3  3  3  3
    (2, 2.7,  6)        2  2  2  2
    (3, 2.7,  9)        3  3  3  3
    (4, 2.7, 12)        4  4  4  4
    (5, 2.7, 10)        5  5  5* 5        (* gax 2 at n[0] = 61: the plan groups by axis 3; not used)
    (6, 2.7, 16)        6  6  6* 6        (* at n[0] = 61 the plan groups by the other axis; not used)

Every member of these has cs_dpp 1, cs_coop 0 and 3 or 4 parts per column ("cs_split").  At these sizes hjb_solve_batch's own
choice of parts (all the batch's columns in about one round of the wave slots) is never SMALLER than a member's, so the handles'
parts are not touched: test_colsweep_batch_that_takes_fewer_parts_gives_them_back is the one place with larger members (8 x
~1e5 states, 16 parts each when alone), where the condition is computed from the sizes and asserted.

The host loop at 100 stages, monitor period 40, graph on (kGraphStages = 32): 21 eager stages to the monitor point 80; a run of
40 = one eager stage (parity), a capture, one replay, 7 eager stages; at 40 exactly one member stops; a run of 39 = one eager
stage, a capture under the smaller mask, one replay, 6 eager stages.  The tolerances come from the oracle's own |e| at the two
points (the midpoint, asserted apart by more than 1e-6), the stop from the member's results and progress calls."""
import contextlib
import ctypes as C

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


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def _retype(hjbdp, spec, **kw):
    args = dict(dtype=spec.dtype, index_base=spec.index_base, j_storage=None if spec.j_dtype == spec.dtype else spec.j_dtype,
                idx_dtype=spec.idx_dtype, table_dtype=spec.table_dtype, cost_dtype=spec.cost_dtype)
    args.update(kw)
    return hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, **args)


def _terminal(spec, seed, offset=0.0):
    return (offset + np.random.default_rng(seed).random(spec.nS)).astype(spec.j_dtype)


def _bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a


def _job(term=None, tol=0.0, single=False, progress=False, null=False):
    """One member's own options: terminal (None: zeros), monitor_tol, monitor_single, a progress callback, null outputs."""
    return {"term": term, "tol": float(tol), "single": bool(single), "progress": bool(progress), "null": bool(null)}


_FIELDS = ("stages_done", "stopped_early", "last_e", "last_e2")


def _oracle(env, spec, job, n_st, period=0):
    """oracle/c_oracle.sweep of the member, with the oracle's progress calls [(k_s, e, e2)] beside its results."""
    hjbdp, _abi, c_oracle = env
    lib = c_oracle.lib(_abi)
    p, keep = spec.to_c()
    o, r = _abi.hjb_solve_opts(), _abi.hjb_result()
    o.n_stages, o.monitor_period, o.monitor_tol, o.monitor_single = n_st, period, job["tol"], int(job["single"])
    if job["term"] is not None:
        keep.append(np.ascontiguousarray(job["term"], dtype=spec.j_dtype))
        o.terminal = keep[-1].ctypes.data
    events = []
    cb = _abi.hjb_progress_fn(lambda user, k_s, e, e2, sec: events.append((k_s, e, e2)))
    o.progress = cb
    J, idx = np.empty(spec.nS, dtype=spec.j_dtype), np.empty(spec.nS, dtype=np.int32)
    o.J_final, o.idx_final = J.ctypes.data, idx.ctypes.data
    assert lib.orc_sweep(C.byref(p), C.byref(o), C.byref(r), lib.orc_max_threads()) == 0
    assert np.isfinite(J.astype(np.float64)).all()                 # (labels of NaN totals are not defined)
    return {"J": J, "idx": idx, "stages_done": r.stages_done, "stopped_early": bool(r.stopped_early), "last_e": r.last_e,
            "last_e2": r.last_e2, "events": events}


def _solo(bk, job, n_st, period=0):
    """The handle's own hjb_solve of the member."""
    events = []
    out = bk.solve(n_st, terminal=job["term"], monitor_period=period, monitor_tol=job["tol"], monitor_single=job["single"],
                   progress=lambda k_s, e, e2, sec: events.append((k_s, e, e2)))
    out["events"] = events
    return out


def _batch(env, bks, jobs, n_st, period=0, edit=None):
    """hjb_solve_batch on the handles.  -> (status, [member's results, None for a member with null outputs]).  edit(i, opts): a
    last change of member i's hjb_solve_opts (the refusals)."""
    hjbdp, _abi, _ = env
    n = len(bks)
    optp, resp = (C.POINTER(_abi.hjb_solve_opts) * n)(), (C.POINTER(_abi.hjb_result) * n)()
    keep, outs = [], []
    for i, (bk, job) in enumerate(zip(bks, jobs)):
        s = bk.spec
        o, r = _abi.hjb_solve_opts(), _abi.hjb_result()
        o.n_stages, o.monitor_period, o.monitor_tol, o.monitor_single = n_st, period, job["tol"], int(job["single"])
        if job["term"] is not None:
            keep.append(np.ascontiguousarray(job["term"], dtype=s.j_dtype))
            o.terminal = keep[-1].ctypes.data
        events = []
        if job["progress"]:
            keep.append(_abi.hjb_progress_fn(lambda user, k_s, e, e2, sec, ev=events: ev.append((k_s, e, e2))))
            o.progress = keep[-1]
        J, idx = np.empty(s.nS, dtype=s.j_dtype), np.empty(s.nS, dtype=s.idx_np_dtype)
        if not job["null"]:
            o.J_final, o.idx_final = J.ctypes.data, idx.ctypes.data
            resp[i] = C.pointer(r)
        if edit is not None:
            edit(i, o, keep)
        optp[i] = C.pointer(o)
        keep += [o, r]
        outs.append((J, idx, r, events))
    hs = (C.c_void_p * n)(*[bk._h for bk in bks])
    st = bks[0].lib.hjb_solve_batch(n, hs, optp, resp)
    res = []
    for (J, idx, r, events), job in zip(outs, jobs):
        res.append(None if job["null"] else {"J": J, "idx": idx, "stages_done": r.stages_done, "stopped_early": bool(r.stopped_early),
                                             "last_e": r.last_e, "last_e2": r.last_e2, "events": events})
    return st, res


def _equal(got, want, what, events=False):
    assert got["J"].dtype == want["J"].dtype and np.array_equal(_bits(got["J"]), _bits(want["J"])), what
    assert np.array_equal(got["idx"], want["idx"]), what
    for f in _FIELDS:
        assert got[f] == want[f], (what, f, got[f], want[f])
    if events:
        assert got["events"] == want["events"], (what, got["events"], want["events"])


def _sweep_and_check(env, bks, jobs, n_st, period=0, refs=None):
    """The bar of this file: every member's batch results = the oracle's = the handle's own hjb_solve before = after."""
    _abi = env[1]
    refs = refs or [_oracle(env, bk.spec, job, n_st, period) for bk, job in zip(bks, jobs)]
    before = [_solo(bk, job, n_st, period) for bk, job in zip(bks, jobs)]
    st, outs = _batch(env, bks, jobs, n_st, period)
    assert st == _abi.HJB_OK, bks[0].lib.hjb_last_error(bks[0]._h)
    after = [_solo(bk, job, n_st, period) for bk, job in zip(bks, jobs)]
    for i, (ref, b, o, a, job) in enumerate(zip(refs, before, outs, after, jobs)):
        _equal(b, ref, ("hjb_solve before the batch against the oracle", i), events=True)
        _equal(a, b, ("hjb_solve after the batch against before it", i), events=True)
        if o is not None:
            _equal(o, ref, ("batch against the oracle", i), events=job["progress"])
            _equal(o, b, ("batch against the handle's own hjb_solve", i), events=job["progress"])
    return refs, outs


@contextlib.contextmanager
def _handles(hjbdp, specs, variant, options=()):
    with contextlib.ExitStack() as stack:
        bks = [stack.enter_context(hjbdp.Backup(s)) for s in specs]
        for bk in bks:
            bk.set_option("variant", variant)
            for k, v in options:
                bk.set_option(k, v)
        yield bks


def _assert_table_form(bks):
    for bk in bks:
        inf = bk.info()
        assert inf["kernel_variant"] == 5 and bk.get_option("tabled_i32") == 1 and inf["block"] == 256, inf


def _tol_between(events, point):
    """The tolerance that stops a sweep at monitor point `point` and not before: the midpoint between the oracle's own |e| there and
    the smallest |e| of the points before it, which must lie apart."""
    e = {k: abs(v) for k, v, _ in events}
    pts = [k for k, _, _ in events]
    earlier = min(e[k] for k in pts[:pts.index(point)])
    assert earlier > e[point] * (1 + 1e-6), (point, e)
    return 0.5 * (earlier + e[point])


# ---- 1. the table kernel: every (storage, D) ----------------------------------------------------------------------------------------
_TABLE_RAN = set()
TABLE_GRIDS = {1: [(200,), (1300,), (700,), (90,)], 2: [(13, 17), (37, 41), (30, 25), (9, 11)],
               3: [(6, 6, 6), (11, 12, 13), (9, 8, 7), (5, 4, 5)], 4: [(4, 4, 3, 4), (6, 7, 6, 7), (5, 5, 4, 5), (3, 4, 3, 3)]}
TABLE_CONTROLS = [(5,), (3, 4), (3, 2, 2), (4,)]


def _table_members(hjbdp, storage, D):
    """Members that differ on purpose.  0: fewer states than one workgroup, one control dim, index_base 0, uint8 labels; 1: >= 5
    workgroups and not a whole number of them, two control dims, uneven knots, uint16 labels; 2: three control dims, int32 labels,
    zero terminal - in the f32 rows with table_dtype float64; 3 (f32 rows only): cost_dtype float64.  variant_status admits both
    typings on variant 5 (read on the device: "variant" 5 is accepted, info() reports the typing), so no member is dropped."""
    from problems import random_problem
    arith = np.float64 if storage == "f64" else np.float32
    idx = [np.uint8, np.uint16, np.int32, "auto"]
    specs, jobs = [], []
    for i in range(4 if storage == "f32" else 3):
        typed = storage == "f32" and i >= 2
        s = random_problem(5000 + 10 * D + i, TABLE_GRIDS[D][i], TABLE_CONTROLS[i], dtype=np.float64 if typed else arith,
                           nonuniform=(i == 1), index_base=0 if i in (0, 3) else 1, spread=0.15)
        kw = {"idx_dtype": idx[i]}
        if storage == "f16":
            kw["j_storage"] = np.float16
        if typed:
            kw.update(dtype=np.float32, **({"table_dtype": np.float64} if i == 2 else {"cost_dtype": np.float64}))
        s = _retype(hjbdp, s, **kw)
        specs.append(s)
        jobs.append(_job(term=None if i == 2 else _terminal(s, 30 + i)))
    return specs, jobs


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("storage", ["f32", "f64", "f16"])
def test_table_kernel_batch_at_every_storage_and_dimension(env, storage, D):
    hjbdp, _abi, _ = env
    specs, jobs = _table_members(hjbdp, storage, D)
    assert specs[0].nS < 256 and specs[1].nS % 256 != 0 and -(-specs[1].nS // 256) >= 5
    assert {len(s.m) for s in specs} >= {1, 2, 3} and {s.index_base for s in specs} == {0, 1}
    assert [s.idx_np_dtype for s in specs[:3]] == [np.uint8, np.uint16, np.int32]
    assert all(s.j_dtype == {"f32": np.float32, "f64": np.float64, "f16": np.float16}[storage] for s in specs)
    with _handles(hjbdp, specs, 5) as bks:
        _assert_table_form(bks)
        grids = [bk.info()["grid"] for bk in bks]
        assert grids[1] == max(grids) and grids[0] == 1 and sorted(grids)[-2] < grids[1], grids      # one member sets the launch
        if storage == "f32":
            assert bks[2].info()["table_dtype"] == _abi.HJB_TAB_F64 and bks[3].info()["cost_dtype"] == _abi.HJB_COST_F64
            assert all(bk.info()["table_dtype"] == 0 for bk in bks[:2]) and all(bk.info()["cost_dtype"] == 0 for bk in bks[:3])
        _sweep_and_check(env, bks, jobs, STAGES)
    _TABLE_RAN.add((storage, D))


# ---- 2. the table kernel: eight problems, and one -----------------------------------------------------------------------------------
EIGHT = [(13, 17), (37, 41), (30, 25), (50, 40), (20, 11), (64, 33), (7, 9), (45, 45)]
EIGHT_STOPS = [None, 4, 16, 12, 16, None, 16, None]        # the monitor point each member stops at (None: never)


def test_table_kernel_batch_of_eight_members_stopping_at_different_points(env):
    """kCsBatchMax = 8 members (mask 0xff) in D = 2 float64, 20 stages, monitor points 20, 16, 12, 8, 4.  Members stop at three
    different points and three never do: the mask loses bits at three monitor points, and the members still running are the
    ones whose buffers go on."""
    hjbdp, _abi, _ = env
    from problems import random_problem
    n_st, period = 20, 4
    specs, jobs = [], []
    for i, n in enumerate(EIGHT):
        s = random_problem(2200 + i, n, (3, 4) if i == 3 else (3 + i % 4,), dtype=np.float64, nonuniform=bool(i & 1),
                           index_base=i & 1, spread=0.02)
        term = 50.0 * _terminal(s, 40 + i)
        free = _oracle(env, s, _job(term=term), n_st, period)
        assert [k for k, _, _ in free["events"]] == [20, 16, 12, 8, 4]
        tol = 0.0 if EIGHT_STOPS[i] is None else _tol_between(free["events"], EIGHT_STOPS[i])
        specs.append(s)
        jobs.append(_job(term=term, tol=tol, progress=True))
    with _handles(hjbdp, specs, 5) as bks:
        _assert_table_form(bks)
        refs, outs = _sweep_and_check(env, bks, jobs, n_st, period)
    for ref, o, stop in zip(refs, outs, EIGHT_STOPS):
        assert o["stopped_early"] == (stop is not None) and o["stages_done"] == (n_st if stop is None else n_st - stop + 1)
        assert [k for k, _, _ in o["events"]] == [k for k in (20, 16, 12, 8, 4) if stop is None or k >= stop]
    assert len({s for s in EIGHT_STOPS if s}) >= 3 and EIGHT_STOPS.count(None) >= 2


def test_batch_of_one_member_equals_solve(env):
    hjbdp, _abi, _ = env
    from problems import random_problem
    s = random_problem(2300, (23, 19), (4,), dtype=np.float64, index_base=1)
    with _handles(hjbdp, [s], 5) as bks:
        _assert_table_form(bks)
        _sweep_and_check(env, bks, [_job(term=_terminal(s, 5))], STAGES)


# ---- 3. the column sweep: every (group axis, cost typing, NG), NG above a member's own ----------------------------------------------
_COLSWEEP_RAN = set()
CS_GRIDS = {45: (45, 9, 8, 8), 60: (60, 8, 7, 8), 61: (61, 7, 8, 8), 120: (120, 6, 6, 6)}
CS_ROWS = {
    # target NG: [((levels, big, nU), n[0]), ...]; the first member has NG groups (the module docstring's table)
    1: [((1, 2.7, 3), 61), ((1, 2.7, 3), 45)],
    2: [((2, 2.7, 6), 120), ((1, 2.7, 3), 45)],
    3: [((3, 2.7, 9), 61), ((1, 2.7, 6), 60), ((1, 2.7, 3), 120)],
    4: [((4, 2.7, 12), 45), ((3, 2.7, 9), 120)],
    5: [((5, 2.7, 10), 60), ((2, 2.7, 6), 61), ((4, 2.7, 12), 45)],
    6: [((6, 2.7, 16), 120), ((5, 2.7, 10), 45), ((1, 2.7, 3), 61)],
}
CS_EXPLICIT_SPLIT_ROW = 3           # the row of each (gax, typing) in which member 1 carries an explicit "cs_split"


def _colsweep_spec(hjbdp, knobs, n0, gax, c64, n=None, seed=None):
    from problems import colsweep_problem
    levels, big, nU = knobs
    seed = 3000 + 10 * levels + nU + n0 if seed is None else seed
    s = colsweep_problem(seed, n or CS_GRIDS[n0], nU=nU, gax=gax, big=big, levels=levels, cost="fast")
    return _retype(hjbdp, s, cost_dtype=np.float64) if c64 else s


def _assert_colsweep_form(bks, gax, c64):
    for bk in bks:
        inf = bk.info()
        assert inf["kernel_variant"] == 7 and bk.get_option("cs_dpp") == 1 and bk.get_option("cs_coop") == 0, inf
        assert bk.get_option("cs_group_axis") == gax and inf["cost_dtype"] == (1 if c64 else 0), (bk.get_option("cs_group_axis"), inf)


def _parts(bks):
    return [(bk.get_option("cs_split"), bk.info()["grid"]) for bk in bks]


@pytest.mark.parametrize("NG", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("c64", [False, True], ids=["c32", "c64"])
@pytest.mark.parametrize("gax", [2, 3])
def test_colsweep_batch_under_a_group_count_above_a_members_own(env, gax, c64, NG):
    hjbdp, _abi, _ = env
    specs = [_colsweep_spec(hjbdp, knobs, n0, gax, c64) for knobs, n0 in CS_ROWS[NG]]
    assert len({s.n[0] for s in specs}) == len(specs)                # the axis-0 chunk count differs inside the batch
    jobs = [_job(term=None if i == len(specs) - 1 else _terminal(s, 60 + i)) for i, s in enumerate(specs)]
    with _handles(hjbdp, specs, 7) as bks:
        _assert_colsweep_form(bks, gax, c64)
        groups = [bk.get_option("cs_groups") for bk in bks]
        assert max(groups) == NG and groups[0] == NG, groups
        if NG >= 2:
            assert min(groups) < NG, groups                            # a member runs under more groups than its own plan has
        if NG == CS_EXPLICIT_SPLIT_ROW:
            assert bks[1].get_option("cs_split") != 2
            bks[1].set_option("cs_split", 2)
            assert bks[1].get_option("cs_split") == 2
        parts = _parts(bks)
        _sweep_and_check(env, bks, jobs, STAGES)
        assert _parts(bks) == parts, (parts, _parts(bks))
    _COLSWEEP_RAN.add((gax, c64, NG))


def test_colsweep_batch_that_takes_fewer_parts_gives_them_back(env):
    """hjb_solve_batch lowers a member's parts per column when all the batch's columns would otherwise need more than one round
    of the wave slots, and gives every handle its own parts back on the way out.  That takes members whose own choice is large
    (a long axis 1) and many columns: eight members of 7e4 .. 1.3e5 states, 16 parts each when alone, 548 columns together - the
    only sizes in this file above 3e4 states, because below them the path is not taken.  Member 5 carries an explicit option."""
    hjbdp, _abi, _ = env
    grids = [(45, 32, 7, 7), (60, 32, 7, 7), (61, 32, 8, 7), (45, 32, 8, 8)]
    four = [_colsweep_spec(hjbdp, (5, 2.7, 9), n[0], 3, False, n=n, seed=3500 + n[0]) for n in grids]
    specs = four + four
    jobs = [_job(term=None if i == 7 else _terminal(s, 80 + i)) for i, s in enumerate(specs)]
    with _handles(hjbdp, specs, 7) as bks:
        _assert_colsweep_form(bks, bks[0].get_option("cs_group_axis"), False)
        bks[5].set_option("cs_split", 5)
        parts = _parts(bks)
        columns = sum(-(-s.n[0] // 60) * s.n[2] * s.n[3] for s in specs)         # hjbdp_batch.hip: kCsDppLanes = 60 states per wave
        s_batch = max(1, 6 * 4 * 256 // columns)
        assert all(p == 16 for i, (p, _) in enumerate(parts) if i != 5) and parts[5][0] == 5 and 5 < s_batch < 16, (parts, s_batch)
        _sweep_and_check(env, bks, jobs, STAGES)
        assert _parts(bks) == parts, (parts, _parts(bks))


# ---- 4. the host loop at its edges, on both kernels ---------------------------------------------------------------------------------
LOOP_STAGES, LOOP_PERIOD = 100, 40
LOOP_STOPPER = 1                    # the member that stops at monitor point 40


def _loop_table_specs(hjbdp, storage):
    from problems import random_problem
    grids, controls = [(37, 41), (13, 17), (30, 25)], [(4,), (3, 2), (4,)]
    specs = []
    for i in range(3):
        s = random_problem(4100 + i, grids[i], controls[i], dtype=np.float32, nonuniform=(i == 2), index_base=i & 1, spread=0.004)
        specs.append(_retype(hjbdp, s, **({"j_storage": np.float16} if storage == "f16" else {"dtype": np.float64} if storage == "f64" else {})))
    return specs


def _loop_colsweep_specs(hjbdp):
    grids = [(61, 4, 4, 5), (60, 4, 5, 4), (45, 5, 4, 4)]
    return [_colsweep_spec(hjbdp, (1, 2.7, nU), n[0], 2, False, n=n) for nU, n in zip((9, 6, 3), grids)]


def _loop_jobs(env, specs, single_on):
    """Member LOOP_STOPPER starts from a terminal cost 300 above the others', so that the oracle's |e| at the first monitor point
    (the whole sum) is far above the one at the second (40 stages' growth); its tolerance is the midpoint.  The others never stop."""
    jobs = []
    for i, s in enumerate(specs):
        single = i in single_on
        term = _terminal(s, 70 + i, offset=300.0 if i == LOOP_STOPPER else 0.0)
        tol = 0.0
        if i == LOOP_STOPPER:
            free = _oracle(env, s, _job(term=term, single=single), LOOP_STAGES, LOOP_PERIOD)
            assert [k for k, _, _ in free["events"]] == [80, 40]
            tol = _tol_between(free["events"], 40)
        jobs.append(_job(term=term, tol=tol, single=single, progress=True))
    return jobs


def _loop_scenario(env, bks, jobs):
    refs, outs = _sweep_and_check(env, bks, jobs, LOOP_STAGES, LOOP_PERIOD)
    for i, o in enumerate(outs):
        stops = i == LOOP_STOPPER
        assert o["stopped_early"] == stops and o["stages_done"] == (LOOP_STAGES - 40 + 1 if stops else LOOP_STAGES), (i, o["stages_done"])
        assert [k for k, _, _ in o["events"]] == [80, 40], (i, o["events"])        # once per monitor point while the member runs
    assert all(bk.get_option("graph") == 1 for bk in bks)
    for bk in bks:
        bk.set_option("graph", 0)
    st, eager = _batch(env, bks, jobs, LOOP_STAGES, LOOP_PERIOD)
    assert st == env[1].HJB_OK
    for i, (o, e) in enumerate(zip(outs, eager)):
        _equal(e, o, ("graph 0 against graph 1", i), events=True)
    for bk in bks:
        bk.set_option("graph", 1)
    # null outputs on one member leave the others correct
    nulled = [dict(j, null=(i == 0)) for i, j in enumerate(jobs)]
    st, part = _batch(env, bks, nulled, LOOP_STAGES, LOOP_PERIOD)
    assert st == env[1].HJB_OK and part[0] is None
    for i in (1, 2):
        _equal(part[i], outs[i], ("beside a member with null outputs", i), events=True)
    return outs


@pytest.mark.parametrize("storage,single_on", [("f32", ()), ("f32", (LOOP_STOPPER,)), ("f16", (LOOP_STOPPER,)), ("f64", (0, 1, 2))],
                         ids=["f32", "f32-single-on-one-member", "f16-single-on-one-member", "f64-single-ignored"])
def test_host_loop_on_the_table_kernel(env, storage, single_on):
    """The walk of the module docstring on three table-kernel members in D = 2.  monitor_single on the stopping member only is a
    per-problem option: its |e| and its comparison are float32's, the others' double's (with float32 storage the two monitors
    see different numbers, asserted; 221 binary16 values sum exactly either way).  f64: monitor_single on every member is
    ignored - the results equal the double monitor's."""
    hjbdp, _abi, _ = env
    specs = _loop_table_specs(hjbdp, storage)
    jobs = _loop_jobs(env, specs, single_on)
    with _handles(hjbdp, specs, 5) as bks:
        _assert_table_form(bks)
        outs = _loop_scenario(env, bks, jobs)
        if storage == "f64":
            plain = [dict(j, single=False) for j in jobs]
            st, double = _batch(env, bks, plain, LOOP_STAGES, LOOP_PERIOD)
            assert st == _abi.HJB_OK
            for i, (o, d) in enumerate(zip(outs, double)):
                _equal(d, o, ("the double monitor against monitor_single on float64", i), events=True)
        if storage == "f32" and single_on:   # the option is not a no-op: the same member under the double monitor sees another |e|
            other = _solo(bks[LOOP_STOPPER], dict(jobs[LOOP_STOPPER], single=False, tol=0.0), LOOP_STAGES, LOOP_PERIOD)
            assert [e for _, e, _ in other["events"]] != [e for _, e, _ in outs[LOOP_STOPPER]["events"]]


def test_host_loop_on_the_column_sweep(env):
    """The same walk on three column-sweep members of 3, 2 and 1 groups: the captured launches are the NG = 3 kernel's, before and
    after the member with 2 groups has stopped."""
    hjbdp, _abi, _ = env
    specs = _loop_colsweep_specs(hjbdp)
    jobs = _loop_jobs(env, specs, ())
    with _handles(hjbdp, specs, 7) as bks:
        _assert_colsweep_form(bks, 2, False)
        groups = [bk.get_option("cs_groups") for bk in bks]
        assert max(groups) > min(groups) and groups[LOOP_STOPPER] < max(groups), groups
        parts = _parts(bks)
        _loop_scenario(env, bks, jobs)
        assert _parts(bks) == parts


@pytest.mark.parametrize("kernel", ["table", "colsweep"])
@pytest.mark.parametrize("n_st,period", [(1, 0), (1, 1), (5, 1)])
def test_one_stage_and_a_monitor_at_every_stage(env, kernel, n_st, period):
    """n_stages = 1 (one launch, the result in buffer 1) and monitor_period = 1 (a monitor point after every launch; with five
    stages member 1 stops at the second: its terminal cost lies 300 above the others', so the first |e| is the largest)."""
    hjbdp, _abi, _ = env
    specs = _loop_table_specs(hjbdp, "f32") if kernel == "table" else _loop_colsweep_specs(hjbdp)
    jobs = [_job(term=_terminal(s, 90 + i, offset=300.0 if i == 1 else 0.0), progress=True) for i, s in enumerate(specs)]
    if (n_st, period) == (5, 1):
        free = _oracle(env, specs[1], jobs[1], n_st, period)
        jobs[1]["tol"] = _tol_between(free["events"], 4)
    with _handles(hjbdp, specs, 5 if kernel == "table" else 7) as bks:
        refs, outs = _sweep_and_check(env, bks, jobs, n_st, period)
    if (n_st, period) == (5, 1):
        assert outs[1]["stopped_early"] and outs[1]["stages_done"] == 2 and outs[0]["stages_done"] == outs[2]["stages_done"] == 5
    assert all(len(o["events"]) == (o["stages_done"] if period else 0) for o in outs)


# ---- 5. refusals leave every handle as it was ---------------------------------------------------------------------------------------
def _state(bk, J_next):
    J, idx = bk.backup_stage(J_next)
    return bk.info(), _bits(J).copy(), idx.copy()


def _refused(env, bks, n_st=STAGES, period=0, edit=None, text=None):
    """The batch is refused with HJB_E_UNSUPPORTED, and info() and one backup_stage of every handle read as before."""
    _abi = env[1]
    nexts = [np.random.default_rng(11 + i).random(bk.info()["j_elems"]).astype(bk.spec.j_dtype) for i, bk in enumerate(bks)]
    before = [_state(bk, Jn) for bk, Jn in zip(bks, nexts)]
    st, _ = _batch(env, bks, [_job() for _ in bks], n_st, period, edit=edit)
    assert st == _abi.HJB_E_UNSUPPORTED, st
    if text:
        assert any(text in (bk.lib.hjb_last_error(bk._h) or b"") for bk in bks), [bk.lib.hjb_last_error(bk._h) for bk in bks]
    for (inf, J, idx), bk, Jn in zip(before, bks, nexts):
        inf2, J2, idx2 = _state(bk, Jn)
        assert inf2 == inf and np.array_equal(J2, J) and np.array_equal(idx2, idx)


def _table_pair(hjbdp, **kw):
    from problems import random_problem
    return [random_problem(6000 + i, (15, 14), (4,), dtype=np.float32, index_base=1, **kw) for i in range(2)]


def _colsweep_pair(hjbdp):
    return [_colsweep_spec(hjbdp, (1, 2.7, 3), 45, 3, False, n=(45, 5, 5, 6)), _colsweep_spec(hjbdp, (2, 2.7, 6), 60, 3, False, n=(60, 5, 5, 6))]


def test_refusals_of_unlike_table_kernel_members(env):
    hjbdp, _abi, _ = env
    from problems import random_problem
    a, b = _table_pair(hjbdp)
    cases = {
        "mixed dtype": [a, _retype(hjbdp, b, dtype=np.float64)],
        "mixed storage": [a, _retype(hjbdp, b, j_storage=np.float16)],
        "mixed D": [a, random_problem(6002, (7, 6, 5), (4,), dtype=np.float32, index_base=1)],
        "D = 5": [random_problem(6003 + i, (4, 3, 3, 3, 2), (3,), dtype=np.float32) for i in range(2)],
    }
    for name, specs in cases.items():
        with _handles(hjbdp, specs, 5) as bks:
            _assert_table_form(bks)
            _refused(env, bks)
    with _handles(hjbdp, [a, b], 5) as bks:                     # the 64-bit form of the table kernel on one member
        bks[1].set_option("tabled_i32", 0)
        assert bks[1].get_option("tabled_i32") == 0 and bks[1].info()["kernel_variant"] == 5
        _refused(env, bks)


def test_refusal_of_a_slab_handle(env):
    hjbdp, _abi, _ = env
    from problems import random_problem
    a = random_problem(6010, (12, 11, 14), (4,), dtype=np.float32, index_base=1, spread=0.05)
    with hjbdp.Backup(a, variant=5) as whole:
        need = whole.info()
    b, e = 4, 10
    hl, hh = min(max(need["halo_needed_lo"], 1), b), min(max(need["halo_needed_hi"], 1), a.n[-1] - e)
    with hjbdp.Backup(a, variant=5) as bk0, hjbdp.Backup(a, slab=(b, e, hl, hh), variant=5) as bk1:
        inf = bk1.info()
        assert inf["kernel_variant"] == 5 and bk1.get_option("tabled_i32") == 1 and inf["j_elems"] > inf["n_states"]
        _refused(env, [bk0, bk1])
        _refused(env, [bk1, bk0])


def test_refusals_of_unlike_column_sweep_members(env):
    hjbdp, _abi, _ = env
    from problems import colsweep_problem
    a, b = _colsweep_pair(hjbdp)
    with _handles(hjbdp, [a, b], 7) as bks:                     # (the pair itself is taken)
        _assert_colsweep_form(bks, 3, False)
        _sweep_and_check(env, bks, [_job(), _job()], 1)
    ta = _table_pair(hjbdp)[0]
    for order in ((0, 1), (1, 0)):                              # a variant-5 member beside a variant-7 member, either first
        with hjbdp.Backup(ta, variant=5) as t, hjbdp.Backup(a, variant=7) as c:
            assert t.info()["kernel_variant"] == 5 and c.info()["kernel_variant"] == 7
            _refused(env, [(t, c)[i] for i in order])
    cases = {
        "float16 storage": _retype(hjbdp, b, j_storage=np.float16),
        "cost shape": colsweep_problem(3100, (60, 5, 5, 6), nU=6, gax=3, levels=2, cost="multi"),
        "group axis": _colsweep_spec(hjbdp, (2, 2.7, 6), 60, 2, False, n=(60, 5, 6, 5)),
        "cost typing": _retype(hjbdp, b, cost_dtype=np.float64),
    }
    for name, other in cases.items():
        with _handles(hjbdp, [a, other], 7) as bks:
            assert all(bk.info()["kernel_variant"] == 7 for bk in bks), name
            if name == "group axis":
                assert [bk.get_option("cs_group_axis") for bk in bks] == [3, 2]
            _refused(env, bks)
    with _handles(hjbdp, [a, b], 7) as bks:                     # the two-loads-per-row form on one member
        bks[1].set_option("cs_dpp", 0)
        assert bks[1].get_option("cs_dpp") == 0
        _refused(env, bks)
    # the cooperative form, on a problem whose plan offers it (axis 1 sees the group axis only; n[0] a multiple of 4)
    coop = [colsweep_problem(914, (8, 4, 3, 4), nU=6, gax=3, cost="fast", levels=3, a1_axis=3) for _ in range(2)]
    with _handles(hjbdp, coop, 7) as bks:
        _sweep_and_check(env, bks, [_job(), _job()], 1)         # (taken in the usual form)
        bks[1].set_option("cs_coop", 1)
        assert bks[1].get_option("cs_coop") == 1, bks[1].get_option("cs_coop_why")
        _refused(env, bks)


def test_refusals_of_options_a_batch_does_not_take(env):
    hjbdp, _abi, _ = env
    specs = _table_pair(hjbdp)

    def stages(i, o, keep):
        if i == 1:
            o.n_stages = STAGES + 1

    def period(i, o, keep):
        if i == 1:
            o.monitor_period = 2

    def per_stage(i, o, keep):
        if i == 1:
            keep.append(np.zeros((specs[1].nS, STAGES), dtype=specs[1].j_dtype, order="F"))
            o.J_stages = keep[-1].ctypes.data

    def probe(i, o, keep):
        if i == 0:
            pb = _abi.hjb_probe()
            pb.hi[0] = pb.hi[1] = 2
            keep.append(np.zeros((2, 2, STAGES), dtype=specs[0].dtype, order="F"))
            pb.g = keep[-1].ctypes.data
            keep.append(pb)
            o.probe = C.pointer(pb)

    with _handles(hjbdp, specs, 5) as bks:
        _assert_table_form(bks)
        for edit in (stages, period, per_stage, probe):
            _refused(env, bks, edit=edit)
        _sweep_and_check(env, bks, [_job(), _job()], STAGES)     # ... and the same handles are taken without them


# ---- 6. closing the table -----------------------------------------------------------------------------------------------------------
def test_every_batched_instantiation_was_launched():
    """Runs after the parametrised cases."""
    assert _TABLE_RAN == {(s, D) for s in ("f32", "f64", "f16") for D in (1, 2, 3, 4)}, _TABLE_RAN
    assert _COLSWEEP_RAN == {(g, c, NG) for g in (2, 3) for c in (False, True) for NG in range(1, 7)}, _COLSWEEP_RAN
