"""GPU tests (-m gpu): the cost-to-go's value range in every kernel that stores or reads it.

The parity suite feeds every stage kernel a terminal in [0, 1) and costs of order one, so no kernel ever stored or read a
subnormal of its storage type, a value on the normal / subnormal boundary, a signed zero, a value in binary16's top binade or one
that the store rounds to 65504 rather than to infinity (or the other way round).  The binary16 paths are written by hand in a dozen
places (stj / ldj, raw_to and the async store of the column sweep, the h2u pair loads of the table and packed kernels, the LDS tiles
of K9 and K15, the monitor's partial sums), each compiled on its own: a convert that rounds toward zero, packed binary16
arithmetic, a min3 on +-0 or a flush-to-zero flag on one translation unit would pass the rest of the suite.  Here (helpers and
regimes: tests/value_range.py, checked on the CPU by tests/test_value_range_refs.py):

a. the store census: fill_separable on a binary16-storage handle over every finite half, every midpoint between two halves and
   the midpoints' float32 neighbours (plus a -0 axis: x + (-0) = x) against half_rne, integer arithmetic on the float32 bits.
b. the identity stage: integer knots, the next state is the knot itself, one control whose cost is -0.0 - a stage returns its
   input bit for bit at every state that is not the last point of an axis.  The input holds every finite half (binary16), or
   float32 / float64 subnormals of every binade, normals up to 2^126 / 2^1022 and both zeros.  For every variant the problem
   accepts, through K9 (16 and 19 stages) and through the monitor's sums in both precisions.
c. regime sweeps: three stages (`top`: one) of every kernel family and form, with each storage type it is built for, against the C
   twin: J of every stage as raw bits, labels, progress events; slab handles into NaN-prefilled buffers; hjb_solve_batch with
   members in three different regimes.  The launch of the scaled problem equals the unscaled one's.

No tolerance appears: a difference between a kernel and the twin in any regime is a bug in one of them.  NaN or infinity as the
INPUT of a stage are out of scope (`top` is one stage: reading a stored infinity back gives inf - inf), and so are the rollout
kernels' value planes.

d. the other readers and writers of stored J, one `sub` and one `edge` case per storage type each builds: the fixed-label stage
   (K22) against the rational reference of tests/evaluate_refs.py, the disturbed stage (K24, five kernels, both modes) against
   tests/disturbance_refs.py, hjb_policy_lookup 'linear' on subnormal value tables against scipy.

What the device reported (MI355X): the identity problem accepts variants 0, 5 (both index forms) and 6 in binary16 storage and 0, 1,
3, 5 (both forms) and 6 in float32 / float64; the cooperative column-sweep form is admitted on the twin of the corpus's `cs_coop`
entry whose axis 1 moves with axis 2 and refused (cs_coop_why 2) on the entry itself, so both are asked; the batched column sweep
is built for float32 storage only, and the pos-att channel has no `top` regime (value_range.NO_TOP says why).  Nothing differed
from the twin or the references in any regime.

Mutations tried by hand and reverted (each on a rebuilt library): a round-toward-zero binary16 convert in stj and in the fill
kernel fails a, b and c; -fgpu-flush-denormals-to-zero on stage_tabled.hip alone fails b and c for variant 5 only (and the batched
table kernel); +0.0 instead of -0.0 as the identity problem's cost fails b on the -0 pattern alone.

Wall time of the default `-m gpu` run on one MI355X box, both runs back to back (tests/conftest.py states a 540 s budget): 386 s
without this file (970 tests), 378 s with it (1,114 tests) - the difference is the box's run-to-run noise; this file's 144 tests
take 5.2 s when run alone, the oracle's sweeps included (0.4 s the slowest), so nothing of it is `extended`."""
import contextlib

import numpy as np
import pytest

import value_range as vr

pytestmark = pytest.mark.gpu

TILE_K = 8                                  # csrc/kernels_tile2d.h: stages per K9 launch


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi, c_oracle


def _snap(bk):
    from test_gpu_launch_choice import _snap as snap
    return snap(bk)


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(vr.bits(got).reshape(-1) != vr.bits(want).reshape(-1))
    assert bad.size == 0, (what, bad.size, bad[:8], got.reshape(-1)[bad[:4]], want.reshape(-1)[bad[:4]],
                           vr.bits(got).reshape(-1)[bad[:4]], vr.bits(want).reshape(-1)[bad[:4]])


def _same_events(got, want, what):
    assert len(got) == len(want) and np.array_equal(np.array(got, dtype=np.float64), np.array(want, dtype=np.float64), equal_nan=True), \
        (what, got, want)


# ---- a. the store census ---------------------------------------------------------------------------------------------------------
def test_store_census_against_half_rne(env):
    """k_fill_separable<float, _Float16>: the same (TJ)v conversion as stj, on every float32 value of the census."""
    hjbdp, _abi, _ = env
    from hjbdp import Term
    x = vr.census32()
    knots = [np.arange(x.size, dtype=np.float64), np.arange(2, dtype=np.float64)]
    spec = hjbdp.ProblemSpec(knots, (1,), [[Term((a,), knots[a].copy())] for a in range(2)], [Term((2,), np.zeros(1))],
                             dtype=np.float32, index_base=1, j_storage=np.float16)
    want = vr.half_rne(x)
    with hjbdp.Backup(spec) as bk, hjbdp.DeviceBuffer(spec.nS * 2) as dJ:
        assert spec.j_dtype == np.float16 and bk.info()["j_elems"] == spec.nS
        bk.fill_separable([x, np.float32([-0.0, -0.0])], dJ)
        got = dJ.download(np.float16).view(np.uint16).reshape(x.size, 2, order="F")
    for col in (0, 1):
        bad = np.flatnonzero(got[:, col] != want)
        assert bad.size == 0, (col, bad.size, x[bad[:8]], got[bad[:8], col], want[bad[:8]])


# ---- b. the identity stage -------------------------------------------------------------------------------------------------------
_IDENTITY_RAN = {}
STORAGES = ["f16s", "f32", "f64"]


@pytest.mark.parametrize("storage", STORAGES)
def test_identity_stage_every_variant(env, storage):
    """One stage of the identity problem under every variant hjb_set_option("variant", v) accepts (variant 5 in both index forms):
    the interior equals the INPUT bit for bit (no oracle in that claim), the whole array and the labels equal the oracle's."""
    hjbdp, _abi, c_oracle = env
    spec = vr.identity_problem(storage)
    J_in = vr.identity_input(storage)
    Jr, ir = c_oracle.backup_stage(_abi, spec, J_in)
    inside = vr.interior_mask()
    ran = []
    for v in range(0, 8):
        forms = [(("tabled_i32", 1),), (("tabled_i32", 0),)] if v == 5 else [()]
        for form in forms:
            with hjbdp.Backup(spec) as bk:
                try:
                    bk.set_option("variant", v)
                except hjbdp.HjbError as e:
                    assert e.status == _abi.HJB_E_UNSUPPORTED, (v, str(e))
                    continue
                if bk.info()["kernel_variant"] != v:
                    continue
                for key, value in form:
                    bk.set_option(key, value)
                    assert bk.get_option(key) == value
                bk.set_option("temporal", 0)               # the stage kernel, not K9
                out = bk.solve(1, terminal=J_in)
                assert bk.info()["kernel_variant"] == v
            what = (storage, "variant %d" % v, form)
            _same_bits(out["J"][inside], J_in[inside], what + ("the interior against the input",))
            _same_bits(out["J"], Jr, what + ("against the oracle",))
            assert np.array_equal(out["idx"], ir), what
            ran.append((v,) + tuple(x for kv in form for x in kv))
    print("\n[value range] identity stage, %s: variants %s" % (storage, ran))
    _IDENTITY_RAN[storage] = ran
    assert {(0,), (5, "tabled_i32", 1), (5, "tabled_i32", 0)} <= set(ran), ran


def test_identity_stage_variants_that_ran():
    """Runs after the parametrised cases: variants 0 and 5, the latter in both index forms, for every storage type."""
    assert sorted(_IDENTITY_RAN) == sorted(STORAGES), _IDENTITY_RAN
    for storage, ran in _IDENTITY_RAN.items():
        assert {(0,), (5, "tabled_i32", 1), (5, "tabled_i32", 0)} <= set(ran), (storage, ran)


@pytest.mark.parametrize("n_stages", [2 * TILE_K, 2 * TILE_K + 3])
@pytest.mark.parametrize("storage", STORAGES)
def test_identity_through_the_several_stages_per_launch_kernel(env, storage, n_stages):
    """K9 (temporal = 2: hjb_solve fails unless K9 ran; it takes sweeps of 16 stages and more), two full launches and two plus one
    of depth 3: J passes through the LDS tile n_stages times.  The states further than n_stages points from an upper face still equal the input."""
    hjbdp, _abi, c_oracle = env
    spec = vr.identity_problem(storage)
    J_in = vr.identity_input(storage)
    ref = c_oracle.sweep(_abi, spec, n_stages, terminal=J_in)
    far = vr.interior_mask(margin=n_stages + 1)
    assert far.sum() == (257 - n_stages - 1) * (249 - n_stages - 1)
    _same_bits(ref["J"][far], J_in[far], (storage, "the oracle itself"))
    with hjbdp.Backup(spec) as bk:
        bk.set_option("temporal", 2)
        out = bk.solve(n_stages, terminal=J_in)
    _same_bits(out["J"][far], J_in[far], (storage, n_stages, "against the input"))
    _same_bits(out["J"], ref["J"], (storage, n_stages, "against the oracle"))
    assert np.array_equal(out["idx"], ref["idx"])


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("storage", STORAGES)
def test_monitor_sums_of_the_census(env, storage, single):
    """k_partial_sums<_Float16 | float | double, float | double> reading subnormals: hjb_solve's monitor after one identity stage
    reports the sums c_oracle.monitor_sums forms of the same array, bit for bit."""
    hjbdp, _abi, c_oracle = env
    spec = vr.identity_problem(storage)
    inside = vr.interior_mask()
    for name, vals in vr.monitor_values(storage).items():
        w = vr.identity_input(storage, vals)
        events = []
        with hjbdp.Backup(spec) as bk:
            bk.set_option("temporal", 0)
            out = bk.solve(1, terminal=w, monitor_period=1, monitor_tol=0.0, monitor_single=single,
                           progress=lambda k_s, e, e2, sec: events.append((k_s, e, e2)))
        _same_bits(out["J"][inside], w[inside], (storage, name, "the array summed is the census"))
        fs, isum = c_oracle.monitor_sums(_abi, spec, out["J"], out["idx"], single=single)
        assert np.isfinite(fs) and (fs > 0 or name == "signed")
        assert len(events) == 1 and events[0][0] == 1, events
        assert np.float64(events[0][1]).view(np.uint64) == np.float64(fs).view(np.uint64), (storage, name, single, events, fs)
        assert events[0][2] == isum == spec.nS and out["last_e"] == events[0][1], (events, isum)


# ---- c. regime sweeps ------------------------------------------------------------------------------------------------------------
_RAN = set()


def _apply(bk, case):
    if bk.info()["kernel_variant"] != case.variant:        # (forcing the variant a handle already has can change its form)
        bk.set_option("variant", case.variant)
    for key, value in case.options:
        bk.set_option(key, value)
    inf = bk.info()
    assert inf["kernel_variant"] == case.variant, (case.id, inf["kernel_variant"])
    for key, value in case.options:
        got = inf["block"] if key == "block" else bk.get_option(key)
        assert got == value or key == "cs_coop", (case.id, key, value, got)      # (cs_coop reads back the form in effect)
    if case.check is not None:
        assert case.check(bk), case.id
    form = case.form
    if form == "mode":
        form = "mode%d" % bk.get_option("packed2_mode")
    elif form == "coop":
        form = "coop" if bk.get_option("cs_coop") == 1 else "coop refused (%d)" % bk.get_option("cs_coop_why")
    elif form == "plan":
        form = "g%d" % bk.get_option("cs_group_axis")
    return (case.variant, form, case.storage)


def _sweep_equals_oracle(bk, r, what):
    events = []
    ref = r["ref"]
    out = bk.solve(r["stages"], terminal=r["terminal"], keep_J=True, keep_idx=True, monitor_period=1, monitor_tol=0.0,
                   progress=lambda k_s, e, e2, sec: events.append((k_s, e, e2)))
    for k in range(r["stages"] - 1, -1, -1):
        _same_bits(out["J_stages"][:, k], ref["J_stages"][:, k], what + ("J of stage column %d" % k,))
        bad = np.flatnonzero(out["idx_stages"][:, k] != ref["idx_stages"][:, k])
        assert bad.size == 0, what + ("labels of stage column %d" % k, bad.size, bad[:8])
    _same_bits(out["J"], ref["J"], what + ("the final J",))
    assert np.array_equal(out["idx"], ref["idx"]), what
    _same_events(events, ref["events"], what)
    assert out["stages_done"] == ref["stages_done"] == r["stages"] and not out["stopped_early"], what


_CASES = vr.sweep_cases()


@pytest.mark.parametrize("case", _CASES, ids=[c.id for c in _CASES])
def test_regime_sweeps_against_the_oracle(env, case):
    """Every regime of the case's storage type on one handle form.  2-D problems run under temporal = 0 (the stage kernel) and
    under the default, which may take K9."""
    hjbdp, _abi, c_oracle = env
    with hjbdp.Backup(case.spec) as b0:
        triple = _apply(b0, case)
        snap0 = _snap(b0)
    for regime in vr.regimes_of(case.spec, case.name):
        r = vr.regime_ref(_abi, c_oracle, case.name, case.spec, regime)
        with hjbdp.Backup(r["spec"]) as bk:
            assert _apply(bk, case) == triple
            assert _snap(bk) == snap0, (case.id, regime, "the launch of the scaled problem", _snap(bk), snap0)
            temporals = (0, 1) if case.spec.D == 2 else (None,)
            for temporal in temporals:
                if temporal is not None:
                    bk.set_option("temporal", temporal)
                _sweep_equals_oracle(bk, r, (case.id, regime, "2^%d" % r["k"], "temporal %s" % temporal))
        _RAN.add(triple + (regime,))


def test_the_forms_that_were_swept():
    """Runs after the parametrised cases: which (kernel_variant, form, storage, regime) ran."""
    ran = {t[:3] for t in _RAN}
    print("\n[value range] swept: %s" % sorted(ran))
    want = set()
    for st in ("f32", "f64", "f16s"):
        want |= {(0, "", st), (5, "i32=1", st), (5, "i32=0", st)}
    want |= {(5, "tab64", "f32"), (5, "cost64", "f32")}
    want |= {(3, "block=%d" % b, st) for b in (256, 1024) for st in ("f32", "f64")}
    want |= {(4, "mode7", st) for st in ("f32", "f16s")}
    want |= {(6, "lean=%d" % l, st) for l in (0, 1) for st in ("f32", "f16s")}
    want |= {(7, "dpp=0", "f32"), (7, "dpp=1", "f32"), (7, "coop", "f32"), (7, "coop", "f16s")}
    assert want <= ran, sorted(want - ran)
    for st in ("f32", "f16s"):
        modes = {int(f[4:]) for v, f, s in ran if v == 4 and s == st}
        assert 0 in modes and modes & {1, 4} and 2 in modes and 5 in modes and 7 in modes, (st, modes)
    assert {s for v, f, s in ran if v == 2} == {"f32"}
    plans = {(f, s) for v, f, s in ran if v == 7 and f.startswith("g")}
    assert {s for f, s in plans} == {"f32", "f16s"} and len({f for f, s in plans}) == 2, plans         # both group axes
    for v, f, s in ran:
        got = {t[3] for t in _RAN if t[:3] == (v, f, s)}
        assert {"sub", "edge"} <= got, (v, f, s, got)
    tops = {t[0] for t in _RAN if t[3] == "top"}
    assert tops == {0, 4, 5, 6, 7}, tops                                  # every variant built for binary16 storage


SLAB_REGIMES = [(name, regime) for name, spec, slab in vr.slab_cases() for regime in vr.regimes_of(spec, name)]


@pytest.mark.parametrize("name,regime", SLAB_REGIMES, ids=["%s-%s" % c for c in SLAB_REGIMES])
def test_slab_stage_into_prefilled_buffers(env, name, regime):
    """One hjb_backup_stage_device of a slab handle from the regime's terminal into a NaN-prefilled J buffer and a 0xff-prefilled
    label buffer: the owned planes equal c_oracle.backup_stage(..., slab=...) bit for bit, the halo planes are still NaN."""
    hjbdp, _abi, c_oracle = env
    from test_gpu_launch_walk import _buffers
    s = vr.slab_ref(_abi, c_oracle, name, regime)
    sp, slab, sub, own = s["spec"], s["slab"], s["input"], s["own"]
    with hjbdp.Backup(s["spec0"], slab=slab) as b0:
        snap0 = _snap(b0)
    with hjbdp.Backup(sp, slab=slab) as bk:
        assert _snap(bk) == snap0 and bk.info()["j_elems"] == sub.size
        bufs = _buffers(hjbdp, bk, sp, sub)
        try:
            bk.backup_stage_device(*bufs)
            bk.check_device_status()
            Jg, ig = bufs[1].download(sp.j_dtype), bufs[2].download(sp.idx_np_dtype)
        finally:
            for d in bufs:
                d.free()
    _same_bits(Jg[own], s["J"][own], (name, regime, "owned planes"))
    assert np.array_equal(ig, s["idx"]), (name, regime)
    outside = np.ones(Jg.size, dtype=bool)
    outside[own] = False
    assert outside.any() and np.isnan(Jg[outside]).all(), (name, regime, "a write outside the owned planes")


@pytest.mark.parametrize("name,variant", vr.BATCHES, ids=[b[0] + "-v%d" % b[1] for b in vr.BATCHES])
def test_batch_of_three_members_in_three_regimes(env, name, variant):
    """hjb_solve_batch's k_backup_tabled32_batch and batched column sweep: one launch per stage over three members that are the
    same problem in three different regimes - sub, edge and the unscaled problem over three stages; with binary16 storage also
    sub, top and the unscaled problem over one stage.  Every member's J, labels, results and progress events equal the oracle's."""
    hjbdp, _abi, c_oracle = env
    from test_gpu_batch import _batch, _job
    for n_st, members in vr.batch_members(_abi, c_oracle, name):
        jobs = [_job(term=term, progress=True) for _, term, _ in members]
        with contextlib.ExitStack() as stack:
            bks = [stack.enter_context(hjbdp.Backup(sp)) for sp, _, _ in members]
            for bk in bks:
                bk.set_option("variant", variant)
                assert bk.info()["kernel_variant"] == variant
            assert len({_snap(bk) for bk in bks}) == 1
            st, outs = _batch(env, bks, jobs, n_st, period=1)
            assert st == _abi.HJB_OK, bks[0].lib.hjb_last_error(bks[0]._h)
        for i, (o, (_, _, ref)) in enumerate(zip(outs, members)):
            _same_bits(o["J"], ref["J"], (name, n_st, "member %d" % i))
            assert np.array_equal(o["idx"], ref["idx"]), (name, n_st, i)
            _same_events(o["events"], ref["events"], (name, n_st, i))
            assert o["stages_done"] == ref["stages_done"] == n_st and not o["stopped_early"]


# ---- d. the other readers and writers of stored J --------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["sub", "edge"])
@pytest.mark.parametrize("storage", STORAGES)
def test_fixed_label_stage_against_the_rational_reference(env, storage, regime):
    """K22 (hjb_evaluate_stage) from both sources of cells and weights, on seeded random labels: evaluate_refs.evaluate_ref with
    the exact fma, stored through half_rne for binary16."""
    hjbdp, _abi, _ = env
    from test_gpu_evaluate import _sources
    c = vr.k22_case(storage, regime)
    with hjbdp.Backup(c["spec"]) as bk:
        srcs = _sources(hjbdp, _abi, bk)
        for s in srcs:
            bk.set_option("eval_tables", s)
            got = bk.evaluate_stage(c["terminal"], c["labels"])
            _same_bits(got, c["J"], ("K22", storage, regime, "2^%d" % c["k"], "source %d" % s))
    assert set(srcs) == {0, 1}


@pytest.mark.parametrize("regime", ["sub", "edge"])
@pytest.mark.parametrize("mode", ["expect", "worst"])
@pytest.mark.parametrize("kernel", list(vr.K24_TYPINGS))
def test_disturbed_stage_against_the_restatement(env, kernel, mode, regime):
    """K24 (stage_disturb_<kernel>) in the expectation and worst-case modes: J as raw bits and labels against
    disturbance_refs.DisturbedRef."""
    hjbdp, _abi, _ = env
    c = vr.k24_case(kernel, mode, regime)
    with hjbdp.Backup(c["spec"]) as bk:
        bk.set_disturbance(c["offsets"], c["weights"], mode)
        assert bk.info()["kernel_variant"] == 8 and bk.get_option("dist_nodes") == c["offsets"].shape[1]
        J, idx = bk.backup_stage(c["terminal"])
    _same_bits(J, c["J"], ("K24", kernel, mode, regime, "2^%d" % c["k"]))
    assert idx.dtype == c["labels"].dtype and np.array_equal(idx, c["labels"]), (kernel, mode, regime)


@pytest.mark.parametrize("regime", ["sub", "edge"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_linear_lookup_of_a_subnormal_value_table(env, dt, regime):
    """hjb_policy_lookup 'linear' on a table of subnormal values: scipy's RegularGridInterpolator in float64 to linear_tol with the
    value scale max(max|V|, the smallest normal) - and the C twin's lookup bit for bit."""
    hjbdp, _abi, c_oracle = env
    from float64_refs import linear_ref
    knots, V, pts = vr.lookup_case(dt, regime)
    got = hjbdp.policy_lookup(knots, V, pts, "linear")
    assert got.dtype == V.dtype and got.shape == (len(pts),)
    ref, w = linear_ref(knots, V, pts)
    err = np.abs(got.astype(np.float64) - ref)
    tol = vr.lookup_tol(V.dtype, 3, V, w)
    print("\n[value range] lookup %s %s: max err / tol %.3g" % (dt, regime, np.max(err / tol)))
    assert np.all(err <= tol), (dt, regime, np.max(err / tol))
    _same_bits(got, c_oracle.lookup(_abi, knots, V, pts, "linear"), ("lookup", dt, regime))
