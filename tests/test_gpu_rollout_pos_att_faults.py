"""GPU tests of the pos-att fault campaign (hjb_rollout_set_pos_att_fault_controller / hjb_rollout_run_pos_att_faults, K23
csrc/kernels_rollout_pos_att_faults.h; hjbdp.Rollout.run_pos_att_faults, Solver_pos_att.get_fault_campaign): no fault equals K18,
a hand-over at stage 0 equals K18 on the swapped object, the general case equals tests/pos_att_fault_rollout_refs.py bit for bit
at every instantiation, chunking, optional outputs, starts that overflow, the policies simplified_run leaves, the lifetime of the
attached object and every refusal.  The channel and start generators are the K18 test's."""
import ctypes as C

import numpy as np
import pytest

import pos_att_fault_rollout_refs as fr
from test_gpu_rollout_pos_att import INERTIA, MASS, T_DIST, _channels, _diff, _orbit, _same, _starts, _Three

pytestmark = pytest.mark.gpu

KEYS = ("X_final", "X_path", "F_path", "FM_path")
ALL = KEYS + ("impulse", "settle_stage")
SENT = -12345.678
H, K = 0.01, 48


def _eq(a, b, key):
    if key == "settle_stage":
        return a.dtype == np.int32 and np.array_equal(a, b)
    return _same(a, b)


def _check(out, ref, keys=ALL):
    for key in keys:
        assert out[key] is not None and _eq(out[key], ref[key], key), (key, _diff(out[key], ref[key]) if key != "settle_stage" else (out[key], ref[key]))


def _fault_channel(rng, dtype, n_labels, n_planes=3):
    """the fault controller of channel x on a grid of its own: other extents and fewer knots (3 .. 5 an axis) than channel x's"""
    from hjbdp.matlab_compat import sym_linspace_pos_att
    knots = [sym_linspace_pos_att(-0.25, 0.25, int(rng.integers(3, 5))), sym_linspace_pos_att(-0.12, 0.12, int(rng.integers(3, 5))),
             sym_linspace_pos_att(-0.11, 0.11, 3), sym_linspace_pos_att(-0.04, 0.04, int(rng.integers(3, 5)))]
    nS = int(np.prod([len(k) for k in knots]))
    base = int(rng.integers(0, 2))
    labels = rng.integers(base, base + n_labels, size=(nS, n_planes)).astype(dtype)
    ut = rng.choice([0.0, 0.11, -0.11], size=(n_labels, 4)) * rng.uniform(0.5, 1.0, size=(n_labels, 4))
    return knots, labels, ut, base


def _campaign(rng, n, n_steps=K):
    """masks random 12-bit words, a third of them zero; fault and hand-over stages uniform in [0, n_steps + 8] per lane (some never
    come, waves diverge); lanes 64 .. 127 share one pair of stages (one wave with a uniform branch)"""
    mask = rng.integers(1, 4096, size=n).astype(np.int32)
    mask[rng.random(n) < 1 / 3] = 0
    f_at = rng.integers(0, n_steps + 9, size=n).astype(np.int32)
    s_at = rng.integers(0, n_steps + 9, size=n).astype(np.int32)
    f_at[64:128] = 7
    s_at[64:128] = 19
    return mask, f_at, s_at


def _tolerances(tw):
    """percentiles of the twin's own path norms: about half the states outside in position, a fifth in attitude"""
    pn = np.sqrt((tw["X_path"][:, 0:3] ** 2).sum(axis=1))
    an = np.sqrt((tw["X_path"][:, 6:9] ** 2).sum(axis=1))
    return float(np.percentile(pn[np.isfinite(pn)], 50)), float(np.percentile(an[np.isfinite(an)], 80))


class _Four(_Three):
    """channels x, y, z and the fault controller as four hjbdp.Rollout objects"""


def _raw(ro, X0, planes, mask=None, f_at=None, s_at=None, pos_tol=np.inf, att_tol=np.inf,
         want=("impulse", "settle_stage", "X_path", "F_path", "FM_path", "device_ms")):
    """hjb_rollout_run_pos_att_faults through ctypes with every output pre-filled with a sentinel and only `want` passed"""
    X = np.ascontiguousarray(np.asarray(X0, dtype=np.float64).reshape(13, -1).T)
    nt = X.shape[0]
    ps = np.ascontiguousarray(np.asarray(planes).reshape(-1).astype(np.int32))
    n = int(ps.size)
    out = {"X_final": np.full((nt, 13), SENT), "impulse": np.full(nt, SENT), "settle_stage": np.full(nt, -77, np.int32),
           "X_path": np.full(nt * 13 * (n + 1), SENT), "F_path": np.full(nt * 12 * n, SENT), "FM_path": np.full(nt * 6 * n, SENT)}
    ms = C.c_double(-1.0)
    f64 = lambda key: out[key].ctypes.data_as(C.POINTER(C.c_double)) if (key in want or key == "X_final") else None
    i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    ins = [None if a is None else np.ascontiguousarray(np.asarray(a).reshape(-1).astype(np.int32)) for a in (mask, f_at, s_at)]
    st = ro.lib.hjb_rollout_run_pos_att_faults(ro._ro, n, i32(ps), nt, X.ctypes.data_as(C.POINTER(C.c_double)), i32(ins[0]), i32(ins[1]),
                                               i32(ins[2]), float(pos_tol), float(att_tol), f64("X_final"), f64("impulse"),
                                               i32(out["settle_stage"]) if "settle_stage" in want else None, f64("X_path"),
                                               f64("F_path"), f64("FM_path"), C.byref(ms) if "device_ms" in want else None)
    out["device_ms"] = ms.value
    shaped = dict(out)
    shaped["X_final"] = out["X_final"].T
    for key, rows, cols in (("X_path", 13, n + 1), ("F_path", 12, n), ("FM_path", 6, n)):
        shaped[key] = out[key].reshape((nt, rows, cols), order="F")
    return st, shaped


def _untouched(out):
    return all((out[k] == SENT).all() for k in KEYS + ("impulse",)) and (out["settle_stage"] == -77).all() and out["device_ms"] == -1.0


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_no_fault_equals_the_pos_att_kernel(built, dtype):
    """all three arrays NULL, then a fault controller attached and every hand-over at or after n_steps: X_final and the paths are
    hjb_rollout_run_pos_att's on the same objects, bit for bit (LDS and global form, substeps 1 and 3)"""
    rng = np.random.default_rng(2300 + np.dtype(dtype).itemsize)
    chans = _channels(rng, dtype, 40)
    fault = _fault_channel(rng, dtype, 25)
    X0 = _starts(rng, 257)
    planes = rng.integers(0, 3, size=K)
    never = rng.integers(K, K + 20, size=257)
    with _Four(chans + [fault]) as (rx, ry, rz, rf):
        for S in (1, 3):
            rsw, coef = _orbit(K, H, S)
            for lds in (1, 0):
                rx.set_option("lds", lds)
                rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, H, rsw, coef, S)
                ref = rx.run_pos_att(X0, planes, keep_path=True)
                assert np.isfinite(ref["X_final"]).all()
                _check(rx.run_pos_att_faults(X0, planes, keep_path=True), ref, KEYS)
                rx.set_pos_att_fault_controller(rf)
                _check(rx.run_pos_att_faults(X0, planes, switch_stage=never, keep_path=True), ref, KEYS)
                _check(rx.run_pos_att_faults(X0, planes, fault_mask=0xFFF, fault_stage=never, switch_stage=never, keep_path=True), ref, KEYS)
                _check(rx.run_pos_att(X0, planes, keep_path=True), ref, KEYS)          # K18 ignores the attachment
        rx.set_option("lds", 1)


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_hand_over_at_stage_0_equals_the_swapped_object(built, dtype):
    """switch_stage = 0 and no fault: everything equals hjb_rollout_run_pos_att with the fault controller's object (a grid of its
    own, other knot counts) in channel x's place"""
    rng = np.random.default_rng(2310 + np.dtype(dtype).itemsize)
    chans = _channels(rng, dtype, 40)
    fault = _fault_channel(rng, dtype, 25)
    assert [len(k) for k in fault[0]] != [len(k) for k in chans[0][0]]
    X0 = _starts(rng, 257)
    planes = rng.integers(0, 3, size=K)
    with _Four(chans + [fault]) as (rx, ry, rz, rf), _Three([fault]) as (sx,):
        for S, lds in ((1, 1), (3, 0)):
            rsw, coef = _orbit(K, H, S)
            model = (INERTIA, MASS, T_DIST, H, rsw, coef, S)
            rx.set_option("lds", lds)
            sx.set_option("lds", lds)
            rx.set_pos_att_model(ry, rz, *model)
            rx.set_pos_att_fault_controller(rf)
            sx.set_pos_att_model(ry, rz, *model)
            ref = sx.run_pos_att(X0, planes, keep_path=True)
            assert not _same(ref["F_path"], rx.run_pos_att(X0, planes, keep_path=True)["F_path"])
            _check(rx.run_pos_att_faults(X0, planes, switch_stage=0, keep_path=True), ref, KEYS)
            _check(rx.run_pos_att_faults(X0, planes, fault_mask=0, fault_stage=0, switch_stage=np.zeros(257, int), keep_path=True), ref, KEYS)


@pytest.fixture(scope="module")
def general(built):
    """the general case's inputs and the twin's answer per label type, computed once; the seed is chosen so that the TWIN alone
    meets the conditions below (the comparison with the kernel cannot pass empty)"""
    cases = {}
    for dtype in (np.uint8, np.uint16, np.int32):
        rng = np.random.default_rng(2320 + np.dtype(dtype).itemsize)
        chans = _channels(rng, dtype, 40)
        fault = _fault_channel(rng, dtype, 25)
        X0 = _starts(rng, 257)
        planes = rng.integers(0, 3, size=K)
        mask, f_at, s_at = _campaign(rng, 257)
        per_S = {}
        for S in (1, 3):
            rsw, coef = _orbit(K, H, S)
            probe = fr.rollout(chans, fault, INERTIA, MASS, T_DIST, H, S, rsw, coef, X0, planes, mask, f_at, s_at)
            pos_tol, att_tol = _tolerances(probe)
            tw = fr.rollout(chans, fault, INERTIA, MASS, T_DIST, H, S, rsw, coef, X0, planes, mask, f_at, s_at, pos_tol, att_tol)
            faulted = (mask != 0) & (f_at < K)
            hit = (tw["F_cmd"] != tw["F_path"]).any(axis=(1, 2))
            assert faulted.sum() >= 64 and hit[faulted].sum() * 2 >= faulted.sum(), (faulted.sum(), hit[faulted].sum())
            assert not hit[~faulted].any()
            switched = s_at < K
            other = (tw["Fx_nominal"] != tw["F_cmd"][:, [0, 1, 6, 7]]).any(axis=(1, 2))
            assert switched.sum() >= 64 and other[switched].sum() * 4 >= switched.sum(), (switched.sum(), other[switched].sum())
            assert not other[~switched].any()
            vals = set(tw["settle_stage"].tolist())
            assert len(vals) >= 3 and K + 1 in vals and any(1 <= v <= K for v in vals), sorted(vals)
            per_S[S] = (rsw, coef, pos_tol, att_tol, tw)
        cases[np.dtype(dtype).name] = (chans, fault, X0, planes, mask, f_at, s_at, per_S)
    return cases


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_general_case_equals_the_twin_at_every_instantiation(general, dtype):
    """257 starts (two blocks, the second partial), then 255 and 1; random masks, per-lane fault and hand-over stages, one wave
    with a uniform branch; LDS and global form, substeps 1 and 3: X_final, the three paths and impulse as bits, settle_stage as
    integers"""
    chans, fault, X0, planes, mask, f_at, s_at, per_S = general[np.dtype(dtype).name]
    with _Four(chans + [fault]) as (rx, ry, rz, rf):
        for S in (1, 3):
            rsw, coef, pos_tol, att_tol, tw = per_S[S]
            for lds in (1, 0):
                rx.set_option("lds", lds)
                rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, H, rsw, coef, S)
                rx.set_pos_att_fault_controller(rf)
                out = rx.run_pos_att_faults(X0, planes, mask, f_at, s_at, pos_tol, att_tol, keep_path=True)
                _check(out, tw)
                assert out["device_ms"] > 0
                for n in (255, 1):
                    part = rx.run_pos_att_faults(X0[:, :n], planes, mask[:n], f_at[:n], s_at[:n], pos_tol, att_tol, keep_path=True)
                    _check(part, {k: (tw[k][:, :n] if k == "X_final" else tw[k][:n]) for k in ALL})


def test_chunking_and_optional_outputs(general):
    """chunk = 100 with 257 starts: every output equals the unchunked call (a per-trajectory array without its chunk offset shows
    here); each optional output asked for on its own equals the full call; device_ms > 0 when asked for"""
    chans, fault, X0, planes, mask, f_at, s_at, per_S = general["uint16"]
    rsw, coef, pos_tol, att_tol, tw = per_S[1]
    with _Four(chans + [fault]) as (rx, ry, rz, rf):
        rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, H, rsw, coef, 1)
        rx.set_pos_att_fault_controller(rf)
        rx.set_option("chunk", 100)
        _check(rx.run_pos_att_faults(X0, planes, mask, f_at, s_at, pos_tol, att_tol, keep_path=True), tw)
        lean = rx.run_pos_att_faults(X0, planes, mask, f_at, s_at, pos_tol, att_tol)
        _check(lean, tw, ("X_final", "impulse", "settle_stage"))
        assert lean["X_path"] is None and lean["F_path"] is None and lean["FM_path"] is None
        for chunk in (100, 1 << 20):
            rx.set_option("chunk", chunk)
            st, full = _raw(rx, X0, planes, mask, f_at, s_at, pos_tol, att_tol)
            assert st == 0 and full["device_ms"] > 0
            _check(full, tw)
            for key in ("impulse", "settle_stage", "X_path", "F_path", "FM_path", "device_ms"):
                st, one = _raw(rx, X0, planes, mask, f_at, s_at, pos_tol, att_tol, want=(key,))
                assert st == 0, key
                _check(one, tw, ("X_final",) + ((key,) if key != "device_ms" else ()))
                for other in ("impulse", "X_path", "F_path", "FM_path"):
                    assert other == key or (one[other] == SENT).all(), (key, other)
                assert key == "settle_stage" or (one["settle_stage"] == -77).all(), key
                assert (one["device_ms"] > 0) if key == "device_ms" else (one["device_ms"] == -1.0), key
        st, none = _raw(rx, X0[:, :0], planes)
        assert st == 0 and none["device_ms"] == 0.0


def test_omitted_per_trajectory_inputs_chunked(general):
    """chunk = 100 with 257 starts and fault_mask, fault_stage and switch_stage omitted (NULL) one at a time, then all three: every
    output equals the same call unchunked (a NULL array skipped at the wrong place among the per-trajectory inputs shows here and
    nowhere else); each single omission flies another campaign than the general case; with all three omitted X_final is
    hjb_rollout_run_pos_att's"""
    chans, fault, X0, planes, mask, f_at, s_at, per_S = general["uint16"]
    rsw, coef, pos_tol, att_tol, tw = per_S[1]
    given = {"fault_mask": mask, "fault_stage": f_at, "switch_stage": s_at}
    with _Four(chans + [fault]) as (rx, ry, rz, rf):
        rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, H, rsw, coef, 1)
        rx.set_pos_att_fault_controller(rf)
        for omit in (("fault_mask",), ("fault_stage",), ("switch_stage",), tuple(given)):
            kw = {k: v for k, v in given.items() if k not in omit}
            rx.set_option("chunk", 1 << 20)
            whole = rx.run_pos_att_faults(X0, planes, pos_tol=pos_tol, att_tol=att_tol, keep_path=True, **kw)
            assert not _same(whole["F_path"], tw["F_path"]), omit
            rx.set_option("chunk", 100)
            _check(rx.run_pos_att_faults(X0, planes, pos_tol=pos_tol, att_tol=att_tol, keep_path=True, **kw), whole)
        assert _same(whole["X_final"], rx.run_pos_att(X0, planes)["X_final"])


def test_starts_that_overflow_during_the_run(built):
    """the K18 test's overflowing starts (position 1e300, rate 1e200, ...) with faults and hand-overs: the run completes, equals
    the twin (NaN = NaN) and reports the overflowed starts as never settled"""
    rng = np.random.default_rng(2330)
    chans = _channels(rng, np.uint8, 25)
    fault = _fault_channel(rng, np.uint8, 20)
    X0 = _starts(rng, 256)
    X0[0, 3] = 1e300
    X0[1, 4] = -1e300
    X0[10:13, 5] = [1e200, -1e200, 1e200]
    X0[3, 6] = 1e308
    X0[6, 7] = 5.0
    n_steps, S = 12, 1
    planes = rng.integers(0, 3, size=n_steps)
    mask, f_at, s_at = _campaign(rng, 256, n_steps)
    f_at[3:8] = [0, 2, 1, 0, 3]
    s_at[3:8] = [1, 0, 2, 5, 0]
    mask[3:8] = [0x3, 0xFFF, 0x41, 0x800, 0x1]
    rsw, coef = _orbit(n_steps, H, S)
    pos_tol, att_tol = 0.3, 0.1
    tw = fr.rollout(chans, fault, INERTIA, MASS, T_DIST, H, S, rsw, coef, X0, planes, mask, f_at, s_at, pos_tol, att_tol)
    with _Four(chans + [fault]) as (rx, ry, rz, rf):
        rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, H, rsw, coef, S)
        rx.set_pos_att_fault_controller(rf)
        out = rx.run_pos_att_faults(X0, planes, mask, f_at, s_at, pos_tol, att_tol, keep_path=True)
    _check(out, tw)
    assert not np.isfinite(out["X_final"][:, 5]).all()
    assert (out["settle_stage"][3:8] == n_steps + 1).all(), out["settle_stage"][3:8]
    keep = np.delete(np.arange(256), [3, 4, 5, 6, 7])
    assert np.isfinite(out["X_final"][:, keep]).all() and np.isfinite(out["impulse"]).all()


@pytest.fixture(scope="module")
def pos_att_solver(built):
    import hjbdp
    pa = hjbdp.Solver_pos_att()
    pa.simplified_run()
    return pa


def test_reference_policies(pos_att_solver):
    """the policies simplified_run leaves: 257 starts around the default X0, thruster 0 dead from stage 200, hand-over at 200, at
    400 and never, 600 stages with paths: the twin for all starts, pos_att_fault_path_fixed for the default start and three more,
    get_fault_campaign against the raw calls, and the all-failure-controller run against get_optimal_paths"""
    import hjbdp
    from hjbdp.rollout import pos_att_channels, pos_att_default_X0, pos_att_fault_path_fixed, pos_att_orbit_table
    pa = pos_att_solver
    rng = np.random.default_rng(23)
    n, N = 257, 600
    X0 = np.tile(pos_att_default_X0().reshape(13, 1), (1, n))
    X0[0:3, 1:] += rng.uniform(-0.05, 0.05, size=(3, n - 1))
    X0[3:6, 1:] += rng.uniform(-0.02, 0.02, size=(3, n - 1))
    ang = 2 * np.arcsin(X0[6:9, 1:]) + rng.uniform(-0.03, 0.03, size=(3, n - 1))
    X0[6:9, 1:] = np.sin(ang / 2)
    X0[9, 1:] = np.sqrt(1.0 - (X0[6:9, 1:] ** 2).sum(axis=0))
    X0[10:13, 1:] += rng.uniform(-0.01, 0.01, size=(3, n - 1))
    chans = [(k, l, t, 1) for k, l, t in pos_att_channels(pa)]
    fault = [(k, l, t, 1) for k, l, t in pos_att_channels(pa, "channel_x_controller_1_failure")][0]
    rsw, coef = pos_att_orbit_table(N, pa.h, 1)
    pos_tol, att_tol = 0.08, 0.02
    zeros = np.zeros(N, int)
    ros = [hjbdp.Rollout(k, l, t, index_base=b) for k, l, t, b in chans + [fault]]
    try:
        rx, ry, rz, rf = ros
        rx.set_pos_att_model(ry, rz, pa.InertiaM, pa.Mass, pa.T_dist, pa.h, rsw, coef, 1)
        rx.set_pos_att_fault_controller(rf)
        for s_at in (200, 400, None):
            out = rx.run_pos_att_faults(X0, zeros, 1, 200, s_at, pos_tol, att_tol, keep_path=True)
            tw = fr.rollout(chans, fault, pa.InertiaM, pa.Mass, pa.T_dist, pa.h, 1, rsw, coef, X0, zeros, np.full(n, 1), np.full(n, 200),
                            None if s_at is None else np.full(n, s_at), pos_tol, att_tol)
            _check(out, tw)
            assert not out["F_path"][:, 0, 200:].any() and np.isfinite(out["X_final"]).all()
            for t in range(4):
                T, X, F, FM, imp, settle = pos_att_fault_path_fixed(pa, X0[:, t], 1, 200, s_at, n_steps=N, pos_tol=pos_tol, att_tol=att_tol)
                assert _same(out["X_path"][t].T, X), _diff(out["X_path"][t].T, X)
                assert _same(out["F_path"][t].T, F[:N]) and _same(out["FM_path"][t].T, FM[:N])
                assert _same(out["impulse"][t], imp) and int(out["settle_stage"][t]) == settle
            if s_at == 400:
                camp = pa.get_fault_campaign(X0, fault_mask=1, fault_stage=200, switch_stage=400, n_steps=N, pos_tol=pos_tol,
                                             att_tol=att_tol, keep_path=True)
                _check(camp, out)
                lean = pa.get_fault_campaign(X0, np.full(n, 1), np.full(n, 200), np.full(n, 400), n_steps=N, pos_tol=pos_tol, att_tol=att_tol)
                _check(lean, out, ("X_final", "impulse", "settle_stage"))
                assert lean["X_path"] is None
        # the failure table never commands f0, so masking f0 from stage 0 under the failure controller changes nothing
        assert not np.asarray(pa.controllers["channel_x_controller_1_failure"]["f0_allcomb"]).any()
        allf = rx.run_pos_att_faults(X0, zeros, 1, 0, 0)
        assert _same(allf["X_final"], pa.get_optimal_paths(X0, n_steps=N, channel_x="channel_x_controller_1_failure"))
    finally:
        for ro in ros:
            ro.close()


def test_lifetime_and_non_interference(built):
    import hjbdp
    rng = np.random.default_rng(2340)
    chans = _channels(rng, np.int32, 20)
    fault = _fault_channel(rng, np.int32, 15)
    X0 = _starts(rng, 257)
    planes = rng.integers(0, 3, size=K)
    mask, f_at, s_at = _campaign(rng, 257)
    rsw, coef = _orbit(K, H, 1)
    model = (INERTIA, MASS, T_DIST, H, rsw, coef, 1)
    with _Four(chans + [fault]) as (rx, ry, rz, rf):
        rx.set_pos_att_model(ry, rz, *model)
        k18 = rx.run_pos_att(X0, planes, keep_path=True)
        rx.set_pos_att_fault_controller(rf)
        before = rx.run_pos_att_faults(X0, planes, mask, f_at, s_at, 0.2, 0.05, keep_path=True)
        rf.close()
        other = _fault_channel(rng, np.int32, 15)
        with _Three([other]) as (of,):                          # a fresh allocation where the closed object's would have been freed
            _check(rx.run_pos_att_faults(X0, planes, mask, f_at, s_at, 0.2, 0.05, keep_path=True), before)
        _check(rx.run_pos_att_faults(X0, planes, mask, f_at, s_at, 0.2, 0.05, keep_path=True), before)
        _check(rx.run_pos_att(X0, planes, keep_path=True), k18, KEYS)
        # detaching, and setting the model again, drop the attachment
        rx.set_pos_att_fault_controller(None)
        with pytest.raises(hjbdp.HjbError, match="no fault controller"):
            rx.run_pos_att_faults(X0, planes, switch_stage=K - 1)
        with _Three([fault]) as (rf2,):
            rx.set_pos_att_fault_controller(rf2)
            _check(rx.run_pos_att_faults(X0, planes, mask, f_at, s_at, 0.2, 0.05, keep_path=True), before)
            rx.set_pos_att_model(ry, rz, *model)
            with pytest.raises(hjbdp.HjbError, match="no fault controller"):
                rx.run_pos_att_faults(X0, planes, switch_stage=s_at)
            _check(rx.run_pos_att_faults(X0, planes, switch_stage=K, keep_path=True), k18, KEYS)


def test_refusals(built):
    """each is HJB_E_INVALID with every output still holding its sentinel; a later valid call succeeds"""
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(2350)
    chans = _channels(rng, np.uint8, 12)
    fault = _fault_channel(rng, np.uint8, 10, n_planes=2)       # one plane fewer than the channels
    X0 = _starts(rng, 64)
    n_steps, S = 6, 2
    rsw, coef = _orbit(n_steps, H, S)
    model = (INERTIA, MASS, T_DIST, H, rsw, coef, S)
    ok = [0, 1, 0, 1, 1, 0]
    i64 = lambda v: np.full(64, v)

    def refused(needle, *a, **kw):
        st, out = _raw(rx, *a, **kw)
        msg = rx.lib.hjb_rollout_last_error(rx._ro).decode()
        assert st == _abi.HJB_E_INVALID and needle in msg, (st, needle, msg)
        assert _untouched(out), needle

    def refused_set(fn, *needles):
        with pytest.raises(hjbdp.HjbError) as ei:
            fn()
        assert ei.value.status == _abi.HJB_E_INVALID, str(ei.value)
        for nd in needles:
            assert nd in str(ei.value), (nd, str(ei.value))

    with _Four(chans + [fault]) as (rx, ry, rz, rf):
        refused_set(lambda: rx.set_pos_att_fault_controller(rf), "hjb_rollout_set_pos_att_model")
        refused("hjb_rollout_set_pos_att_model", X0, ok)
        rx.set_pos_att_model(ry, rz, *model)
        refused("no fault controller", X0, ok, None, None, i64(3))                     # a hand-over without an attachment
        st, out = _raw(rx, X0, ok, None, None, i64(n_steps))                           # ... at n_steps it never comes
        assert st == 0
        # what cannot be attached: D = 2, n_u = 1, another label type, the object itself
        k, lab, ut, base = fault
        with hjbdp.Rollout(k[:2], np.ones(len(k[0]) * len(k[1]), np.uint8), np.zeros((1, 4)), index_base=1) as d2:
            refused_set(lambda: rx.set_pos_att_fault_controller(d2), "D == 4", "rollout_xf")
        with hjbdp.Rollout(k, lab, ut[:, :1], index_base=base) as u1:
            refused_set(lambda: rx.set_pos_att_fault_controller(u1), "n_u == 4", "rollout_xf")
        with hjbdp.Rollout(k, lab.astype(np.uint16), ut, index_base=base) as l16:
            refused_set(lambda: rx.set_pos_att_fault_controller(l16), "label")
        refused_set(lambda: rx.set_pos_att_fault_controller(rx), "same object")
        refused("no fault controller", X0, ok, None, None, i64(0))                     # the refused attachments left nothing behind
        rx.set_pos_att_fault_controller(rf)
        refused("fault_mask[5]", X0, ok, np.where(np.arange(64) == 5, 1 << 12, 3))
        refused("fault_mask[0]", X0, ok, i64(-1))
        refused("fault_stage[7]", X0, ok, i64(1), np.where(np.arange(64) == 7, -1, 2))
        refused("switch_stage[63]", X0, ok, None, None, np.where(np.arange(64) == 63, -4, 2))
        for tol in (np.nan, -1e-9, -np.inf):
            refused("pos_tol", X0, ok, pos_tol=tol)
            refused("att_tol", X0, ok, att_tol=tol)
        for bad in (np.nan, np.inf):
            Xn = X0.copy()
            Xn[8, 3] = bad
            refused("not finite", Xn, ok)
        refused("plane_of_step[1] = 2", X0, [0, 2, 0], None, None, i64(9))              # channels have plane 2, the fault controller not
        refused("plane_of_step[0] = 3", X0, [3])
        refused("plane_of_step", X0, [-1])
        refused("orbit table", X0, ok + [0])
        rx.set_pos_att_fault_controller(None)
        st, out = _raw(rx, X0, [0, 2, 0])                                               # without the attachment plane 2 is there
        assert st == 0
        rx.set_pos_att_fault_controller(rf)
        # a later valid call succeeds, and equals the twin
        mask, f_at, s_at = _campaign(rng, 64, n_steps)
        st, out = _raw(rx, X0, ok, mask, f_at, s_at, np.inf, np.inf)
        assert st == 0
        tw = fr.rollout(chans, fault, INERTIA, MASS, T_DIST, H, S, rsw, coef, X0, ok, mask, f_at, s_at)
        _check(out, tw)
        assert (out["settle_stage"] == 0).all()
        # the other run functions refuse a pos-att object as before, and the affine model drops the attachment with the model
        rx.set_model(np.eye(4), np.zeros((4, 4)))
        refused("hjb_rollout_run", X0, ok)
        refused_set(lambda: rx.set_pos_att_fault_controller(rf), "hjb_rollout_set_pos_att_model")
