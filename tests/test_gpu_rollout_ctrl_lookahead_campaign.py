"""GPU tests of the control-lookahead campaign (hjb_rollout_run_control_lookahead_campaign,
csrc/kernels_rollout_ctrl_lookahead_campaign.h: K36; hjbdp.ControlLookaheadRollout.run_control_lookahead_campaign,
Dynamic_Solver.get_actuator_lookahead_cost_statistics): the statistics bit-equal to the existing host reduce
(hjbdp.campaign_reduce) of hjb_rollout_run_control_lookahead's own outputs at every instantiation and block shape, with options
"chunk" and "lds" varied; on the exactly posed lattice the campaign against the stored labels' actuator campaign (K34) on common
random numbers and "promised equals paid"; the refusals, as K29's campaign test has them."""
import ctypes as C

import numpy as np
import pytest

import actuator_rollout_refs as arefs
import campaign_refs as crefs
import control_lookahead_rollout_refs as refs
from test_gpu_rollout_ctrl_lookahead import _open

pytestmark = pytest.mark.gpu

PLANES = refs.PLANES
N_STARTS = 5
SENT = -12345.678


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _flown(ro, knots, X0, M, seed, first):
    """run_control_lookahead(actuator=True)'s per-trajectory outputs for every start repeated M times, plus the left flags"""
    out = ro.run_control_lookahead(np.repeat(X0, M, axis=1), PLANES, actuator=True, seed=seed, first_stream=first, keep_path=True)
    out["left"] = crefs.left_flags(out["X_path"], knots)
    return out


def _same_stats(got, want, what):
    assert got["stats"].shape == want["stats"].shape, what
    assert np.array_equal(bits(got["stats"]), bits(want["stats"])), (what, got["stats"], want["stats"])
    for key in ("mean", "var", "std", "min", "max", "n_exceed", "n_left", "n_settled", "mean_settled"):
        assert np.array_equal(got[key], want[key], equal_nan=True), (what, key)


# ---- 1. every instantiation and block shape ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_every_instantiation_is_bit_equal_to_the_reduced_k35_run(built, D, dtype):
    """n_samples 1 and 3 (G = 1 and 4, one padding slot), 64 (one full block), 65 (a second block of one), 200 (four blocks, the
    last partial); streams first_stream + s * M + m"""
    import hjbdp
    pb = refs.problem(D, dtype, salt=3)
    knots = pb["model"]["knots"]
    X0 = pb["X0"][:, [0, 1, 30, 50, 69]]                   # both corners, an inner start, two starts outside the grid
    assert X0.shape[1] == N_STARTS
    seed, first = pb["seed"], pb["first"]
    left_total = 0
    with _open(pb) as ro:
        for M, lds, chunk in ((1, 1, 1 << 20), (3, 0, 1 << 20), (64, 1, 128), (65, 0, 64), (200, 1, 192), (200, 0, 1 << 20)):
            ro.set_option("lds", 1)
            ro.set_option("chunk", 1 << 20)
            flown = _flown(ro, knots, X0, M, seed, first)
            # a threshold and a tolerance taken from the flight itself, so that slots 4, 6 and 7 are neither empty nor full
            bounds = (float(np.median(flown["cost"])), np.abs(flown["X_final"]).mean(axis=1))
            ro.set_option("lds", lds)
            ro.set_option("chunk", chunk)
            for thr, tol in ((None, None), bounds):
                got = ro.run_control_lookahead_campaign(X0, PLANES, M, seed=seed, first_stream=first, cost_threshold=thr, settle_tol=tol)
                want = hjbdp.campaign_reduce(flown["cost"], M, X_final=flown["X_final"], left=flown["left"], cost_threshold=thr, settle_tol=tol)
                _same_stats(got, want, (M, lds, chunk, thr is not None))
            c2 = flown["cost"].reshape(N_STARTS, M)
            assert np.array_equal(got["min"], c2.min(axis=1)) and np.array_equal(got["max"], c2.max(axis=1))
            assert got["n_left"].max() <= M and (M == 1 or 0 < got["n_exceed"].sum() < N_STARTS * M)
            left_total += int(got["n_left"].sum())
        other = ro.run_control_lookahead_campaign(X0, PLANES, 200, seed=seed + 1, first_stream=first)
        assert not np.array_equal(other["stats"][:, 0], got["stats"][:, 0])
    assert left_total > 0                                  # trajectories did leave the grid


# ---- 2. the lattice: common random numbers with the label campaign, promised equals paid -------------------------------------------------
LATTICE_M, LATTICE_SEED = 1 << 12, 2036


@pytest.mark.parametrize("mode", ["expect", "worst"])
def test_lattice_campaign_is_the_label_campaign_and_pays_what_was_promised(built, mode):
    import hjbdp
    K = arefs.LATTICE_STAGES
    spec = arefs.lattice_spec(mode)
    with hjbdp.Backup(spec) as bk:
        sol = bk.solve(K, keep_J=True, keep_idx=True)
    J = sol["J_stages"].reshape(33, K, order="F")
    idx = sol["idx_stages"].reshape(33, K, order="F")
    off, weights, _ = spec.control_disturbance
    starts = (arefs.LATTICE_STARTS + 16).astype(np.int64)
    promised = J[starts, 0]
    costs, prob, _ = arefs.lattice_enumeration(idx)                             # exact, from the 3^6 sequences: never from the run
    M = LATTICE_M
    X0 = arefs.LATTICE_STARTS.reshape(1, -1)
    with hjbdp.ControlLookaheadRollout([arefs.LATTICE_KNOTS], idx, arefs.LATTICE_U, index_base=0) as ro:
        ro.set_model([[1.0]], [[1.0]], q=[1.0], r=[arefs.LATTICE_R])
        ro.set_values(J)
        ro.set_control_lookahead(off, weights, mode)
        ro.set_actuator_noise(arefs.LATTICE_EPS, weights)
        thr = promised if mode == "worst" else None
        look = ro.run_control_lookahead_campaign(X0, list(range(1, K)) + [-1], M, seed=LATTICE_SEED, cost_threshold=thr)
        stored = ro.run_actuator_campaign(X0, np.arange(K), M, seed=LATTICE_SEED, method="nearest", cost_threshold=thr)
    _same_stats(look, stored, mode)                                             # common random numbers: the same flights
    assert not look["n_left"].any()                                             # every flown state stays within |x| <= 4
    if mode == "worst":
        assert np.array_equal(costs.max(axis=1), promised)
        # the seed's own draws do contain a worst sequence for every start (checked here from the sampler's host twin, no device)
        drawn = hjbdp.noise_draw(hjbdp.noise_thresholds(None, 3), 9 * M, K, seed=LATTICE_SEED).reshape(9, M, K)
        seq = (drawn * 3 ** np.arange(K - 1, -1, -1)).sum(axis=2)              # itertools.product's order: the first step slowest
        assert np.array_equal(np.take_along_axis(costs, seq, axis=1).max(axis=1), promised)
        assert np.array_equal(look["max"], promised) and not look["n_exceed"].any()
    else:
        mean = costs @ prob
        assert np.array_equal(mean, promised)
        sigma = np.sqrt(((costs - mean[:, None]) ** 2) @ prob)
        err = np.abs(look["mean"] - promised)
        print("promised", promised, "paid", look["mean"], "err / (sigma / sqrt(M))", err / np.where(sigma > 0, sigma / np.sqrt(M), 1.0))
        assert np.all(err <= 6.0 * sigma / np.sqrt(M)), (err, sigma)            # equality where sigma = 0 (x = 0)


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_device(built):
    import hjbdp
    from hjbdp import _abi
    pb = refs.problem(3, np.float64, salt=3)
    m = pb["model"]
    ns, M = N_STARTS, 6
    X0 = pb["X0"][:, :ns]
    vplanes = np.array([1, 0, -1, 1], dtype=np.int32)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    Xc = np.ascontiguousarray(X0.T)

    def raw(ro, **call):
        """hjb_rollout_run_control_lookahead_campaign through ctypes on sentinel-filled outputs -> (status, outputs untouched, the text)"""
        stats = np.full(ns * 8, SENT)
        ms = C.c_double(SENT)
        st = ro.lib.hjb_rollout_run_control_lookahead_campaign(ro._ro, call.get("K", len(vplanes)), call.get("pl", ip(vplanes)),
                                                               call.get("ns", ns), call.get("M", M), call.get("X", dp(Xc)), 4,
                                                               call.get("first", 0), call.get("thr", None), call.get("tol", None),
                                                               call.get("stats", dp(stats)), C.byref(ms))
        return st, bool(np.all(stats == SENT) and ms.value == SENT), ro.lib.hjb_rollout_last_error(ro._ro).decode()

    def refused(ro, text, **call):
        st, untouched, err = raw(ro, **call)
        assert st == _abi.HJB_E_INVALID and untouched and text in err, (call, st, untouched, err)

    with hjbdp.ControlLookaheadRollout(m["knots"], refs.labels_stub(m["knots"], pb["nl"], 1), m["u_table"], index_base=1) as ro:
        refused(ro, "before hjb_rollout_set_model")
        ro.set_model(m["A"], m["B"], c=m["c"], q=m["q"], r=m["r"])
        refused(ro, "before hjb_rollout_set_values")
        st, untouched, err = raw(ro, pl=ip(np.full(4, -1, dtype=np.int32)))     # only -1 needs no values, but the sets are still missing
        assert st == _abi.HJB_E_INVALID and untouched and "before hjb_rollout_set_control_lookahead" in err
        ro.set_values(m["J"])
        ro.set_lookahead(np.zeros((3, 1)))                                      # hjb_rollout_set_lookahead's set is not this call's
        ro.set_noise(np.full((3, 2), 0.01))                                     # ... nor hjb_rollout_set_noise's its plant
        refused(ro, "before hjb_rollout_set_control_lookahead")
        ro.set_control_lookahead(pb["E"], pb["P"], pb["mode"])
        refused(ro, "before hjb_rollout_set_actuator_noise")
        ro.set_actuator_noise(pb["eps"], pb["Pf"], pb["base"])
        good = ro.run_control_lookahead_campaign(X0, vplanes, M, seed=4, cost_threshold=0.5, settle_tol=0.4)
        Xn = Xc.copy()
        Xn[3, 2] = np.inf
        thr, tol = np.full(ns, 0.5), np.full(3, 0.4)
        bad_thr, bad_tol, neg_tol = thr.copy(), tol.copy(), tol.copy()
        bad_thr[4], bad_tol[1], neg_tol[2] = np.nan, np.nan, -0.1
        for call, text in ((dict(first=-1), "first_stream=-1 < 0"), (dict(first=2 ** 63 - 10), "overflows"), (dict(M=0), "n_samples=0 < 1"),
                           (dict(M=2 ** 62), "n_starts * n_samples overflows"), (dict(K=-1), "n_steps=-1"), (dict(ns=-2), "n_traj=-2"),
                           (dict(pl=ip(np.array([0, 3, 0, 0], dtype=np.int32))), "value_plane_of_step[1] = 3 outside [-1, 3)"),
                           (dict(pl=ip(np.array([0, 0, -2, 0], dtype=np.int32))), "value_plane_of_step[2] = -2 outside [-1, 3)"),
                           (dict(pl=None), "null value_plane_of_step"), (dict(X=dp(Xn)), "not finite"), (dict(X=None), "null X0"),
                           (dict(thr=dp(bad_thr)), "threshold[4] is NaN"), (dict(tol=dp(bad_tol)), "tol[1]"),
                           (dict(tol=dp(neg_tol)), "tol[2]"), (dict(stats=None), "null stats")):
            refused(ro, text, **call)
        st, untouched, _ = raw(ro, ns=0)                                        # no starts: no work
        assert st == _abi.HJB_OK
        none = ro.run_control_lookahead_campaign(np.zeros((3, 0)), vplanes, M)
        assert none["stats"].shape == (0, 8) and none["device_ms"] == 0.0
        again = ro.run_control_lookahead_campaign(X0, vplanes, M, seed=4, cost_threshold=0.5, settle_tol=0.4)
        assert np.array_equal(bits(again["stats"]), bits(good["stats"])) and again["device_ms"] > 0
    assert hjbdp.load_library().hjb_rollout_run_control_lookahead_campaign(None, 0, None, 0, 1, None, 0, 0, None, None, None,
                                                                           None) == _abi.HJB_E_INVALID
    knots6 = [np.linspace(-1, 1, 3)] * 6                                        # a model other than the affine one
    rng = np.random.default_rng(364)
    with hjbdp.ControlLookaheadRollout(knots6, rng.integers(1, 4, size=(3 ** 6, 1)).astype(np.uint8), rng.uniform(-1, 1, size=(3, 3)),
                                       index_base=1) as ro:
        ro.set_attitude_model([1.0, 2.0, 3.0], 0.01)
        ro.set_values(np.zeros((3 ** 6, 1)))
        ro.set_control_lookahead(np.zeros((6, 1, 3)))
        ro.set_actuator_noise([0.1, -0.1])
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_control_lookahead_campaign(np.zeros((6, 4)), [0, -1], 3)
        assert ei.value.status == _abi.HJB_E_INVALID and "needs the affine model" in str(ei.value)
