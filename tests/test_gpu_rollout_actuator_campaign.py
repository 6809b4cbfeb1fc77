"""GPU tests of the actuator-noise campaign (hjb_rollout_run_actuator_campaign, csrc/kernels_rollout_actuator_campaign.h: K34;
hjbdp.ActuatorRollout.run_actuator_campaign, Dynamic_Solver.get_actuator_cost_statistics): the statistics bit-equal to the existing host
reduce (hjbdp.campaign_reduce) of hjb_rollout_run_actuator's own outputs at every instantiation and block shape, chunking, strict
thresholds, "promised equals paid" on the exactly posed lattice problem, validation, and the mirror."""
import ctypes as C

import numpy as np
import pytest

import actuator_rollout_refs as refs
import campaign_refs as crefs
from test_gpu_rollout_campaign import _bits, _problem, _starts

pytestmark = pytest.mark.gpu


def _check_against_run_actuator(ro, knots, X0, planes, M, seed, first, method, thr, tol):
    """run_actuator_campaign's stats against campaign_reduce of run_actuator(np.repeat(X0, M), keep_path=True), the left flags
    from the kept paths.  Returns (stats, the run_actuator output)."""
    import hjbdp
    flown = ro.run_actuator(np.repeat(X0, M, axis=1), planes, seed=seed, first_stream=first, method=method, keep_path=True)
    left = crefs.left_flags(flown["X_path"], knots)
    got = ro.run_actuator_campaign(X0, planes, M, seed=seed, first_stream=first, method=method, cost_threshold=thr, settle_tol=tol)
    via_host = hjbdp.campaign_reduce(flown["cost"], M, X_final=flown["X_final"], left=left, cost_threshold=thr, settle_tol=tol)
    assert got["stats"].shape == (X0.shape[1], 8)
    assert np.array_equal(_bits(got["stats"]), _bits(via_host["stats"])), (M, method, got["stats"], via_host["stats"])
    for key in ("mean", "var", "std", "min", "max", "n_exceed", "n_left", "n_settled", "mean_settled"):
        assert np.array_equal(got[key], via_host[key], equal_nan=True), key
    return got, flown


def _actuator_set(rng, D, nu, W):
    """eps [W, n_u] with a dead input from n_u = 2 on, base [D, W] with an all-zero axis from D = 2 on, weights"""
    eps = rng.uniform(-1.0, 1.0, size=(W, nu))
    if nu > 1:
        eps[:, int(rng.integers(0, nu))] = np.where(rng.integers(0, 2, size=W) == 0, 0.0, -0.0)
    base = rng.uniform(-0.3, 0.3, size=(D, W))
    if D > 1:
        base[int(rng.integers(0, D))] = 0.0
    return eps, base, rng.uniform(0.1, 1.0, size=W)


# ---- 1. every instantiation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_every_instantiation_is_bit_equal_to_the_reduced_actuator_run(built, D, dtype):
    import hjbdp
    rng = np.random.default_rng(3400 + 100 * D + np.dtype(dtype).itemsize)
    nu = 1 + D % 3
    knots, labels, ut, base, A, B, c = _problem(rng, D, nu, dtype)
    if D > 1:
        B[int(rng.integers(0, D)), int(rng.integers(0, nu))] = 0.0              # a term that does not exist
    M, ns = 5, 37                                   # G = 8 with three padding slots; 37 blocks: the last wave part-filled
    X0 = _starts(rng, knots, ns)
    planes = rng.integers(0, 3, size=6)             # the Philox block boundary at k = 4
    eps, nodes, p = _actuator_set(rng, D, nu, 5)
    model = dict(c=c, q=rng.uniform(0, 1, size=D), r=rng.uniform(0, 1, size=nu))
    seed, first = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
    left_total = 0
    with hjbdp.ActuatorRollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, **model)
        ro.set_actuator_noise(eps, p, nodes)
        for method in ("nearest", "linear"):
            flown = ro.run_actuator(np.repeat(X0, M, axis=1), planes, seed=seed, first_stream=first, method=method)
            # a threshold and a tolerance taken from the flight itself, so that slots 4, 6 and 7 are neither empty nor full
            bounds = (np.median(flown["cost"]), np.abs(flown["X_final"]).mean(axis=1))
            for lds in (1, 0):
                ro.set_option("lds", lds)
                for thr, tol in ((None, None), bounds):         # both settings under both forms
                    got, kept = _check_against_run_actuator(ro, knots, X0, planes, M, seed, first, method, thr, tol)
                assert got["n_left"].max() <= M and 0 < got["n_exceed"].sum() < ns * M
            left_total += int(got["n_left"].sum())
        # ... and the flight itself is the restatement's (once per object: test_gpu_rollout_actuator.py covers every form)
        ref = refs.rollout(knots, labels, ut, base, A, B, np.repeat(X0, M, axis=1), planes, eps, p, nodes, seed, first, "linear", **model)
        assert np.array_equal(_bits(kept["cost"]), _bits(ref[1]))
    assert left_total > 0                           # trajectories did leave the grid


# ---- 2. block shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3, 63, 64, 65, 200])
def test_block_shapes(built, M):
    """one block per start (M <= 64: one lane, two, four of which one is padding, 64 with one padding slot, 64 full), two blocks
    with the second almost all padding (65), four blocks (200); with 1, 3 and 70 starts"""
    import hjbdp
    rng = np.random.default_rng(340 + M)
    knots, labels, ut, base, A, B, c = _problem(rng, 2, 2, np.uint16)
    planes = rng.integers(0, 3, size=6)
    eps, nodes, p = _actuator_set(rng, 2, 2, 4)
    with hjbdp.ActuatorRollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=[1.0, 0.5], r=[0.1, 0.2])
        ro.set_actuator_noise(eps, p, nodes)
        for ns in (1, 3, 70):
            X0 = _starts(rng, knots, ns)
            got, flown = _check_against_run_actuator(ro, knots, X0, planes, M, 11 + ns, 1000 * ns, "linear", np.full(ns, 0.4),
                                                     np.array([0.3, 0.3]))
            c2 = flown["cost"].reshape(ns, M)
            assert np.array_equal(got["min"], c2.min(axis=1)) and np.array_equal(got["max"], c2.max(axis=1))


# ---- 3. chunking -------------------------------------------------------------------------------------------------------------------
def test_chunks_and_streams_change_no_bit(built):
    import hjbdp
    rng = np.random.default_rng(343)
    knots, labels, ut, base, A, B, c = _problem(rng, 2, 2, np.uint8)
    planes = rng.integers(0, 3, size=6)
    eps, nodes, p = _actuator_set(rng, 2, 2, 9)
    M = 200
    X0 = _starts(rng, knots, 14)
    with hjbdp.ActuatorRollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=[1.0, 0.5], r=[0.1, 0.2])
        ro.set_actuator_noise(eps, p, nodes)
        kw = dict(seed=12, cost_threshold=0.5, settle_tol=0.3)
        whole, _ = _check_against_run_actuator(ro, knots, X0[:, :7], planes, M, 12, 0, "linear", 0.5, 0.3)
        for chunk in (64, 192, 1 << 20, 1):         # one block a launch; three: a start's four blocks across launches; one launch;
            ro.set_option("chunk", chunk)           # below one block: a launch still takes a whole block
            got = ro.run_actuator_campaign(X0[:, :7], planes, M, **kw)
            assert np.array_equal(_bits(got["stats"]), _bits(whole["stats"])), chunk
        ro.set_option("chunk", 1 << 20)
        for lds in (0, 1):
            ro.set_option("lds", lds)
            assert np.array_equal(_bits(ro.run_actuator_campaign(X0[:, :7], planes, M, **kw)["stats"]), _bits(whole["stats"])), lds
        both = ro.run_actuator_campaign(X0, planes, M, **kw)
        second = ro.run_actuator_campaign(X0[:, 7:], planes, M, first_stream=7 * M, **kw)
        assert np.array_equal(_bits(both["stats"][:7]), _bits(whole["stats"]))
        assert np.array_equal(_bits(both["stats"][7:]), _bits(second["stats"]))
        other = ro.run_actuator_campaign(X0[:, :7], planes, M, seed=13)
        assert not np.array_equal(other["stats"][:, 0], whole["stats"][:, 0])
        assert not other["n_exceed"].any() and not other["n_settled"].any() and not other["stats"][:, 7].any()


# ---- 4. threshold and tol ------------------------------------------------------------------------------------------------------------
def test_threshold_is_strict_and_tolerance_is_not(built):
    import hjbdp
    rng = np.random.default_rng(355)
    knots, labels, ut, base, A, B, c = _problem(rng, 2, 1, np.uint8)
    M, ns = 24, 9
    X0 = _starts(rng, knots, ns) * 0.3
    planes = rng.integers(0, 3, size=6)
    with hjbdp.ActuatorRollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, q=[1.0, 0.5], r=[0.1])
        ro.set_actuator_noise([-0.5, 0.1, 0.7], None, rng.uniform(-0.1, 0.1, size=(2, 3)))
        flown = ro.run_actuator(np.repeat(X0, M, axis=1), planes, seed=8)
        cost, Xf = flown["cost"].reshape(ns, M), flown["X_final"]
        thr = cost[np.arange(ns), np.arange(ns) % M].copy()                 # each start's threshold exactly at one of its samples' costs
        tol = np.abs(Xf[:, 5])                                              # the tolerance exactly at one sample's |xf|
        got = ro.run_actuator_campaign(X0, planes, M, seed=8, cost_threshold=thr, settle_tol=tol)
        settled = (np.abs(Xf) <= tol[:, None]).all(axis=0).reshape(ns, M)
        assert np.array_equal(got["n_exceed"], (cost > thr[:, None]).sum(axis=1))
        assert np.all(got["n_exceed"] < (cost >= thr[:, None]).sum(axis=1))  # the sample at the threshold is not counted
        assert np.array_equal(got["n_settled"], settled.sum(axis=1)) and settled[0, 5] and got["n_settled"].sum() > 1
        want7 = hjbdp.campaign_reduce(flown["cost"], M, X_final=Xf, settle_tol=tol)["stats"][:, 7]
        assert np.array_equal(_bits(got["stats"][:, 7]), _bits(want7))
        plain = ro.run_actuator_campaign(X0, planes, M, seed=8)
        assert not plain["stats"][:, [4, 6, 7]].any() and np.array_equal(_bits(plain["stats"][:, :4]), _bits(got["stats"][:, :4]))


# ---- 5. promised equals paid ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice(built):
    """the lattice problem solved on the GPU under both modes: {mode: (J at stage 1 [33], labels [33, 6])}"""
    import hjbdp
    out = {}
    for mode in ("expect", "worst"):
        with hjbdp.Backup(refs.lattice_spec(mode)) as bk:
            sol = bk.solve(refs.LATTICE_STAGES, keep_J=True, keep_idx=True)
        out[mode] = (sol["J_stages"].reshape(33, refs.LATTICE_STAGES, order="F")[:, 0],
                     sol["idx_stages"].reshape(33, refs.LATTICE_STAGES, order="F"))
    return out


def _lattice_campaign(labels, weights, n_samples, seed, threshold):
    import hjbdp
    with hjbdp.ActuatorRollout([refs.LATTICE_KNOTS], labels, refs.LATTICE_U, index_base=0) as ro:
        ro.set_model([[1.0]], [[1.0]], q=[1.0], r=[refs.LATTICE_R])
        ro.set_actuator_noise(refs.LATTICE_EPS, weights)
        return ro.run_actuator_campaign(refs.LATTICE_STARTS.reshape(1, -1), np.arange(refs.LATTICE_STAGES), n_samples, seed=seed,
                                        cost_threshold=threshold)


def test_expected_cost_promised_is_the_mean_paid(lattice):
    J1, labels = lattice["expect"]
    starts = (refs.LATTICE_STARTS + 16).astype(np.int64)
    costs, prob, _ = refs.lattice_enumeration(labels)
    mean = costs @ prob
    assert np.array_equal(mean, J1[starts])
    sigma = np.sqrt(((costs - mean[:, None]) ** 2) @ prob)                      # exact, from the 3^6 sequences: never from samples
    out = _lattice_campaign(labels, refs.LATTICE_P, 1 << 16, 2033, None)
    err = np.abs(out["mean"] - J1[starts])
    print("promised", J1[starts], "paid", out["mean"], "err / (sigma / 2^8)", err / np.where(sigma > 0, sigma / 256.0, 1.0))
    assert np.all(err <= 6.0 * sigma / 256.0), (err, sigma)                     # equality where sigma = 0 (x = 0)
    assert not out["n_left"].any()                                              # every flown state stays within |x| <= 4


def test_worst_case_promised_is_the_maximum_paid(lattice):
    J1, labels = lattice["worst"]
    starts = (refs.LATTICE_STARTS + 16).astype(np.int64)
    costs, _, _ = refs.lattice_enumeration(labels)
    assert np.array_equal(costs.max(axis=1), J1[starts])
    out = _lattice_campaign(labels, None, 1 << 16, 2034, J1[starts])            # uniform over the three nodes
    assert np.array_equal(out["max"], J1[starts]) and not out["n_exceed"].any() and not out["n_left"].any()
    below = _lattice_campaign(labels, None, 1 << 16, 2034, J1[starts] - 0.5)
    assert np.all(below["n_exceed"] > 0) and np.array_equal(_bits(below["stats"][:, :4]), _bits(out["stats"][:, :4]))


# ---- 6. validation with a device -----------------------------------------------------------------------------------------------------
def test_validation_with_a_device(built):
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(377)
    knots, labels, ut, base, A, B, c = _problem(rng, 3, 2, np.int32, 9, 5)
    ns, M = 11, 6
    X0 = _starts(rng, knots, ns)
    planes = rng.integers(0, 5, size=6)
    eps, nodes, p = _actuator_set(rng, 3, 2, 5)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    with hjbdp.ActuatorRollout(knots, labels, ut, index_base=base) as ro:
        lib, h = ro.lib, ro._ro
        err = lambda: lib.hjb_rollout_last_error(h).decode()
        with pytest.raises(hjbdp.HjbError) as ei:                               # no model yet
            ro.run_actuator_campaign(X0, planes, M)
        assert ei.value.status == _abi.HJB_E_INVALID and "hjb_rollout_set_model" in str(ei.value)
        ro.set_model(A, B, c=c, q=[1, 1, 1])
        ro.set_noise(nodes, p)                                                  # an additive set is not an actuator set
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_actuator_campaign(X0, planes, M)
        assert ei.value.status == _abi.HJB_E_INVALID and "before hjb_rollout_set_actuator_noise" in str(ei.value)
        ro.set_actuator_noise(eps, p, nodes)
        good = ro.run_actuator_campaign(X0, planes, M, seed=4, cost_threshold=0.5, settle_tol=0.4)
        Xc = np.ascontiguousarray(X0.T)
        ps = np.ascontiguousarray(planes, dtype=np.int32)
        pp = ps.ctypes.data_as(C.POINTER(C.c_int32))
        K = len(ps)
        Xn = Xc.copy()
        Xn[7, 2] = np.inf
        far = np.array([0, 5] + [0] * (K - 2), dtype=np.int32)
        thr, tol = np.full(ns, 0.5), np.full(3, 0.4)
        bad_thr, bad_tol, neg_tol = thr.copy(), tol.copy(), tol.copy()
        bad_thr[4], bad_tol[1], neg_tol[2] = np.nan, np.nan, -0.1
        for call, text in ((dict(first=-1), "first_stream=-1 < 0"), (dict(first=2 ** 63 - 10), "overflows"), (dict(M=0), "n_samples=0 < 1"),
                           (dict(M=2 ** 62), "n_starts * n_samples overflows"), (dict(method=7), "method 7"), (dict(K=-1), "n_steps=-1"),
                           (dict(ns=-2), "n_traj=-2"), (dict(pl=far.ctypes.data_as(C.POINTER(C.c_int32))), "plane_of_step[1] = 5"),
                           (dict(pl=None), "null plane_of_step"), (dict(X=dp(Xn)), "not finite"), (dict(X=None), "null X0"),
                           (dict(thr=dp(bad_thr)), "threshold[4] is NaN"), (dict(tol=dp(bad_tol)), "tol[1]"),
                           (dict(tol=dp(neg_tol)), "tol[2]"), (dict(stats=None), "null stats")):
            stats = np.full(ns * 8, 7.25)
            ms = C.c_double(7.25)
            st = lib.hjb_rollout_run_actuator_campaign(h, call.get("method", 1), call.get("K", K), call.get("pl", pp), call.get("ns", ns),
                                                       call.get("M", M), call.get("X", dp(Xc)), 4, call.get("first", 0),
                                                       call.get("thr", dp(thr)), call.get("tol", dp(tol)), call.get("stats", dp(stats)),
                                                       C.byref(ms))
            assert st == _abi.HJB_E_INVALID and text in err(), (call, err())
            assert np.all(stats == 7.25) and ms.value == 7.25, call
        again = ro.run_actuator_campaign(X0, planes, M, seed=4, cost_threshold=0.5, settle_tol=0.4)
        assert np.array_equal(_bits(again["stats"]), _bits(good["stats"])) and again["device_ms"] > 0
        none = ro.run_actuator_campaign(np.zeros((3, 0)), planes, M)            # no starts: no work
        assert none["stats"].shape == (0, 8) and none["device_ms"] == 0.0
    k6, l6, u6, b6, _, _, _ = _problem(rng, 6, 3, np.uint8, 5, 2)               # a model other than the affine one
    with hjbdp.ActuatorRollout(k6, l6, u6, index_base=b6) as ro:
        ro.set_attitude_model([1.0, 2.0, 3.0], 0.01)
        ro.set_actuator_noise([0.1, -0.1])
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_actuator_campaign(np.zeros((6, 4)), [0, 1], 3)
        assert ei.value.status == _abi.HJB_E_INVALID and "attitude model" in str(ei.value)


# ---- 7. the mirror -------------------------------------------------------------------------------------------------------------------
def test_dynamic_solver_actuator_cost_statistics(built):
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N, ds.dx, ds.du = 6, 9, 20
    eps, w = np.array([-0.2, -0.1, 0.0, 0.1, 0.2]), np.array([1.0, 4.0, 6.0, 4.0, 1.0])
    ds.actuator_noise = (eps, w, "expect")
    ds.run()
    M = 64
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    X0s = np.stack([np.tile(s_r, 9), np.repeat(s_r, 9)])                        # node (i, j) at column i + 9 j: axis 0 fastest
    stat = ds.get_actuator_cost_statistics(X0s, M, seed=6, cost_threshold=1.0)
    cost = ds.get_actuator_paths(X0s, M, seed=6)                                # [81, 64], the same streams
    want = hjbdp.campaign_reduce(cost.reshape(-1), M, cost_threshold=1.0)
    for key in ("mean", "var", "std", "min", "max", "n_exceed"):
        assert np.array_equal(stat[key], want[key]), key
    assert np.array_equal(_bits(stat["stats"][:, :5]), _bits(want["stats"][:, :5]))
    cmap = ds.actuator_cost_map(M, seed=6, cost_threshold=1.0)
    assert cmap["stats"].shape == (9, 9, 8)
    assert np.array_equal(_bits(cmap["stats"].reshape(81, 8, order="F")), _bits(stat["stats"]))
    assert cmap["n_left"][4, 4] == 0
