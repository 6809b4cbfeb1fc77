"""GPU tests of the lookahead campaign (hjb_rollout_run_lookahead_campaign, csrc/kernels_rollout_lookahead_campaign.h: K29;
hjbdp.Rollout.run_lookahead_campaign, Dynamic_Solver.lookahead_cost_map).  The anchor is code older than the campaign:
run_lookahead(noisy=True) (K27) and hjbdp.campaign_reduce (K28's host reduce).  Every check is "K29's stats == campaign_reduce of
K27's own per-trajectory outputs on np.repeat(X0, M, axis=1), with campaign_refs.left_flags of its X_path", compared as bits: at
every instantiation (and against the host twin), at every block shape, under chunking and split calls, with one zero node against
K26, on the exactly posed lattice against the label campaign (K28), with the refusals, and through Dynamic_Solver."""
import ctypes as C

import numpy as np
import pytest

import campaign_refs as crefs
import lookahead_campaign_refs as lc
import lookahead_rollout_refs as lrefs
import noisy_rollout_refs as nrefs
from lookahead_campaign_refs import PLANES, bits

pytestmark = pytest.mark.gpu

KEYS = ("mean", "var", "std", "min", "max", "n_exceed", "n_left", "n_settled", "mean_settled")
SENT = 7.25


def _labels_stub(knots, n_labels, base):
    """labels the lookahead never reads: one plane of the last label"""
    return np.full((int(np.prod([len(k) for k in knots])), 1), base + n_labels - 1, dtype=np.int32)


def _open(pb):
    """an object holding the problem's model, value planes, lookahead set and flight set"""
    import hjbdp
    ro = hjbdp.Rollout(pb["knots"], _labels_stub(pb["knots"], 5, 1), pb["ut"], index_base=1)
    try:
        ro.set_model(pb["A"], pb["B"], **pb["model"])
        ro.set_values(pb["V"])
        ro.set_lookahead(pb["E"], pb["P"], pb["mode"])
        ro.set_noise(pb["F"], pb["Pf"])
    except Exception:
        ro.close()
        raise
    return ro


def _k27(ro, knots, X0, M, planes, seed, first):
    """K27's own per-trajectory outputs on the starts repeated M times, with the left-the-grid flags of its X_path"""
    flown = ro.run_lookahead(np.repeat(X0, M, axis=1), planes, noisy=True, seed=seed, first_stream=first, keep_path=True)
    flown["left"] = crefs.left_flags(flown["X_path"], knots)
    return flown


def _same_stats(got, want, what):
    assert got["stats"].shape == want["stats"].shape, what
    assert np.array_equal(bits(got["stats"]), bits(want["stats"])), (what, got["stats"], want["stats"])
    for key in KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), (what, key)


# ---- 1. every instantiation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_every_instantiation_is_bit_equal_to_the_reduced_k27_run_and_the_host_twin(built, D, dtype):
    import hjbdp
    pb = lc.problem(D, dtype)                       # seeds checked without a device: test_lookahead_campaign_host.py
    M, ns = 5, lc.N_STARTS                          # G = 8 with three padding slots; 37 blocks: the last wave part-filled
    X0, seed, first = pb["X0"], pb["seed"], pb["first"]
    with _open(pb) as ro:
        flown = _k27(ro, pb["knots"], X0, M, PLANES, seed, first)
        bounds = lc.bounds_of(flown)                # the median cost, the mean |x_final|: slots 4, 6 and 7 neither empty nor full
        for lds in (1, 0):
            ro.set_option("lds", lds)
            for thr, tol in ((None, None), bounds):
                got = ro.run_lookahead_campaign(X0, PLANES, M, seed=seed, first_stream=first, cost_threshold=thr, settle_tol=tol)
                _same_stats(got, lc.reduce_flown(flown, M, thr, tol), (lds, thr))
                twin = hjbdp.lookahead_campaign_host(pb["knots"], pb["ut"], pb["A"], pb["B"], pb["V"], X0, PLANES, M, pb["E"], pb["F"],
                                                     weights=pb["P"], mode=pb["mode"], flight_weights=pb["Pf"], seed=seed, first_stream=first,
                                                     cost_threshold=thr, settle_tol=tol, **pb["model"])
                _same_stats(got, twin, (lds, thr, "host twin"))
            assert got["device_ms"] > 0
    assert flown["left"].any() and got["n_left"].sum() == flown["left"].sum()
    assert 0 < got["n_exceed"].sum() < ns * M and 0 < got["n_settled"].sum() < ns * M


# ---- 2. block shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3, 63, 64, 65, 200])
def test_block_shapes(built, M):
    """one block per start (M <= 64: one lane, two, four of which one is padding, 64 with one padding slot, 64 full), two blocks
    with the second almost all padding (65), four blocks (200); with 1, 3 and 70 starts"""
    pb = lc.problem(2, np.float64, n_starts=70)
    with _open(pb) as ro:
        for ns in (1, 3, 70):
            X0 = pb["X0"][:, 70 - ns:] if ns < 70 else pb["X0"]     # the few starts from the end: outside the grid
            flown = _k27(ro, pb["knots"], X0, M, PLANES, 11 + ns, 1000 * ns)
            thr, tol = np.full(ns, np.median(flown["cost"])), np.array([0.3, 0.3])
            got = ro.run_lookahead_campaign(X0, PLANES, M, seed=11 + ns, first_stream=1000 * ns, cost_threshold=thr, settle_tol=tol)
            _same_stats(got, lc.reduce_flown(flown, M, thr, tol), (M, ns))
            c2 = flown["cost"].reshape(ns, M)
            assert np.array_equal(got["min"], c2.min(axis=1)) and np.array_equal(got["max"], c2.max(axis=1))


# ---- 3. chunks and streams -----------------------------------------------------------------------------------------------------------
def test_chunks_and_streams_change_no_bit(built):
    pb = lc.problem(2, np.float32, n_starts=14)
    M, first = 200, 300
    X0 = pb["X0"]
    kw = dict(seed=12, cost_threshold=0.5, settle_tol=0.3)
    with _open(pb) as ro:
        flown = _k27(ro, pb["knots"], X0[:, :7], M, PLANES, 12, first)
        whole = ro.run_lookahead_campaign(X0[:, :7], PLANES, M, first_stream=first, **kw)
        _same_stats(whole, lc.reduce_flown(flown, M, 0.5, 0.3), "whole")
        for chunk in (64, 192, 1 << 20, 1):         # one block a launch; three: a start's four blocks across launches; one launch;
            ro.set_option("chunk", chunk)           # below one block: a launch still takes a whole block
            got = ro.run_lookahead_campaign(X0[:, :7], PLANES, M, first_stream=first, **kw)
            assert np.array_equal(bits(got["stats"]), bits(whole["stats"])), chunk
        ro.set_option("chunk", 1 << 20)
        both = ro.run_lookahead_campaign(X0, PLANES, M, first_stream=first, **kw)
        second = ro.run_lookahead_campaign(X0[:, 7:], PLANES, M, first_stream=first + 7 * M, **kw)
        assert np.array_equal(bits(both["stats"][:7]), bits(whole["stats"]))
        assert np.array_equal(bits(both["stats"][7:]), bits(second["stats"]))
        other = ro.run_lookahead_campaign(X0[:, :7], PLANES, M, seed=13, first_stream=first)
        assert not np.array_equal(other["stats"][:, 0], whole["stats"][:, 0])
        assert not other["n_exceed"].any() and not other["n_settled"].any() and not other["stats"][:, 7].any()


# ---- 4. identities -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_one_zero_node_in_both_sets_is_m_copies_of_run_greedy(built, D):
    import hjbdp
    pb = lc.problem(D, np.float32 if D % 2 else np.float64)
    zero = np.zeros((D, 1))
    zero[D - 1, 0] = -0.0
    M = 5
    with _open(pb) as ro:
        greedy = ro.run_greedy(pb["X0"], PLANES, keep_path=True)
        ro.set_noise(zero, None)
        for mode, P in (("expect", [1.0]), ("worst", None)):
            ro.set_lookahead(zero, P, mode)
            got = ro.run_lookahead_campaign(pb["X0"], PLANES, M, seed=3)
            assert np.array_equal(bits(got["min"]), bits(greedy["cost"])) and np.array_equal(bits(got["max"]), bits(greedy["cost"]))
            want = hjbdp.campaign_reduce(np.repeat(greedy["cost"], M), M, X_final=np.repeat(greedy["X_final"], M, axis=1),
                                         left=np.repeat(crefs.left_flags(greedy["X_path"], pb["knots"]), M))
            _same_stats(got, want, mode)


# ---- 5. the exactly posed lattice: the lookahead campaign is the label campaign --------------------------------------------------------
@pytest.mark.parametrize("mode", ["expect", "worst"])
def test_lattice_lookahead_campaign_is_the_label_campaign(built, mode):
    """K27's lattice test shows the flights of the two controllers coincide under one seed; so do their campaigns, bit for bit,
    and K28's "promised is paid" carries over"""
    import hjbdp
    K = nrefs.LATTICE_STAGES
    with hjbdp.Backup(nrefs.lattice_spec(mode)) as bk:
        sol = bk.solve(K, keep_J=True, keep_idx=True)
    J = sol["J_stages"].reshape(33, K, order="F")
    idx = sol["idx_stages"].reshape(33, K, order="F")
    weights = nrefs.LATTICE_P if mode == "expect" else None
    X0 = nrefs.LATTICE_STARTS.reshape(1, -1)                                    # 9 starts
    M, seed = 1 << 12, 2029
    thr = J[(nrefs.LATTICE_STARTS + 16).astype(np.int64), 0]                    # what the solve promised at the start
    with hjbdp.Rollout([nrefs.LATTICE_KNOTS], idx, nrefs.LATTICE_U, index_base=0) as ro:
        ro.set_model([[1.0]], [[1.0]], q=[1.0], r=[0.5])
        ro.set_noise(nrefs.LATTICE_NODES, weights)
        ro.set_values(J)
        ro.set_lookahead(nrefs.LATTICE_NODES, weights, mode)
        labels = ro.run_campaign(X0, np.arange(K), M, seed=seed, method="nearest", cost_threshold=thr, settle_tol=1.0)
        look = ro.run_lookahead_campaign(X0, list(range(1, K)) + [-1], M, seed=seed, cost_threshold=thr, settle_tol=1.0)
    _same_stats(look, labels, mode)
    assert not look["n_left"].any()                                             # every reachable state is a knot inside the grid
    assert look["n_settled"].sum() > 0 and np.all(look["std"] > 0)
    if mode == "worst":
        assert not look["n_exceed"].any()                                       # the promised maximum is never exceeded


# ---- 6. isolation and refusals with a device ---------------------------------------------------------------------------------------
def _others(ro, X0, label_planes):
    """every other run function of the object, paths kept"""
    return (ro.run(X0, label_planes, keep_path=True), ro.run_noisy(X0, label_planes, seed=5, keep_path=True),
            ro.run_greedy(X0, [1, 0, -1], keep_path=True), ro.run_lookahead(X0, [1, 0, -1], keep_path=True),
            ro.run_lookahead(X0, [1, 0, -1], noisy=True, seed=5, first_stream=9, keep_path=True),
            ro.run_campaign(X0[:, :11], label_planes, 6, seed=5, cost_threshold=0.5, settle_tol=0.4))


def test_isolation_and_refusals_with_a_device(built):
    import hjbdp
    from hjbdp import _abi
    from test_gpu_rollout import _random_problem
    rng = np.random.default_rng(294)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 3, 2, np.uint16, 9, 4)
    lo = np.array([k[0] for k in knots]) - 0.1
    hi = np.array([k[-1] for k in knots]) + 0.1
    X0 = rng.uniform(lo[:, None], hi[:, None], size=(3, 300))
    label_planes = rng.integers(0, 4, size=6)
    nS = int(np.prod([len(k) for k in knots]))
    V = rng.uniform(0, 1, size=(nS, 2))
    off, p = rng.uniform(-0.2, 0.2, size=(3, 5)), rng.uniform(0.1, 1.0, size=5)
    E, P = lrefs.node_sets(rng, 3, 3, [0, 2])
    ns, M = 11, 6
    vplanes = np.array([1, 0, -1, 1], dtype=np.int32)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    Xc = np.ascontiguousarray(X0[:, :ns].T)

    def raw(ro, **call):
        """hjb_rollout_run_lookahead_campaign through ctypes on sentinel-filled outputs -> (status, outputs untouched, the text)"""
        stats = np.full(ns * 8, SENT)
        ms = C.c_double(SENT)
        st = ro.lib.hjb_rollout_run_lookahead_campaign(ro._ro, call.get("K", len(vplanes)), call.get("pl", ip(vplanes)), call.get("ns", ns),
                                                       call.get("M", M), call.get("X", dp(Xc)), 4, call.get("first", 0), call.get("thr", None),
                                                       call.get("tol", None), call.get("stats", dp(stats)), C.byref(ms))
        return st, bool(np.all(stats == SENT) and ms.value == SENT), ro.lib.hjb_rollout_last_error(ro._ro).decode()

    def refused(ro, text, **call):
        st, untouched, err = raw(ro, **call)
        assert st == _abi.HJB_E_INVALID and untouched and text in err, (call, st, untouched, err)

    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        refused(ro, "before hjb_rollout_set_model")
        ro.set_model(A, B, c=c, q=np.ones(3), r=[0.5, 0.25])
        refused(ro, "before hjb_rollout_set_lookahead")
        ro.set_lookahead(E, P)
        refused(ro, "before hjb_rollout_set_noise")
        ro.set_noise(off, p)
        refused(ro, "before hjb_rollout_set_values")
        st, untouched, _ = raw(ro, pl=ip(np.full(4, -1, dtype=np.int32)))       # only -1: needs no values
        assert st == _abi.HJB_OK and not untouched
        ro.set_values(V)
        # the object holds all three sets: every other run function gives the bits it gave before
        before = _others(ro, X0, label_planes)
        good = ro.run_lookahead_campaign(X0[:, :ns], vplanes, M, seed=4, cost_threshold=0.5, settle_tol=0.4)
        flown = _k27(ro, knots, X0[:, :ns], M, vplanes, 4, 0)
        _same_stats(good, lc.reduce_flown(flown, M, 0.5, 0.4), "good")
        after = _others(ro, X0, label_planes)
        for a, b in zip(after, before):
            for key in a:
                if key != "device_ms" and a[key] is not None:
                    assert np.array_equal(a[key], b[key], equal_nan=True), key
        # the refusals, each on sentinel-filled outputs that stay untouched
        Xn = Xc.copy()
        Xn[7, 2] = np.inf
        thr, tol = np.full(ns, 0.5), np.full(3, 0.4)
        bad_thr, bad_tol, neg_tol = thr.copy(), tol.copy(), tol.copy()
        bad_thr[4], bad_tol[1], neg_tol[2] = np.nan, np.nan, -0.1
        for call, text in ((dict(first=-1), "first_stream=-1 < 0"), (dict(first=2 ** 63 - 10), "overflows"), (dict(M=0), "n_samples=0 < 1"),
                           (dict(M=2 ** 62), "n_starts * n_samples overflows"), (dict(K=-1), "n_steps=-1"), (dict(ns=-2), "n_traj=-2"),
                           (dict(pl=ip(np.array([0, 2, 0, 0], dtype=np.int32))), "value_plane_of_step[1] = 2 outside [-1, 2)"),
                           (dict(pl=ip(np.array([0, 0, -2, 0], dtype=np.int32))), "value_plane_of_step[2] = -2 outside [-1, 2)"),
                           (dict(pl=None), "null value_plane_of_step"), (dict(X=dp(Xn)), "not finite"), (dict(X=None), "null X0"),
                           (dict(thr=dp(bad_thr)), "threshold[4] is NaN"), (dict(tol=dp(bad_tol)), "tol[1]"),
                           (dict(tol=dp(neg_tol)), "tol[2]"), (dict(stats=None), "null stats")):
            refused(ro, text, **call)
        st, untouched, _ = raw(ro, ns=0)                                        # no starts: no work
        assert st == _abi.HJB_OK
        none = ro.run_lookahead_campaign(np.zeros((3, 0)), vplanes, M)
        assert none["stats"].shape == (0, 8) and none["device_ms"] == 0.0
        again = ro.run_lookahead_campaign(X0[:, :ns], vplanes, M, seed=4, cost_threshold=0.5, settle_tol=0.4)
        assert np.array_equal(bits(again["stats"]), bits(good["stats"])) and again["device_ms"] > 0
    assert hjbdp.load_library().hjb_rollout_run_lookahead_campaign(None, 0, None, 0, 1, None, 0, 0, None, None, None, None) == _abi.HJB_E_INVALID
    knots6 = [np.linspace(-1, 1, 3)] * 6                                        # a model other than the affine one
    with hjbdp.Rollout(knots6, rng.integers(1, 4, size=(3 ** 6, 1)).astype(np.uint8), rng.uniform(-1, 1, size=(3, 3)), index_base=1) as ro:
        ro.set_attitude_model([1.0, 2.0, 3.0], 0.01)
        ro.set_values(np.zeros((3 ** 6, 1)))
        ro.set_lookahead(np.zeros((6, 1)))
        ro.set_noise(np.full((6, 2), 0.01))
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_lookahead_campaign(np.zeros((6, 4)), [0, -1], 3)
        assert ei.value.status == _abi.HJB_E_INVALID and "needs the affine model" in str(ei.value)


# ---- 7. the mirror -------------------------------------------------------------------------------------------------------------------
# Dynamic_Solver at dx = 13, du = 17, N = 6 under a 3-node set.  The 17 controls span [-4, 1] here, not the fixture's [-40, 10]: over
# [-40, 10] they lie 3.125 apart, the smallest control other than 0.625 costs more (R u^2) than five steps can win back, and the
# solve stores ONE label in every plane but the first (measured: labels 13 and 14 in plane 0, 14 alone in planes 1 - 4).  The
# flights start on nodes, where plane 0 is read exactly, so every controller then flies the same constant control and the maps
# cannot differ whatever the node set (24 sets tried).  Over [-4, 1] (0.3125 apart) the solve uses the control - 8, 5, 3 and 2
# labels in planes 0 - 3 - and interpolated labels, nominal lookahead and disturbed lookahead have something to disagree about.
DS_U_RANGE = (-4.0, 1.0)
DS_NODES = np.array([[-0.03, 0.0, 0.03], [0.08, 0.0, -0.08]])
DS_WEIGHTS = np.array([1.0, 4.0, 1.0]) / 6.0


@pytest.fixture(scope="module")
def kirk(built):
    """Dynamic_Solver at dx = 13, du = 17, N = 6, float64, solved under the 3-node set; the grid's nodes as starts"""
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.dx, ds.du, ds.N = 13, 17, 6
    ds.u_min, ds.u_max = DS_U_RANGE
    ds.disturbance = (DS_NODES, DS_WEIGHTS, "expect")
    ds.run()
    assert all(len(np.unique(ds.u_star_idxs[:, :, k])) > 1 for k in range(4))  # the policy does use the control beyond the first plane
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    return ds, s_r, np.stack([np.tile(s_r, 13), np.repeat(s_r, 13)])           # node (i, j) at column i + 13 j: axis 0 fastest


def test_dynamic_solver_lookahead_cost_map(kirk):
    import hjbdp
    ds, s_r, nodes = kirk
    M = 8
    cmap = ds.lookahead_cost_map(M, seed=6, cost_threshold=1.0)
    cost = ds.get_lookahead_paths(nodes, n_samples=M, seed=6)                   # [169, 8], the same streams
    want = hjbdp.campaign_reduce(cost.reshape(-1), M, cost_threshold=1.0)
    for key in ("mean", "var", "std", "min", "max", "n_exceed"):
        assert cmap[key].shape == (13, 13), key
        assert np.array_equal(cmap[key].reshape(-1, order="F"), want[key]), key
    assert cmap["stats"].shape == (13, 13, 8) and cmap["n_left"].dtype == np.int64 and cmap["device_ms"] > 0
    assert np.array_equal(bits(cmap["stats"].reshape(169, 8, order="F")[:, :5]), bits(want["stats"][:, :5]))
    # 'nominal': the same with a one-zero-node lookahead set, flown by hand under the same plant
    nominal = ds.lookahead_cost_map(M, seed=6, lookahead="nominal", cost_threshold=1.0, settle_tol=0.5)
    ut = np.asarray(ds._U_mesh, dtype=np.float64)
    with hjbdp.Rollout([s_r, s_r], ds.u_star_idxs, ut, index_base=1) as ro:
        ro.set_model(ds.A, ds.B, q=np.diag(ds.Q), r=[ds.R])
        ro.set_values(ds.J_star)
        ro.set_lookahead(np.zeros((2, 1)), [1.0], "expect")
        ro.set_noise(DS_NODES, DS_WEIGHTS)
        flown = _k27(ro, [s_r, s_r], nodes, M, np.arange(1, 6), 6, 0)
    full = lc.reduce_flown(flown, M, 1.0, 0.5)
    assert np.array_equal(bits(nominal["stats"].reshape(169, 8, order="F")), bits(full["stats"]))
    assert 0 < nominal["n_left"].sum() < 169 * M                                # some flights are carried out of the grid, not all
    stat = ds.get_lookahead_cost_statistics(nodes[:, 10:13], M, seed=6)        # three starts on streams 0 .. 3 M
    cost3 = ds.get_lookahead_paths(nodes[:, 10:13], n_samples=M, seed=6)
    assert np.array_equal(bits(stat["stats"][:, :4]), bits(hjbdp.campaign_reduce(cost3.reshape(-1), M)["stats"][:, :4]))
    with pytest.raises(ValueError):
        ds.get_lookahead_cost_statistics(nodes[:, :2], M, lookahead="other")
    saved, ds.disturbance = ds.disturbance, None
    try:
        with pytest.raises(RuntimeError):
            ds.lookahead_cost_map(4)
    finally:
        ds.disturbance = saved


def test_dynamic_solver_maps_differ_from_the_label_map(kirk):
    """The streams pair with noisy_cost_map's, and both lookahead maps differ from its mean somewhere: the interpolated labels fly a
    continuous control, the lookaheads the best of 17 discrete ones, and the nominal lookahead ignores the nodes.  Measured on an
    MI355X: the disturbed map differs from the label map at 80 of 169 nodes, the nominal map at 80, the two from each other at 12."""
    ds, s_r, nodes = kirk
    M = 8
    labels = ds.noisy_cost_map(M, seed=6)
    assert labels["mean"].shape == (13, 13)
    nominal = ds.lookahead_cost_map(M, seed=6, lookahead="nominal")
    disturbed = ds.lookahead_cost_map(M, seed=6)
    n_nominal, n_disturbed = int((nominal["mean"] != labels["mean"]).sum()), int((disturbed["mean"] != labels["mean"]).sum())
    print("nodes whose mean differs from noisy_cost_map's: nominal %d, disturbed %d of 169" % (n_nominal, n_disturbed))
    assert n_nominal > 0
    assert n_disturbed > 0
    assert not np.array_equal(nominal["mean"], disturbed["mean"])
