"""GPU tests of the lookahead under a control-dependent node set (hjb_rollout_set_control_lookahead /
hjb_rollout_run_control_lookahead, csrc/kernels_rollout_ctrl_lookahead.h: K35; hjbdp.ControlLookaheadRollout.run_control_lookahead,
Dynamic_Solver.get_actuator_lookahead_paths): every instantiation bit-equal to the host twin and to
tests/control_lookahead_rollout_refs.py, staged and not, on the nominal and on the actuator plant; the node counts; the identities
with K27 and K26; one step at every grid node against the control-dependent backup (K32) it restates; the closed loop on the
exactly posed lattice against the stored labels' actuator flight (K33); streams and chunks; isolation, the refusals that need a
device, and the mirror."""
import ctypes as C

import numpy as np
import pytest

import actuator_rollout_refs as arefs
import control_lookahead_rollout_refs as refs
import lookahead_rollout_refs as lrefs
from test_rollout_lookahead_abi import NAMES, _same, check_bits

pytestmark = pytest.mark.gpu

PLANES, N_TRAJ = refs.PLANES, refs.N_TRAJ
SENT = -12345.678


def _open(pb, actuator=True):
    """an hjbdp.ControlLookaheadRollout on problem pb with the model, the values, the per-control set and (actuator) the plant"""
    import hjbdp
    m = pb["model"]
    ro = hjbdp.ControlLookaheadRollout(m["knots"], refs.labels_stub(m["knots"], pb["nl"], 1), m["u_table"], index_base=1)
    ro.set_model(m["A"], m["B"], c=m["c"], q=m["q"], r=m["r"])
    ro.set_values(m["J"])
    ro.set_control_lookahead(pb["E"], pb["P"], pb["mode"])
    if actuator:
        ro.set_actuator_noise(pb["eps"], pb["Pf"], pb["base"])
    return ro


def _drawn(Pf, W, n, K, seed, first):
    import hjbdp
    return hjbdp.noise_draw(hjbdp.noise_thresholds(Pf, W), n, K, seed=seed, first_stream=first)


# ---- 1. every instantiation against the host twin and the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("fly", [False, True], ids=["nominal", "actuator"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_every_instantiation_is_bit_equal_to_the_host_twin_and_the_restatement(built, D, dtype, fly):
    import hjbdp
    pb = refs.problem(D, dtype, salt=int(fly))
    m, X0, seed, first = pb["model"], pb["X0"], pb["seed"], pb["first"]
    kw = dict(nodes=_drawn(pb["Pf"], 3, N_TRAJ, len(PLANES), seed, first), eps=pb["eps"], base=pb["base"]) if fly else {}
    ref = refs.rollout(m["knots"], m["u_table"], m["A"], m["B"], m["J"], X0, PLANES, pb["E"], pb["P"], pb["mode"], c=m["c"], q=m["q"],
                       r=m["r"], index_base=1, **kw)
    check_bits(hjbdp.control_lookahead_host(X0=X0, value_plane_of_step=PLANES, offsets=pb["E"], weights=pb["P"], mode=pb["mode"],
                                            index_base=1, keep_path=True, **m, **kw), ref, "host twin")
    assert not (ref[4] - 1 == pb["nl"] - 1).any()          # the last row of u_table and of the table duplicates another: the lower label wins
    assert len(np.unique(ref[4])) > 1                      # (the argmin is not one label everywhere)
    lo = np.array([k[0] for k in m["knots"]])
    hi = np.array([k[-1] for k in m["knots"]])
    assert (ref[2] < lo[None, :, None]).any() and (ref[2] > hi[None, :, None]).any()       # (states outside the grid on both sides)
    with _open(pb) as ro:                                  # the actuator set is held in the nominal runs too: they must not read it
        ro.set_lookahead(np.full((D, 2), 0.25), None, "worst")     # ... nor hjb_rollout_set_lookahead's set
        for lds in (1, 0):
            ro.set_option("lds", lds)
            out = ro.run_control_lookahead(X0, PLANES, actuator=fly, seed=seed, first_stream=first, keep_path=True)
            check_bits(out, ref, (lds, "kernel"))          # X_final, cost, X_path, U_path, L_path, V_path
            if fly:
                assert np.array_equal(out["W_path"], kw["nodes"]) and len(np.unique(out["W_path"])) == 3
            else:
                assert out["W_path"] is None
        lean = ro.run_control_lookahead(X0, PLANES, actuator=fly, seed=seed, first_stream=first)
        assert lean["X_path"] is None and lean["L_path"] is None and lean["V_path"] is None and lean["W_path"] is None
        assert _same(lean["X_final"], ref[0]) and _same(lean["cost"], ref[1])


# ---- 2. node counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 128])
def test_node_counts_at_d2(built, W):
    """W = 128 with 5 labels puts the table (128 + 5 * 2 * 128 doubles) well past any scalar-cache line"""
    import hjbdp
    pb = refs.problem(2, np.float64)
    m, X0 = pb["model"], pb["X0"]
    rng = np.random.default_rng(3690 + W)
    nodes = _drawn(pb["Pf"], 3, N_TRAJ, len(PLANES), 9, 0)
    with _open(pb) as ro:
        for mode in ("expect", "worst"):
            E, P = refs.control_table(rng, 2, W, pb["nl"], [0, 1], with_weights=(mode == "expect"))
            ref = refs.rollout(m["knots"], m["u_table"], m["A"], m["B"], m["J"], X0, PLANES, E, P, mode, c=m["c"], q=m["q"], r=m["r"],
                               index_base=1, nodes=nodes, eps=pb["eps"], base=pb["base"])
            ro.set_control_lookahead(E, P, mode)
            for lds in (1, 0):
                ro.set_option("lds", lds)
                check_bits(ro.run_control_lookahead(X0, PLANES, actuator=True, seed=9, keep_path=True), ref, (W, mode, lds))


# ---- 3. identities --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_a_table_constant_along_l_is_k27_and_one_zero_node_is_run_greedy(built, D):
    pb = refs.problem(D, np.float32 if D % 2 else np.float64, salt=2)
    X0 = pb["X0"]
    rng = np.random.default_rng(3620 + D)
    axes = [0, D - 1] if D >= 3 else [D - 1]
    zero = np.zeros((D, 1, pb["nl"]))
    zero[D - 1, 0, 0] = -0.0
    with _open(pb, actuator=False) as ro:
        for mode in ("expect", "worst"):
            E, P = lrefs.node_sets(rng, D, 3, axes, with_weights=(mode == "expect"))
            ro.set_lookahead(E, P, mode)
            want = ro.run_lookahead(X0, PLANES, keep_path=True)
            ro.set_control_lookahead(np.repeat(E[:, :, None], pb["nl"], axis=2), P, mode)
            got = ro.run_control_lookahead(X0, PLANES, keep_path=True)
            for name in NAMES:
                assert _same(got[name], want[name]), (mode, name)
            assert got["L_path"].dtype == np.int32 and got["W_path"] is None
        want = ro.run_greedy(X0, PLANES, keep_path=True)
        for mode, P in (("expect", [1.0]), ("worst", None)):
            ro.set_control_lookahead(zero, P, mode)
            got = ro.run_control_lookahead(X0, PLANES, keep_path=True)
            for name in NAMES:
                assert _same(got[name], want[name]), (mode, name)


# ---- 4. one step at every grid node is K32's backup ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["expect", "worst"])
@pytest.mark.parametrize("u_range", [None, (-4.0, 1.0)], ids=["kirk_controls", "fine_controls"])
def test_one_step_at_every_grid_node_is_the_control_dependent_backup(built, u_range, mode):
    """Dynamic_Solver's float64 terms are summed in K16's order and K32 combines candidate l's nodes as the lookahead does, so a
    candidate at a grid node is the control-dependent backup's candidate bit for bit: label and minimum of a one-step run on plane
    k + 1 are idx_stages[:, k] and J_stages[:, k].  Over Kirk's own controls ([-40, 10], 3.125 apart) the worst-case design
    stores one label everywhere; over [-4, 1] (tests/test_gpu_rollout_lookahead_campaign.py's range, for its reason) the design
    uses the control, so the labels compared are not one constant."""
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.dx, ds.du, ds.N = 13, 17, 6
    if u_range is not None:
        ds.u_min, ds.u_max = u_range
    w = np.array([0.25, 0.5, 0.25])
    ds.actuator_noise = ([-0.5, 0.0, 0.4], w if mode == "expect" else None, mode)
    spec = ds.build_spec()
    off, wts, _ = spec.control_disturbance
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    n_st = ds.N - 1
    with hjbdp.Backup(spec) as bk:
        assert bk.info()["kernel_variant"] == 8 and bk.get_option("dist_ctrl") == 1
        out = bk.solve(n_st, keep_J=True, keep_idx=True)
    J, idx = out["J_stages"], out["idx_stages"]
    nodes = np.array([[s_r[i], s_r[j]] for j in range(13) for i in range(13)]).T           # axis 0 fastest, as the planes
    with hjbdp.ControlLookaheadRollout([s_r, s_r], idx, np.asarray(ds._U_mesh, dtype=np.float64), index_base=1) as ro:
        ro.set_model(ds.A, ds.B, q=np.diag(ds.Q), r=[ds.R])
        ro.set_values(J)
        ro.set_control_lookahead(off, wts, mode)
        for k in range(n_st):
            got = ro.run_control_lookahead(nodes, [k + 1 if k + 1 < n_st else -1], keep_path=True)
            assert np.array_equal(got["L_path"][:, 0], idx[:, k].astype(np.int32)), k
            assert _same(got["V_path"][:, 0], J[:, k]), k
        own = ro.run_control_lookahead(nodes, [1], keep_path=True)
        ro.set_control_lookahead(np.repeat(off[:, :, :1], off.shape[2], axis=2), wts, mode)
        first = ro.run_control_lookahead(nodes, [1], keep_path=True)
        assert not _same(first["V_path"][:, 0], own["V_path"][:, 0])                       # (the per-candidate read is live)
    print("labels in use:", len(np.unique(idx)))
    assert len(np.unique(idx)) > 1 or u_range is None                                      # (the argmin is not one label everywhere)


# ---- 5. design, fly, compare on the exactly posed lattice -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["expect", "worst"])
def test_lattice_lookahead_on_the_actuator_plant_is_the_stored_labels_actuator_flight(built, mode):
    """Under the lattice's exact policy all 3^6 node sequences from all 9 starts visit only integer knots with |x| <= 4
    (tests/test_control_lookahead_refs.py checks it without a device); the grid is +-16, so no flight leaves it and 'nearest'
    reads the stored label exactly: the lookahead on J and the stored labels fly the same loop."""
    import hjbdp
    K = arefs.LATTICE_STAGES
    spec = arefs.lattice_spec(mode)
    with hjbdp.Backup(spec) as bk:
        assert bk.info()["kernel_variant"] == 8 and bk.get_option("dist_ctrl") == 1
        sol = bk.solve(K, keep_J=True, keep_idx=True)
    J = sol["J_stages"].reshape(33, K, order="F")
    idx = sol["idx_stages"].reshape(33, K, order="F")
    off, weights, _ = spec.control_disturbance
    X0 = np.repeat(arefs.LATTICE_STARTS, 32).reshape(1, -1)                                # 288 trajectories
    seed = 2035
    with hjbdp.ControlLookaheadRollout([arefs.LATTICE_KNOTS], idx, arefs.LATTICE_U, index_base=0) as ro:
        ro.set_model([[1.0]], [[1.0]], q=[1.0], r=[arefs.LATTICE_R])
        ro.set_values(J)
        ro.set_control_lookahead(off, weights, mode)
        ro.set_actuator_noise(arefs.LATTICE_EPS, weights)
        stored = ro.run_actuator(X0, np.arange(K), seed=seed, method="nearest", keep_path=True)
        look = ro.run_control_lookahead(X0, list(range(1, K)) + [-1], actuator=True, seed=seed, keep_path=True)
    for key in ("X_path", "U_path", "cost", "W_path", "X_final"):
        assert _same(look[key], stored[key]), key
    Xp = look["X_path"]
    assert np.abs(Xp).max() <= 16 and np.array_equal(Xp, np.round(Xp))                      # every visited state a knot inside the grid
    assert len(np.unique(look["W_path"])) == 3 and len(np.unique(look["U_path"])) >= 3
    node = Xp[:, 0, :].astype(np.int64) + 16
    for k in range(K):
        assert np.array_equal(look["L_path"][:, k], idx[node[:, k], k].astype(np.int32)), k
        assert _same(look["V_path"][:, k], J[node[:, k], k]), k


# ---- 6. streams and chunks -------------------------------------------------------------------------------------------------------------
def test_streams_count_through_the_call_and_chunks_change_no_bit(built):
    pb = refs.problem(3, np.float64)
    n = N_TRAJ // 2
    X0 = pb["X0"]
    keys = NAMES + ("W_path",)
    with _open(pb) as ro:
        whole = ro.run_control_lookahead(X0, PLANES, actuator=True, seed=41, first_stream=500, keep_path=True)
        assert np.array_equal(whole["W_path"], _drawn(pb["Pf"], 3, N_TRAJ, len(PLANES), 41, 500))      # W_path is hjb_rollout_noise_draw
        halves = [ro.run_control_lookahead(X0[:, i * n:(i + 1) * n], PLANES, actuator=True, seed=41, first_stream=500 + i * n, keep_path=True)
                  for i in (0, 1)]
        for key in keys:
            axis = 1 if key == "X_final" else 0
            assert _same(np.concatenate([h[key] for h in halves], axis=axis), whole[key]), key
        ro.set_option("chunk", 32)                         # 3 chunks: 32 + 32 + 6
        chunked = ro.run_control_lookahead(X0, PLANES, actuator=True, seed=41, first_stream=500, keep_path=True)
        nominal_chunked = ro.run_control_lookahead(X0, PLANES, keep_path=True)
        ro.set_option("chunk", 1 << 20)
        nominal = ro.run_control_lookahead(X0, PLANES, keep_path=True)
        for key in keys:
            assert _same(chunked[key], whole[key]), key
        for key in NAMES:
            assert _same(nominal_chunked[key], nominal[key]), key
        assert not _same(nominal["X_final"], whole["X_final"])
        other = ro.run_control_lookahead(X0, PLANES, actuator=True, seed=42, first_stream=500, keep_path=True)
        assert not np.array_equal(other["W_path"], whole["W_path"])


# ---- 7. isolation and refusals with a device -------------------------------------------------------------------------------------------
def _raw_run(ro, fly, planes, X0, first_stream=0, with_W=False):
    """hjb_rollout_run_control_lookahead through ctypes on sentinel-filled outputs -> (status, the outputs)"""
    planes = np.ascontiguousarray(planes, dtype=np.int32)
    X = np.ascontiguousarray(np.asarray(X0, dtype=np.float64).T)
    nt, D = X.shape
    K, nu = int(planes.size), ro.n_u
    out = {"X_final": np.full((nt, D), SENT), "cost": np.full(nt, SENT), "X_path": np.full(nt * D * (K + 1), SENT),
           "U_path": np.full(nt * nu * K, SENT), "L_path": np.full(nt * K, SENT), "V_path": np.full(nt * K, SENT),
           "W_path": np.full(nt * K, SENT)}
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ms = C.c_double(SENT)
    st = ro.lib.hjb_rollout_run_control_lookahead(ro._ro, fly, K, planes.ctypes.data_as(C.POINTER(C.c_int32)), nt, f(X), 5, first_stream,
                                                  f(out["X_final"]), f(out["cost"]), f(out["X_path"]), f(out["U_path"]), f(out["L_path"]),
                                                  f(out["V_path"]), f(out["W_path"]) if with_W else None, C.byref(ms))
    out["device_ms"] = np.array([ms.value])
    return st, out


def _untouched(out):
    return all((a == SENT).all() for a in out.values())


def _others(ro, X0, label_planes):
    """every other run function of the object, paths kept"""
    return (ro.run(X0, label_planes, keep_path=True), ro.run_noisy(X0, label_planes, seed=5, keep_path=True),
            ro.run_greedy(X0, [1, 0, -1], keep_path=True), ro.run_lookahead(X0, [1, 0, -1], keep_path=True),
            ro.run_lookahead(X0, [1, 0, -1], noisy=True, seed=5, first_stream=9, keep_path=True),
            ro.run_actuator(X0, label_planes, seed=5, first_stream=3, keep_path=True),
            ro.run_campaign(X0[:, :11], label_planes, 6, seed=5, cost_threshold=0.5, settle_tol=0.4),
            ro.run_lookahead_campaign(X0[:, :11], [1, 0, -1], 6, seed=5, cost_threshold=0.5, settle_tol=0.4),
            ro.run_actuator_campaign(X0[:, :11], label_planes, 6, seed=5, cost_threshold=0.5, settle_tol=0.4))


def test_the_control_lookahead_set_is_read_by_its_run_functions_alone_and_refusals(built):
    import hjbdp
    from hjbdp import _abi
    from test_gpu_rollout import _random_problem
    rng = np.random.default_rng(354)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 3, 2, np.uint16, 9, 4)
    nl = ut.shape[0]
    lo = np.array([k[0] for k in knots]) - 0.1
    hi = np.array([k[-1] for k in knots]) + 0.1
    X0 = rng.uniform(lo[:, None], hi[:, None], size=(3, N_TRAJ))
    planes = rng.integers(0, 4, size=6)
    nS = int(np.prod([len(k) for k in knots]))
    V = rng.uniform(0, 1, size=(nS, 2))
    off, p = rng.uniform(-0.2, 0.2, size=(3, 5)), rng.uniform(0.1, 1.0, size=5)
    E2, P2 = lrefs.node_sets(rng, 3, 3, [0, 2])
    E, P = refs.control_table(rng, 3, 3, nl, [0, 2])
    eps, abase, Pf = refs.actuator_set(rng, 3, 2)
    err = lambda ro: ro.lib.hjb_rollout_last_error(ro._ro).decode()
    with hjbdp.ControlLookaheadRollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=np.ones(3), r=[0.5, 0.25])
        # without values: refused, outputs untouched
        ro.set_control_lookahead(E, P)
        st, out = _raw_run(ro, 0, [0, 1], X0)
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "hjb_rollout_set_values" in err(ro)
        ro.clear_control_lookahead()
        ro.set_values(V)
        ro.set_lookahead(E2, P2)                           # hjb_rollout_set_lookahead's set is not this call's set
        st, out = _raw_run(ro, 0, [0, 1], X0)
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "before hjb_rollout_set_control_lookahead" in err(ro)
        ro.set_noise(off, p)                               # ... and hjb_rollout_set_noise's set is not the actuator set
        ro.set_actuator_noise(eps, Pf, abase)
        before = _others(ro, X0, planes)
        ro.set_control_lookahead(E, P)
        during = _others(ro, X0, planes)
        for a, b in zip(during, before):
            for key in a:
                if key != "device_ms" and a[key] is not None:
                    assert np.array_equal(a[key], b[key], equal_nan=True), key
        look = ro.run_control_lookahead(X0, [1, 0, -1], keep_path=True)
        check_bits(look, refs.rollout(knots, ut, A, B, V, X0, [1, 0, -1], E, P, c=c, q=np.ones(3), r=[0.5, 0.25], index_base=base))
        assert not _same(look["V_path"], before[3]["V_path"])
        # actuator = True with no actuator set
        ro.clear_actuator_noise()
        st, out = _raw_run(ro, 1, [0, 1], X0, with_W=True)
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "before hjb_rollout_set_actuator_noise" in err(ro)
        ro.set_actuator_noise(eps, Pf, abase)
        # a table whose n_controls is wrong: refused, and the set the object holds stays
        d = np.zeros(3 * 3 * (nl + 1))
        dp = d.ctypes.data_as(C.POINTER(C.c_double))
        for nc in (nl - 1, nl + 1, 0):
            assert ro.lib.hjb_rollout_set_control_lookahead(ro._ro, 0, 3, nc, dp, None) == _abi.HJB_E_INVALID
            assert "n_controls=%d, the object has %d labels" % (nc, nl) in err(ro)
        d[2 + 3 * (1 + 3 * 2)] = np.inf
        assert ro.lib.hjb_rollout_set_control_lookahead(ro._ro, 0, 3, nl, dp, None) == _abi.HJB_E_INVALID
        assert "offset of axis 2, node 1, control 2 is not finite" in err(ro)
        with pytest.raises(ValueError):
            ro.set_control_lookahead(E[:, :, :nl - 1], P)
        again = ro.run_control_lookahead(X0, [1, 0, -1], keep_path=True)
        assert _same(again["V_path"], look["V_path"])
        # the remaining refusals, each with the outputs untouched
        for args, text in (((0, [0], X0, 0, True), "W_path given with fly_noise=0"), ((1, [0], X0, -1, True), "first_stream=-1 < 0"),
                           ((2, [0], X0, 0, False), "fly_noise=2"), ((0, [2], X0, 0, False), "outside [-1, 2)"),
                           ((1, [0, -2], X0, 0, True), "outside [-1, 2)")):
            st, out = _raw_run(ro, *args)
            assert st == _abi.HJB_E_INVALID and _untouched(out), args
            assert text in err(ro), (args, err(ro))
        bad = X0.copy()
        bad[2, 17] = np.inf
        st, out = _raw_run(ro, 1, [0], bad, with_W=True)
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "not finite" in err(ro)
        st, out = _raw_run(ro, 1, [-1, 0], X0, with_W=True)
        assert st == _abi.HJB_OK and not any((a == SENT).any() for a in out.values())
    # an object without a model, and one with another model
    with hjbdp.ControlLookaheadRollout(knots, labels, ut, index_base=base) as ro:
        ro.set_values(V)
        ro.set_control_lookahead(E, P)
        st, out = _raw_run(ro, 0, [0], X0)
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "before hjb_rollout_set_model" in err(ro)
    knots6 = [np.linspace(-1, 1, 3)] * 6
    labels6 = rng.integers(1, 4, size=(3 ** 6, 1)).astype(np.uint8)
    with hjbdp.ControlLookaheadRollout(knots6, labels6, rng.uniform(-1, 1, size=(3, 3)), index_base=1) as ro:
        ro.set_attitude_model([1.0, 2.0, 3.0], 0.01)
        ro.set_values(np.zeros((3 ** 6, 1)))
        ro.set_control_lookahead(np.zeros((6, 1, 3)))
        st, out = _raw_run(ro, 0, [0], np.zeros((6, 2)))
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "needs the affine model" in err(ro)


def test_dynamic_solver_actuator_lookahead_methods(built):
    import hjbdp
    from test_gpu_rollout_lookahead_campaign import DS_U_RANGE
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.dx, ds.du, ds.N = 13, 17, 6
    ds.u_min, ds.u_max = DS_U_RANGE
    eps, w = np.array([-0.4, 0.0, 0.4]), np.array([1.0, 2.0, 1.0])
    with pytest.raises(RuntimeError, match="actuator_noise"):                   # no actuator_noise: refused before any device work
        ds.get_actuator_lookahead_paths(np.zeros((2, 1)))
    ds.actuator_noise = (eps, w, "expect")
    ds.run()
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    X0 = np.array([[s_r[0], s_r[0]], [s_r[6], s_r[8]], [s_r[12], s_r[12]], [2.0, 1.0], [0.3, -0.7]]).T
    X, U = ds.get_actuator_lookahead_paths(X0)
    assert X.shape == (2, 6, 5) and U.shape == (6, 5) and not U[5].any()
    assert ds.actuator_lookahead_cost.shape == (5,) and ds.actuator_lookahead_paths_ms > 0
    cost = ds.get_actuator_lookahead_paths(X0, n_samples=8, seed=6)
    assert cost.shape == (5, 8)
    assert np.array_equal(ds.actuator_lookahead_cost_mean, cost.mean(axis=1)) and np.array_equal(ds.actuator_lookahead_cost_max, cost.max(axis=1))
    assert np.array_equal(ds.actuator_lookahead_cost_std, cost.std(axis=1)) and np.all(ds.actuator_lookahead_cost_std[3:] > 0)
    stat = ds.get_actuator_lookahead_cost_statistics(X0, 8, seed=6, cost_threshold=1.0)
    want = hjbdp.campaign_reduce(cost.reshape(-1), 8, cost_threshold=1.0)       # the same streams: the same costs
    for key in ("mean", "var", "std", "min", "max", "n_exceed"):
        assert np.array_equal(stat[key], want[key]), key
    cmap = ds.actuator_lookahead_cost_map(4, seed=6)
    assert cmap["stats"].shape == (13, 13, 8) and cmap["mean"].shape == (13, 13)
    labels_map = ds.actuator_cost_map(4, seed=6)                                # the stored labels on the same streams
    assert labels_map["mean"].shape == (13, 13) and not np.array_equal(labels_map["mean"], cmap["mean"])
    # by hand: the table build_spec gives the backup, beside set_actuator_noise(eps, weights)
    off, wts, mode = ds.build_spec().control_disturbance
    with hjbdp.ControlLookaheadRollout([s_r, s_r], ds.u_star_idxs, np.asarray(ds._U_mesh, dtype=np.float64), index_base=1) as ro:
        ro.set_model(ds.A, ds.B, q=np.diag(ds.Q), r=[ds.R])
        ro.set_values(ds.J_star)
        ro.set_control_lookahead(off, wts, mode)
        ro.set_actuator_noise(eps, w)
        direct = ro.run_control_lookahead(X0, np.arange(1, 6), keep_path=True)
        assert _same(X, direct["X_path"].transpose(1, 2, 0)) and _same(U[:5], direct["U_path"][:, 0, :].T)
        for i in range(5):                                 # sample j of start i on stream i * n_samples + j
            by_hand = ro.run_control_lookahead(np.repeat(X0[:, i:i + 1], 8, axis=1), np.arange(1, 6), actuator=True, seed=6, first_stream=8 * i)
            assert _same(by_hand["cost"], cost[i]), i
    # the three additive flights keep refusing while actuator_noise is set
    for old in (lambda: ds.get_lookahead_paths(X0), lambda: ds.get_noisy_paths(X0, 2), lambda: ds.get_lookahead_cost_statistics(X0, 2)):
        with pytest.raises(RuntimeError, match="control-dependent noise"):
            old()
