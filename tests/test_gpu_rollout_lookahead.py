"""GPU tests of the disturbance-aware greedy rollout (hjb_rollout_set_lookahead / hjb_rollout_run_lookahead,
csrc/kernels_rollout_lookahead.h: K27; hjbdp.Rollout.run_lookahead, Dynamic_Solver.get_lookahead_paths): every instantiation
bit-equal to the host twin and to tests/lookahead_rollout_refs.py, staged and not, on a nominal and on a noisy plant; the
identities with K26 and K25's sampler; one step at every grid node against the disturbed backup (K24) it restates; the closed
loop on the exactly posed noisy lattice against the stored labels' noisy loop; isolation and the refusals that need a device."""
import ctypes as C

import numpy as np
import pytest

import greedy_rollout_refs as grefs
import lookahead_rollout_refs as refs
import noisy_rollout_refs as nrefs
from test_rollout_lookahead_abi import NAMES, _same, check_bits

pytestmark = pytest.mark.gpu

PLANES = [2, 0, 0, -1, 1, 2, -1, 1, 1]     # 9 steps: the Philox blocks of k = 4 and k = 8 begin inside; -1 twice, planes repeated
N_TRAJ = 300                               # one full 256-thread block and a partial one
SENT = -12345.678


def _labels_stub(knots, n_labels, base):
    """labels run_lookahead never reads: one plane of the last label"""
    return np.full((int(np.prod([len(k) for k in knots])), 1), base + n_labels - 1, dtype=np.int32)


def _axes(D):
    """(lookahead axes, flight axes): a proper subset of the axes from D = 2 on, and another one"""
    look = [0, D - 1] if D >= 3 else [D - 1]
    fly = sorted({D // 2, 1 % D}) if D != 2 else [0]
    return look, fly


def _flight_set(rng, D, axes, W=4):
    F = np.zeros((D, W))
    for a in axes:
        F[a] = rng.uniform(-0.15, 0.15, size=W)
    F[axes[0], 1] = 0.0
    return F, rng.uniform(0.2, 1.0, size=W)


def _drawn(Pf, W, n, K, seed, first):
    import hjbdp
    return hjbdp.noise_draw(hjbdp.noise_thresholds(Pf, W), n, K, seed=seed, first_stream=first)


# ---- 1. every instantiation against the host twin and the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("fly", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_every_instantiation_is_bit_equal_to_the_host_twin_and_the_restatement(built, D, dtype, fly):
    import hjbdp
    wide = np.dtype(dtype).itemsize == 8
    rng = np.random.default_rng(2700 + 10 * D + 2 * wide + fly)
    nu = (D - 1 + 2 * fly + wide) % 4 + 1                  # n_u cycles over 1..4
    mode = "expect" if (D + fly) % 2 else "worst"
    knots, ut, A, B, c, q, r, V = grefs.random_problem(rng, D, nu, 5, 3, dtype)
    X0 = grefs.starts(rng, knots, N_TRAJ)
    look_axes, fly_axes = _axes(D)
    E, P = refs.node_sets(rng, D, 3, look_axes, with_weights=(mode == "expect"))
    F, Pf = _flight_set(rng, D, fly_axes)
    seed, first = 77 + D, 1000
    kw = dict(nodes=_drawn(Pf, 4, N_TRAJ, len(PLANES), seed, first), flight_offsets=F) if fly else {}
    ref = refs.rollout(knots, ut, A, B, V, X0, PLANES, E, P, mode, c=c, q=q, r=r, index_base=1, **kw)
    check_bits(hjbdp.lookahead_host(knots, ut, A, B, V, X0, PLANES, E, P, mode, c=c, q=q, r=r, index_base=1, keep_path=True, **kw), ref,
               "host twin")
    assert not (ref[4] - 1 == 4).any()                     # row 4 of u_table duplicates row 2: the tie goes to the lower label
    lo = np.array([k[0] for k in knots])
    hi = np.array([k[-1] for k in knots])
    assert ((ref[2] < lo[None, :, None]) | (ref[2] > hi[None, :, None])).any()      # (flights did leave the grid)
    with hjbdp.Rollout(knots, _labels_stub(knots, 5, 1), ut, index_base=1) as ro:
        ro.set_model(A, B, c=c, q=q, r=r)
        ro.set_values(V)
        ro.set_lookahead(E, P, mode)
        ro.set_noise(F, Pf)                                # held in the nominal runs too: they must not read it
        for lds in (1, 0):
            ro.set_option("lds", lds)
            out = ro.run_lookahead(X0, PLANES, noisy=fly, seed=seed, first_stream=first, keep_path=True)
            check_bits(out, ref, (lds, "kernel"))
            if fly:
                assert np.array_equal(out["W_path"], kw["nodes"]) and len(np.unique(out["W_path"])) == 4
            else:
                assert out["W_path"] is None
        lean = ro.run_lookahead(X0, PLANES, noisy=fly, seed=seed, first_stream=first)
        assert lean["X_path"] is None and lean["L_path"] is None and lean["V_path"] is None and lean["W_path"] is None
        assert _same(lean["X_final"], ref[0]) and _same(lean["cost"], ref[1])


@pytest.mark.parametrize("W", [1, 2, 128])
def test_node_counts_at_d2(built, W):
    import hjbdp
    rng = np.random.default_rng(2790 + W)
    knots, ut, A, B, c, q, r, V = grefs.random_problem(rng, 2, 2, 5, 3, np.float64)
    X0 = grefs.starts(rng, knots, N_TRAJ)
    for mode in ("expect", "worst"):
        E, P = refs.node_sets(rng, 2, W, [1], with_weights=(mode == "expect"))
        F, Pf = _flight_set(rng, 2, [0], W=W if W > 1 else 2)
        nodes = _drawn(Pf, F.shape[1], N_TRAJ, len(PLANES), 9, 0)
        ref = refs.rollout(knots, ut, A, B, V, X0, PLANES, E, P, mode, c=c, q=q, r=r, index_base=1, nodes=nodes, flight_offsets=F)
        with hjbdp.Rollout(knots, _labels_stub(knots, 5, 1), ut, index_base=1) as ro:
            ro.set_model(A, B, c=c, q=q, r=r)
            ro.set_values(V)
            ro.set_lookahead(E, P, mode)
            ro.set_noise(F, Pf)
            for lds in (1, 0):
                ro.set_option("lds", lds)
                check_bits(ro.run_lookahead(X0, PLANES, noisy=True, seed=9, keep_path=True), ref, (W, mode, lds))


# ---- 2. identities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_one_zero_node_is_run_greedy(built, D):
    import hjbdp
    rng = np.random.default_rng(2720 + D)
    dtype = np.float32 if D % 2 else np.float64
    knots, ut, A, B, c, q, r, V = grefs.random_problem(rng, D, (D - 1) % 4 + 1, 5, 3, dtype)
    X0 = grefs.starts(rng, knots, N_TRAJ)
    zero = np.zeros((D, 1))
    zero[D - 1, 0] = -0.0
    with hjbdp.Rollout(knots, _labels_stub(knots, 5, 1), ut, index_base=1) as ro:
        ro.set_model(A, B, c=c, q=q, r=r)
        ro.set_values(V)
        want = ro.run_greedy(X0, PLANES, keep_path=True)
        ro.set_noise(zero, None)
        for mode, P in (("expect", [1.0]), ("worst", None)):
            ro.set_lookahead(zero, P, mode)
            for noisy in (False, True):                    # one zero node in both sets, flown "noisy": still run_greedy
                got = ro.run_lookahead(X0, PLANES, noisy=noisy, seed=3, keep_path=True)
                for name in NAMES:
                    assert _same(got[name], want[name]), (mode, noisy, name)
                assert got["L_path"].dtype == np.int32
                assert (got["W_path"] is None) if not noisy else not got["W_path"].any()


def test_streams_count_through_the_call_and_chunks_change_no_bit(built):
    import hjbdp
    rng = np.random.default_rng(2731)
    knots, ut, A, B, c, q, r, V = grefs.random_problem(rng, 3, 2, 5, 3, np.float64)
    n = 150
    X0 = grefs.starts(rng, knots, 2 * n)
    E, P = refs.node_sets(rng, 3, 3, [0, 2])
    F, Pf = _flight_set(rng, 3, [1])
    keys = NAMES + ("W_path",)
    with hjbdp.Rollout(knots, _labels_stub(knots, 5, 1), ut, index_base=1) as ro:
        ro.set_model(A, B, c=c, q=q, r=r)
        ro.set_values(V)
        ro.set_lookahead(E, P)
        ro.set_noise(F, Pf)
        whole = ro.run_lookahead(X0, PLANES, noisy=True, seed=41, first_stream=500, keep_path=True)
        assert np.array_equal(whole["W_path"], _drawn(Pf, 4, 2 * n, len(PLANES), 41, 500))      # W_path is hjb_rollout_noise_draw
        halves = [ro.run_lookahead(X0[:, i * n:(i + 1) * n], PLANES, noisy=True, seed=41, first_stream=500 + i * n, keep_path=True)
                  for i in (0, 1)]
        for key in keys:
            axis = 1 if key == "X_final" else 0
            assert _same(np.concatenate([h[key] for h in halves], axis=axis), whole[key]), key
        ro.set_option("chunk", 100)                        # 3 chunks: 100 + 100 + 100
        chunked = ro.run_lookahead(X0, PLANES, noisy=True, seed=41, first_stream=500, keep_path=True)
        nominal_chunked = ro.run_lookahead(X0, PLANES, keep_path=True)
        ro.set_option("chunk", 1 << 20)
        nominal = ro.run_lookahead(X0, PLANES, keep_path=True)
        for key in keys:
            assert _same(chunked[key], whole[key]), key
        for key in NAMES:
            assert _same(nominal_chunked[key], nominal[key]), key
        assert not _same(nominal["X_final"], whole["X_final"])


# ---- 3. one step at every grid node is the disturbed backup --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["expect", "worst"])
@pytest.mark.parametrize("which", ["axis1_3", "both_5"])
def test_one_step_at_every_grid_node_is_the_disturbed_backup(built, which, mode):
    """Dynamic_Solver's float64 terms are summed in K16's order and K24 combines the nodes as the lookahead does, so a candidate
    at a grid node is the disturbed backup's candidate bit for bit: label and minimum of a one-step run on plane k + 1 are
    idx_stages[:, k] and J_stages[:, k].  The edge nodes put offset next states outside the grid on both sides."""
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.dx, ds.du, ds.N = 13, 17, 6
    ds.build_spec()
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    h = s_r[1] - s_r[0]
    if which == "axis1_3":
        off = np.array([[0.0, 0.0, 0.0], [-0.7 * h, 0.0, 0.45 * h]])
        w = np.array([0.25, 0.5, 0.25])
    else:
        off = np.array([[0.3 * h, -0.6 * h, 0.0, 1.2 * h, -0.1 * h], [-0.7 * h, 0.25 * h, 0.0, -0.2 * h, 1.1 * h]])
        w = np.array([0.1, 0.2, 0.4, 0.2, 0.1])
    ds.disturbance = (off, w if mode == "expect" else None, mode)
    spec = ds.build_spec()
    n_st = ds.N - 1
    with hjbdp.Backup(spec) as bk:
        assert bk.info()["kernel_variant"] == 8
        out = bk.solve(n_st, keep_J=True, keep_idx=True)
    J, idx = out["J_stages"], out["idx_stages"]
    nodes = np.array([[s_r[i], s_r[j]] for j in range(13) for i in range(13)]).T           # axis 0 fastest, as the planes
    with hjbdp.Rollout([s_r, s_r], idx, np.asarray(ds._U_mesh, dtype=np.float64), index_base=1) as ro:
        ro.set_model(ds.A, ds.B, q=np.diag(ds.Q), r=[ds.R])
        ro.set_values(J)
        ro.set_lookahead(off, w if mode == "expect" else None, mode)
        for k in range(n_st):
            got = ro.run_lookahead(nodes, [k + 1 if k + 1 < n_st else -1], keep_path=True)
            assert np.array_equal(got["L_path"][:, 0], idx[:, k].astype(np.int32)), k
            assert _same(got["V_path"][:, 0], J[:, k]), k
        plain = ro.run_greedy(nodes, [1], keep_path=True)
        assert not _same(plain["V_path"][:, 0], J[:, 0])                                   # (the nodes do change the values)
    assert len(np.unique(idx)) > 1                                                         # (the argmin is not one label everywhere)


# ---- 4. design, fly, compare on the exactly posed noisy lattice ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["expect", "worst"])
def test_lattice_lookahead_under_noise_is_the_stored_labels_noisy_loop(built, mode):
    import hjbdp
    K = nrefs.LATTICE_STAGES
    with hjbdp.Backup(nrefs.lattice_spec(mode)) as bk:
        sol = bk.solve(K, keep_J=True, keep_idx=True)
    J = sol["J_stages"].reshape(33, K, order="F")
    idx = sol["idx_stages"].reshape(33, K, order="F")
    weights = nrefs.LATTICE_P if mode == "expect" else None
    X0 = np.repeat(nrefs.LATTICE_STARTS, 32).reshape(1, -1)                                # 288 trajectories
    seed = 2027
    with hjbdp.Rollout([nrefs.LATTICE_KNOTS], idx, nrefs.LATTICE_U, index_base=0) as ro:
        ro.set_model([[1.0]], [[1.0]], q=[1.0], r=[0.5])
        ro.set_noise(nrefs.LATTICE_NODES, weights)
        ro.set_values(J)
        ro.set_lookahead(nrefs.LATTICE_NODES, weights, mode)
        stored = ro.run_noisy(X0, np.arange(K), seed=seed, method="nearest", keep_path=True)
        look = ro.run_lookahead(X0, list(range(1, K)) + [-1], noisy=True, seed=seed, keep_path=True)
    for key in ("X_path", "U_path", "cost", "W_path", "X_final"):
        assert _same(look[key], stored[key]), key
    start = (X0[0] + 16).astype(np.int64)
    assert _same(look["V_path"][:, 0], J[start, 0])                                        # what the controller believed: J_1
    Xp = look["X_path"]
    assert np.array_equal(Xp, np.round(Xp)) and np.abs(Xp).max() <= 16                      # every visited state a knot inside the grid
    assert len(np.unique(look["W_path"])) == 3 and len(np.unique(look["U_path"])) == 3
    node = (Xp[:, 0, :].astype(np.int64) + 16)
    for k in range(K):
        assert np.array_equal(look["L_path"][:, k], idx[node[:, k], k].astype(np.int32)), k
        assert _same(look["V_path"][:, k], J[node[:, k], k]), k


# ---- 5. isolation and refusals with a device -----------------------------------------------------------------------------------------
def _raw_run(ro, fly, planes, X0, first_stream=0, with_W=False):
    """hjb_rollout_run_lookahead through ctypes on sentinel-filled outputs -> (status, the outputs)"""
    planes = np.ascontiguousarray(planes, dtype=np.int32)
    X = np.ascontiguousarray(np.asarray(X0, dtype=np.float64).T)
    nt, D = X.shape
    K, nu = int(planes.size), ro.n_u
    out = {"X_final": np.full((nt, D), SENT), "cost": np.full(nt, SENT), "X_path": np.full(nt * D * (K + 1), SENT),
           "U_path": np.full(nt * nu * K, SENT), "L_path": np.full(nt * K, SENT), "V_path": np.full(nt * K, SENT),
           "W_path": np.full(nt * K, SENT)}
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ms = C.c_double(SENT)
    st = ro.lib.hjb_rollout_run_lookahead(ro._ro, fly, K, planes.ctypes.data_as(C.POINTER(C.c_int32)), nt, f(X), 5, first_stream,
                                          f(out["X_final"]), f(out["cost"]), f(out["X_path"]), f(out["U_path"]), f(out["L_path"]),
                                          f(out["V_path"]), f(out["W_path"]) if with_W else None, C.byref(ms))
    out["device_ms"] = np.array([ms.value])
    return st, out


def _untouched(out):
    return all((a == SENT).all() for a in out.values())


def test_the_lookahead_set_is_read_by_run_lookahead_alone_and_refusals(built):
    import hjbdp
    from hjbdp import _abi
    from test_gpu_rollout import _random_problem
    rng = np.random.default_rng(274)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 3, 2, np.uint16, 9, 4)
    lo = np.array([k[0] for k in knots]) - 0.1
    hi = np.array([k[-1] for k in knots]) + 0.1
    X0 = rng.uniform(lo[:, None], hi[:, None], size=(3, N_TRAJ))
    planes = rng.integers(0, 4, size=6)
    nS = int(np.prod([len(k) for k in knots]))
    V = rng.uniform(0, 1, size=(nS, 2))
    off, p = rng.uniform(-0.2, 0.2, size=(3, 5)), rng.uniform(0.1, 1.0, size=5)
    E, P = refs.node_sets(rng, 3, 3, [0, 2])
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=np.ones(3), r=[0.5, 0.25])
        ro.set_values(V)
        # no lookahead set: refused, outputs untouched
        st, out = _raw_run(ro, 0, [0, 1], X0)
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "before hjb_rollout_set_lookahead" in ro.lib.hjb_rollout_last_error(ro._ro).decode()
        ro.set_lookahead(E, P)
        # fly_noise = 1 without a noise set
        st, out = _raw_run(ro, 1, [0, 1], X0, with_W=True)
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "before hjb_rollout_set_noise" in ro.lib.hjb_rollout_last_error(ro._ro).decode()
        ro.clear_lookahead()
        ro.set_noise(off, p)
        before = (ro.run(X0, planes, keep_path=True), ro.run_noisy(X0, planes, seed=5, keep_path=True), ro.run_greedy(X0, [1, 0, -1], keep_path=True))
        ro.set_lookahead(E, P)
        during = (ro.run(X0, planes, keep_path=True), ro.run_noisy(X0, planes, seed=5, keep_path=True), ro.run_greedy(X0, [1, 0, -1], keep_path=True))
        look = ro.run_lookahead(X0, [1, 0, -1], keep_path=True)
        check_bits(look, refs.rollout(knots, ut, A, B, V, X0, [1, 0, -1], E, P, c=c, q=np.ones(3), r=[0.5, 0.25], index_base=base))
        for a, b in zip(during, before):
            for key in a:
                if key != "device_ms" and a[key] is not None:
                    assert _same(a[key], b[key]), key
        assert not _same(look["V_path"], before[2]["V_path"])
        # the remaining refusals, each with the outputs untouched
        for args, text in (((0, [0], X0, 0, True), "W_path given with fly_noise=0"), ((1, [0], X0, -1, True), "first_stream=-1 < 0"),
                           ((2, [0], X0, 0, False), "fly_noise=2"), ((0, [2], X0, 0, False), "outside [-1, 2)"),
                           ((1, [0, -2], X0, 0, True), "outside [-1, 2)")):
            st, out = _raw_run(ro, *args)
            assert st == _abi.HJB_E_INVALID and _untouched(out), args
            assert text in ro.lib.hjb_rollout_last_error(ro._ro).decode(), (args, ro.lib.hjb_rollout_last_error(ro._ro).decode())
        bad = X0.copy()
        bad[2, 17] = np.inf
        st, out = _raw_run(ro, 1, [0], bad, with_W=True)
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "not finite" in ro.lib.hjb_rollout_last_error(ro._ro).decode()
        ro.clear_values()
        st, out = _raw_run(ro, 0, [0], X0)
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "hjb_rollout_set_values" in ro.lib.hjb_rollout_last_error(ro._ro).decode()
        st, out = _raw_run(ro, 0, [-1], X0)                                                # only -1: needs no values
        assert st == _abi.HJB_OK and not (out["X_final"] == SENT).any() and (out["W_path"] == SENT).all()
        # the set's own refusals with an object: the set it holds stays
        for args in ((off[:, :2], [0.5, -0.5], "expect"), (np.array([[0.0], [np.nan], [0.0]]), None, "expect")):
            with pytest.raises(ValueError):
                ro.set_lookahead(*args)
        d = (C.c_double * 6)(0.0, 0.0, float("inf"), 0.0, 0.0, 0.0)
        assert ro.lib.hjb_rollout_set_lookahead(ro._ro, 0, 2, d, None) == _abi.HJB_E_INVALID
        assert "offset of axis 2, node 0 is not finite" in ro.lib.hjb_rollout_last_error(ro._ro).decode()
        again = ro.run_lookahead(X0, [-1, -1], keep_path=True)
        assert _same(again["X_final"], ro.run_greedy(X0, [-1, -1])["X_final"])
    # an object without a model, and one with another model
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_values(V)
        ro.set_lookahead(E, P)
        st, out = _raw_run(ro, 0, [0], X0)
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "before hjb_rollout_set_model" in ro.lib.hjb_rollout_last_error(ro._ro).decode()
    knots6 = [np.linspace(-1, 1, 3)] * 6
    labels6 = rng.integers(1, 4, size=(3 ** 6, 1)).astype(np.uint8)
    with hjbdp.Rollout(knots6, labels6, rng.uniform(-1, 1, size=(3, 3)), index_base=1) as ro:
        ro.set_attitude_model([1.0, 2.0, 3.0], 0.01)
        ro.set_values(np.zeros((3 ** 6, 1)))
        ro.set_lookahead(np.zeros((6, 1)))
        st, out = _raw_run(ro, 0, [0], np.zeros((6, 2)))
        assert st == _abi.HJB_E_INVALID and _untouched(out) and "needs the affine model" in ro.lib.hjb_rollout_last_error(ro._ro).decode()


# ---- 6. the mirror ----------------------------------------------------------------------------------------------------------------------
def test_dynamic_solver_get_lookahead_paths(built):
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.dx, ds.du, ds.N = 13, 17, 6
    off, w = hjbdp.gaussian_nodes([0.02, 0.05], order=3)
    ds.disturbance = (off, w, "expect")
    ds.run()
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    X0 = np.array([[s_r[0], s_r[0]], [s_r[6], s_r[8]], [s_r[12], s_r[12]], [2.0, 1.0], [0.3, -0.7]]).T
    X, U = ds.get_lookahead_paths(X0)
    assert X.shape == (2, 6, 5) and U.shape == (6, 5) and not U[5].any()
    assert ds.lookahead_cost.shape == (5,) and ds.lookahead_paths_ms > 0
    cost = ds.get_lookahead_paths(X0, n_samples=8, seed=6)
    assert cost.shape == (5, 8)
    assert np.array_equal(ds.lookahead_cost_mean, cost.mean(axis=1)) and np.array_equal(ds.lookahead_cost_max, cost.max(axis=1))
    assert np.array_equal(ds.lookahead_cost_std, cost.std(axis=1)) and np.all(ds.lookahead_cost_std > 0)
    ut = np.asarray(ds._U_mesh, dtype=np.float64)
    planes = np.arange(1, 6)
    with hjbdp.Rollout([s_r, s_r], ds.u_star_idxs, ut, index_base=1) as ro:
        ro.set_model(ds.A, ds.B, q=np.diag(ds.Q), r=[ds.R])
        ro.set_values(ds.J_star)
        ro.set_lookahead(off, w, "expect")
        ro.set_noise(off, w)
        direct = ro.run_lookahead(X0, planes, keep_path=True)
        assert _same(X, direct["X_path"].transpose(1, 2, 0)) and _same(U[:5], direct["U_path"][:, 0, :].T)
        assert _same(ds.lookahead_cost, direct["cost"])
        for i in range(5):                                 # sample j of start i on stream i * n_samples + j
            by_hand = ro.run_lookahead(np.repeat(X0[:, i:i + 1], 8, axis=1), planes, noisy=True, seed=6, first_stream=8 * i)
            assert _same(by_hand["cost"], cost[i]), i
    frozen, _ = ds.get_lookahead_paths(X0, mode="ssu", ssu_num=2)
    assert frozen.shape == X.shape and not _same(frozen, X)
    ds.disturbance = None
    with pytest.raises(RuntimeError):
        ds.get_lookahead_paths(X0)
