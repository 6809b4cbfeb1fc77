"""GPU tests of the greedy rollout (hjb_rollout_set_values / hjb_rollout_run_greedy, csrc/kernels_rollout_greedy.h: K26;
hjbdp.Rollout.run_greedy, Dynamic_Solver.get_greedy_paths): every instantiation bit-equal to the host twin and to
tests/greedy_rollout_refs.py at the wave and block edges, chunked, staged and not; one step of the lookahead against the
Bellman backup it restates, at every grid node; closed loops on two exactly posed lattice problems against the stored labels;
and that the values are read by run_greedy alone."""
import numpy as np
import pytest

import greedy_rollout_refs as refs
from test_rollout_greedy_abi import NAMES, _same, check_bits

pytestmark = pytest.mark.gpu

EDGES = (1, 63, 64, 65, 257)         # one lane, a wave less one, a wave, a wave and one, a 256-thread block and one


def _slice(ref, n):
    """the restatement's outputs of the first n trajectories (they are independent)"""
    Xf, cost, Xp, Up, Lp, Vp = ref
    return Xf[:, :n], cost[:n], Xp[:n], Up[:n], Lp[:n], Vp[:n]


def _labels_stub(knots, n_labels, base):
    """labels run_greedy never reads: one plane of the last label"""
    return np.full((int(np.prod([len(k) for k in knots])), 1), base + n_labels - 1, dtype=np.int32)


# ---- 1. every instantiation against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_every_instantiation_is_bit_equal_to_the_host_twin_and_the_restatement(built, D, dtype):
    import hjbdp
    rng = np.random.default_rng(2600 + 10 * D + np.dtype(dtype).itemsize)
    for (nu, nl, with_c), base in zip(((1, 7, True), (4, 2, False), (2, 1, True), (4, 7, False)), (1, 0, 1, 0)):
        knots, ut, A, B, c, q, r, V = refs.random_problem(rng, D, nu, nl, 3, dtype)
        X0 = refs.starts(rng, knots, 257)
        planes = [2, 0, 0, -1, 1, -1, 2]                               # 7 steps: a repeated plane, the zero function twice
        cc = c if with_c else None
        ref = refs.rollout(knots, ut, A, B, V, X0, planes, c=cc, q=q, r=r, index_base=base)
        ref1 = refs.rollout(knots, ut, A, B, V, X0, planes[:1], c=cc, q=q, r=r, index_base=base)
        check_bits(hjbdp.greedy_host(knots, ut, A, B, V, X0, planes, c=cc, q=q, r=r, index_base=base, keep_path=True), ref, "host twin")
        lo = np.array([k[0] for k in knots])
        hi = np.array([k[-1] for k in knots])
        assert ((ref[2] < lo[None, :, None]) | (ref[2] > hi[None, :, None])).any()      # (flights did leave the grid)
        with hjbdp.Rollout(knots, _labels_stub(knots, nl, base), ut, index_base=base) as ro:
            ro.set_model(A, B, c=cc, q=q, r=r)
            ro.set_values(V)
            for lds in (1, 0):
                ro.set_option("lds", lds)
                for n in EDGES:
                    check_bits(ro.run_greedy(X0[:, :n], planes, keep_path=True), _slice(ref, n), (lds, n))
                check_bits(ro.run_greedy(X0, planes[:1], keep_path=True), ref1, (lds, "one step"))
                lean = ro.run_greedy(X0, planes)
                assert lean["X_path"] is None and lean["L_path"] is None and lean["V_path"] is None
                assert _same(lean["X_final"], ref[0]) and _same(lean["cost"], ref[1])
                ro.set_option("chunk", 100)                            # 100 + 100 + 57
                check_bits(ro.run_greedy(X0, planes, keep_path=True), ref, (lds, "chunk"))
                ro.set_option("chunk", 1 << 20)


def test_a_table_too_large_for_lds_falls_back_to_global_memory(built):
    """1100 labels of 4 controls are 35,200 bytes: beyond the 32 KiB rule, so option "lds" = 1 runs the global-memory form too"""
    import hjbdp
    rng = np.random.default_rng(26)
    knots, ut, A, B, c, q, r, V = refs.random_problem(rng, 2, 4, 1100, 2, np.float64)
    assert ut.size * 8 > 32 << 10
    X0 = refs.starts(rng, knots, 65)
    ref = refs.rollout(knots, ut, A, B, V, X0, [1, 0], c=c, q=q, r=r, index_base=1)
    assert len(np.unique(ref[4])) > 8                                  # (the minimum moves through the table)
    with hjbdp.Rollout(knots, _labels_stub(knots, 1100, 1), ut, index_base=1) as ro:
        ro.set_model(A, B, c=c, q=q, r=r)
        ro.set_values(V)
        for lds in (1, 0):
            ro.set_option("lds", lds)
            check_bits(ro.run_greedy(X0, [1, 0], keep_path=True), ref, lds)


def test_l_path_and_v_path_each_on_its_own_chunked_and_not(built):
    """hjb_rollout_run_greedy through ctypes (hjbdp.Rollout.run_greedy asks for L_path and V_path together or not at all): L_path
    only, V_path only, both and neither, at chunk = 100 (100 + 100 + 57) and unchunked.  Every array asked for is bit-equal to
    run_greedy(keep_path=True)'s; one not asked for keeps the sentinel it was filled with."""
    import ctypes as C
    import hjbdp
    SENT = -12345.678
    rng = np.random.default_rng(2627)                                  # (a seed at which the chosen labels vary: asserted below)
    knots, ut, A, B, c, q, r, V = refs.random_problem(rng, 2, 2, 7, 3, np.float64)
    X0 = refs.starts(rng, knots, 257)
    planes = np.array([2, 0, -1, 1, 1], dtype=np.int32)
    nt, K = 257, int(planes.size)
    X = np.ascontiguousarray(X0.T, dtype=np.float64)
    f64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    with hjbdp.Rollout(knots, _labels_stub(knots, 7, 1), ut, index_base=1) as ro:
        ro.set_model(A, B, c=c, q=q, r=r)
        ro.set_values(V)
        full = ro.run_greedy(X0, planes, keep_path=True)
        assert len(np.unique(full["L_path"])) > 1 and len(np.unique(full["V_path"])) > 1        # (neither path is constant)
        for chunk in (100, 1 << 20):
            ro.set_option("chunk", chunk)
            for want in (("L_path",), ("V_path",), ("L_path", "V_path"), ()):
                out = {"X_final": np.full((nt, 2), SENT), "cost": np.full(nt, SENT), "X_path": np.full(nt * 2 * (K + 1), SENT),
                       "U_path": np.full(nt * 2 * K, SENT), "L_path": np.full(nt * K, SENT), "V_path": np.full(nt * K, SENT)}
                opt = lambda key: f64p(out[key]) if key in want else None
                st = ro.lib.hjb_rollout_run_greedy(ro._ro, K, planes.ctypes.data_as(C.POINTER(C.c_int32)), nt, f64p(X),
                                                   f64p(out["X_final"]), f64p(out["cost"]), f64p(out["X_path"]), f64p(out["U_path"]),
                                                   opt("L_path"), opt("V_path"), None)
                assert st == 0, (chunk, want)
                assert _same(out["X_final"].T, full["X_final"]) and _same(out["cost"], full["cost"]), (chunk, want)
                assert _same(out["X_path"].reshape((nt, 2, K + 1), order="F"), full["X_path"]), (chunk, want)
                assert _same(out["U_path"].reshape((nt, 2, K), order="F"), full["U_path"]), (chunk, want)
                for key in ("L_path", "V_path"):
                    got = out[key].reshape((nt, K), order="F")
                    if key in want:
                        assert _same(got, full[key].astype(np.float64)), (chunk, want, key)
                    else:
                        assert (got == SENT).all(), (chunk, want, key)


# ---- 2. one step of the lookahead is the Bellman backup -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, None])
def test_one_step_at_every_grid_node_is_the_backup(built, variant):
    """Dynamic_Solver's float64 terms are summed in K16's order, so a candidate at a grid node is the generic backup's candidate
    bit for bit: label and minimum of a one-step greedy run on plane k + 1 are idx_stages[:, k] and J_stages[:, k]."""
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.dx, ds.du, ds.N = 13, 17, 6
    spec = ds.build_spec()
    n_st = ds.N - 1
    with hjbdp.Backup(spec, variant=variant) as bk:
        assert variant is None or bk.info()["kernel_variant"] == 0
        out = bk.solve(n_st, keep_J=True, keep_idx=True)
    J, idx = out["J_stages"], out["idx_stages"]
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    nodes = np.array([[s_r[i], s_r[j]] for j in range(13) for i in range(13)]).T           # axis 0 fastest, as the planes
    with hjbdp.Rollout([s_r, s_r], idx, np.asarray(ds._U_mesh, dtype=np.float64), index_base=1) as ro:
        ro.set_model(ds.A, ds.B, q=np.diag(ds.Q), r=[ds.R])
        ro.set_values(J)
        for k in range(n_st):
            got = ro.run_greedy(nodes, [k + 1 if k + 1 < n_st else -1], keep_path=True)
            assert np.array_equal(got["L_path"][:, 0], idx[:, k].astype(np.int32)), k
            assert _same(got["V_path"][:, 0], J[:, k]), k
    assert len(np.unique(idx)) > 1                                     # (the argmin is not one label everywhere)


# ---- 3. closed loops on the exactly posed lattice problems -------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2])
def test_lattice_closed_loop_is_the_stored_labels_loop_and_pays_what_j_promises(built, D):
    import hjbdp
    P = refs.LATTICE1 if D == 1 else refs.LATTICE2
    K, X0, knots = P["stages"], P["starts"], P["knots"]
    with hjbdp.Backup(refs.lattice_spec(D)) as bk:
        out = bk.solve(K, keep_J=True, keep_idx=True)
    J, idx = out["J_stages"], out["idx_stages"]
    with hjbdp.Rollout(knots, idx, refs.LATTICE_U, index_base=0) as ro:
        ro.set_model(P["A"], P["B"], q=P["q"], r=P["r"])
        ro.set_values(J)
        stored = ro.run(X0, np.arange(K), method="nearest", keep_path=True)
        greedy = ro.run_greedy(X0, list(range(1, K)) + [-1], keep_path=True)
    for key in ("X_path", "U_path", "cost", "X_final"):
        assert _same(greedy[key], stored[key]), key
    Xp = greedy["X_path"]                                                                  # [n, D, K + 1]
    assert np.array_equal(Xp, np.round(Xp))                                                # on grid nodes ...
    bound = (15,) if D == 1 else (12, 5)
    for a in range(D):
        assert np.abs(Xp[:, a, :]).max() <= bound[a]                                       # ... inside the grid
    node = sum((Xp[:, a, :].astype(np.int64) + 16) * 33 ** a for a in range(D))            # [n, K + 1] flat state of every visit
    assert _same(greedy["cost"], J[node[:, 0], 0])
    for k in range(K):
        assert _same(greedy["V_path"][:, k], J[node[:, k], k]), k
        assert np.array_equal(greedy["L_path"][:, k], idx[node[:, k], k].astype(np.int32)), k
    assert len(np.unique(greedy["U_path"])) == 3                                           # (all three controls were used)


# ---- 4. isolation ------------------------------------------------------------------------------------------------------------------
def test_values_are_read_by_run_greedy_alone(built):
    import hjbdp
    from test_gpu_rollout import _random_problem
    rng = np.random.default_rng(264)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 3, 2, np.uint16, 9, 4)
    lo = np.array([k[0] for k in knots]) - 0.1
    hi = np.array([k[-1] for k in knots]) + 0.1
    X0 = rng.uniform(lo[:, None], hi[:, None], size=(3, 300))
    planes = rng.integers(0, 4, size=6)
    nS = int(np.prod([len(k) for k in knots]))
    V = rng.uniform(0, 1, size=(nS, 2))
    off, p = rng.uniform(-0.2, 0.2, size=(3, 5)), rng.uniform(0.1, 1.0, size=5)
    keys = ("X_final", "cost", "X_path", "U_path")
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=np.ones(3), r=[0.5, 0.25])
        ro.set_noise(off, p)
        before = ro.run(X0, planes, keep_path=True)
        noisy_before = ro.run_noisy(X0, planes, seed=5, keep_path=True)
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_greedy(X0, [0])
        assert "hjb_rollout_set_values" in str(ei.value)
        zero = ro.run_greedy(X0, [-1, -1], keep_path=True)                                 # needs no values
        check_bits(zero, refs.rollout(knots, ut, A, B, None, X0, [-1, -1], c=c, q=np.ones(3), r=[0.5, 0.25], index_base=base))
        ro.set_values(V)
        during, noisy_during = ro.run(X0, planes, keep_path=True), ro.run_noisy(X0, planes, seed=5, keep_path=True)
        greedy = ro.run_greedy(X0, [1, 0, 1], keep_path=True)
        check_bits(greedy, refs.rollout(knots, ut, A, B, V, X0, [1, 0, 1], c=c, q=np.ones(3), r=[0.5, 0.25], index_base=base))
        for bad in ([2], [-2], [0, 1, 7]):
            with pytest.raises(hjbdp.HjbError) as ei:
                ro.run_greedy(X0, bad)
            assert "outside [-1, 2)" in str(ei.value)
        ro.clear_values()
        after, noisy_after = ro.run(X0, planes, keep_path=True), ro.run_noisy(X0, planes, seed=5, keep_path=True)
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_greedy(X0, [-1, 0])
        assert "hjb_rollout_set_values" in str(ei.value)
        for a, b in ((during, before), (after, before)):
            for key in keys:
                assert _same(a[key], b[key]), key
        for a in (noisy_during, noisy_after):
            for key in keys + ("W_path",):
                assert _same(a[key], noisy_before[key]), key
        assert not _same(greedy["X_final"][:, :3], before["X_final"][:, :3])
        # the other models' objects refuse it
        ro.set_values(V)
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_values(V)
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_greedy(X0, [0])
        assert "hjb_rollout_set_model" in str(ei.value)


def test_run_greedy_on_another_model_is_refused(built):
    import hjbdp
    rng = np.random.default_rng(3)
    knots = [np.linspace(-1, 1, 3)] * 6
    labels = rng.integers(1, 4, size=(3 ** 6, 1)).astype(np.uint8)
    with hjbdp.Rollout(knots, labels, rng.uniform(-1, 1, size=(3, 3)), index_base=1) as ro:
        ro.set_attitude_model([1.0, 2.0, 3.0], 0.01)
        ro.set_values(np.zeros((3 ** 6, 1)))
        out = np.full((6, 2), 7.0)
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_greedy(np.zeros((6, 2)), [0])
        assert "needs the affine model" in str(ei.value) and np.all(out == 7.0)


def test_dynamic_solver_greedy_paths(built):
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N, ds.dx, ds.du = 13, 35, 100
    ds.run()
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    at = [(0, 0), (17, 20), (34, 34), (5, 30)]
    X0 = np.array([[s_r[i], s_r[j]] for i, j in at] + [[2.0, 1.0], [0.3, -0.7]]).T
    X, U = ds.get_greedy_paths(X0)
    assert X.shape == (2, 13, 6) and U.shape == (13, 6) and not U[12].any()
    assert ds.greedy_cost.shape == (6,) and ds.greedy_paths_ms > 0
    for col, (i, j) in enumerate(at):
        assert U[0, col] == ds.u_star[i, j, 0], (i, j)                                     # on a node: the stored argmin
    u_table = np.asarray(ds._U_mesh, dtype=np.float64)
    kw = dict(q=np.diag(ds.Q), r=[ds.R], index_base=1)
    ref = refs.rollout([s_r, s_r], u_table, ds.A, ds.B, ds.J_star, X0, np.arange(1, 13), **kw)
    assert _same(X, ref[2].transpose(1, 2, 0)) and _same(U[:12], ref[3][:, 0, :].T) and _same(ds.greedy_cost, ref[1])
    # 'ssu' with ssu_num = 1 repeats plane 1
    Xs, Us = ds.get_greedy_paths(X0, mode="ssu", ssu_num=1)
    ref = refs.rollout([s_r, s_r], u_table, ds.A, ds.B, ds.J_star, X0, np.full(12, 1), **kw)
    assert _same(Xs, ref[2].transpose(1, 2, 0)) and _same(Us[:12], ref[3][:, 0, :].T)
    assert _same(Xs[:, :2], X[:, :2]) and not _same(Xs, X)
    with pytest.raises(ValueError):
        ds.get_greedy_paths(X0, mode="ssu", ssu_num=13)
    # the number the feature exists for: what the stored labels' loop pays beside the value function's own loop
    ds.get_optimal_paths(X0)
    assert np.all(np.isfinite(ds.paths_cost)) and np.all(np.isfinite(ds.greedy_cost))
