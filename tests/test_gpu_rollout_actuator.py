"""GPU tests of the actuator-noise rollout (hjb_rollout_set_actuator_noise / hjb_rollout_run_actuator,
csrc/kernels_rollout_actuator.h: K33; hjbdp.ActuatorRollout.run_actuator, Dynamic_Solver.get_actuator_paths / actuator_cost_map):
bit-equality with tests/actuator_rollout_refs.py at every instantiation, the contract's consequences (i) - (iv) - zero eps against
K25 and K16, the sampler's nodes and streams, one flown step on K32's query point, "promised equals paid" on the exactly posed
lattice problem - the LDS limit, validation and concurrency with a device, and the mirror."""
import ctypes as C
import threading

import numpy as np
import pytest

import actuator_rollout_refs as refs
from test_gpu_rollout import _diff, _random_problem, _same

pytestmark = pytest.mark.gpu

KEYS = ("X_final", "cost", "X_path", "U_path", "W_path")


def _check_bits(out, ref):
    Xf, cost, Xp, Up, Wp = ref
    assert _same(out["X_final"], Xf), _diff(out["X_final"], Xf)
    assert _same(out["cost"], cost), _diff(out["cost"], cost)
    if out["X_path"] is not None:
        assert _same(out["X_path"], Xp), _diff(out["X_path"], Xp)
        assert _same(out["U_path"], Up), _diff(out["U_path"], Up)
        assert out["W_path"].dtype == np.int32 and np.array_equal(out["W_path"], Wp)


def _equal_runs(a, b, keys=KEYS):
    for key in keys:
        assert (a[key] is None and b[key] is None) or _same(a[key], b[key]), key


def _signed_zeros(rng, shape):
    return np.where(rng.integers(0, 2, size=shape) == 0, 0.0, -0.0)


def _node_sets(rng, D):
    """(n_u, eps [W, n_u], base [D, W] or None, weights) for (n_u, W) = (1, 1), (4, 2), (2, 128).  The 4-input set has a dead
    input (an eps column of +-0 of both signs); from D = 2 on every base has an all-zero axis (both signs of zero) - at D = 1
    the W = 1 set has no base.  The W = 2 and W = 128 sets hold a zero-weight node, and the W = 128 base reaches +-0.6, beyond the
    0.1 the starts lie outside the grid by."""
    zero_axis = int(rng.integers(0, D))
    sets = []
    for nu, W, amp in ((1, 1, 0.05), (4, 2, 0.2), (2, 128, 0.6)):
        eps = rng.uniform(-1.0, 1.0, size=(W, nu))
        if nu == 4:
            eps[:, int(rng.integers(0, 4))] = [0.0, -0.0]
        base = rng.uniform(-amp, amp, size=(D, W))
        if D > 1:
            base[zero_axis] = _signed_zeros(rng, W)
        elif W == 1:
            base = None
        if W == 1:
            p = None
        elif W == 2:
            p = np.array([1.0, 3.0]) if D % 2 else np.array([0.0, 2.0])
        else:
            p = rng.uniform(0.0, 1.0, size=W)
            p[[0, 77, 127]] = 0.0
        sets.append((nu, eps, base, p))
    return sets


def _zeros_in_B(rng, B):
    """a B with zeros on some axis of some column, one of each sign where there is room"""
    B = B.copy()
    D, nu = B.shape
    B[int(rng.integers(0, D)), int(rng.integers(0, nu))] = 0.0
    if D * nu > 2:
        B[int(rng.integers(0, D)), int(rng.integers(0, nu))] = -0.0
    return B


# ---- 1. every instantiation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_every_instantiation_is_bit_equal_to_the_restatement(built, D, dtype):
    import hjbdp
    rng = np.random.default_rng(3300 + 100 * D + np.dtype(dtype).itemsize)
    left_grid = drew = 0
    for nu, eps, base_nodes, p in _node_sets(rng, D):
        knots, labels, ut, base, A, B, c = _random_problem(rng, D, nu, dtype, 7, 3)
        if nu > 1:
            B = _zeros_in_B(rng, B)
        lo = np.array([k[0] for k in knots])
        hi = np.array([k[-1] for k in knots])
        X0 = rng.uniform(lo[:, None] - 0.1, hi[:, None] + 0.1, size=(D, 300))      # two blocks, the second partial
        planes = rng.integers(0, 3, size=9)                                         # two Philox blocks and one word of a third
        q, r = rng.uniform(0, 1, size=D), rng.uniform(0, 1, size=nu)
        seed, first = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
        cc = c if nu == 4 else None
        with hjbdp.ActuatorRollout(knots, labels, ut, index_base=base) as ro:
            if nu == 2:
                ro.set_actuator_noise(eps, p, base_nodes)                           # the setters in either order: B is read at the run
                ro.set_model(A, B, c=cc, q=q, r=r)
            else:
                ro.set_model(A, B, c=cc, q=q, r=r)
                ro.set_actuator_noise(eps, p, base_nodes)
            for method in ("nearest", "linear"):
                ref = refs.rollout(knots, labels, ut, base, A, B, X0, planes, eps, p, base_nodes, seed, first, method, c=cc, q=q, r=r)
                for lds in (1, 0):
                    ro.set_option("lds", lds)
                    out = ro.run_actuator(X0, planes, seed=seed, first_stream=first, method=method, keep_path=True)
                    _check_bits(out, ref)
                    lean = ro.run_actuator(X0, planes, seed=seed, first_stream=first, method=method)
                    assert lean["X_path"] is None and lean["W_path"] is None
                    _equal_runs(lean, out, ("X_final", "cost"))
                assert np.isfinite(ref[1]).mean() > 0.5     # (far outside the grid the 'linear' lookup extrapolates as a degree-D polynomial)
                Xp, Wp = ref[2], ref[4]
                left_grid += int(((Xp < lo[None, :, None]) | (Xp > hi[None, :, None])).any(axis=(1, 2)).sum())
                if p is not None:
                    assert not np.isin(Wp, np.flatnonzero(p == 0)).any()
                    drew += len(np.unique(Wp))
    assert left_grid > 0 and drew > 60              # trajectories did leave the grid, and the 128-node set was really sampled


# ---- 2. consequence (i): eps all +-0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_zero_eps_is_k25_or_k16_and_no_other_run_reads_the_set(built, D):
    import hjbdp
    rng = np.random.default_rng(330 + D)
    knots, labels, ut, base, A, B, c = _random_problem(rng, D, 2, np.uint16, 9, 4)
    lo = np.array([k[0] for k in knots]) - 0.1
    hi = np.array([k[-1] for k in knots]) + 0.1
    X0 = rng.uniform(lo[:, None], hi[:, None], size=(D, 300))
    planes = rng.integers(0, 4, size=9)
    W = 7
    off, p = rng.uniform(-0.5, 0.5, size=(D, W)), rng.uniform(0.1, 1.0, size=W)
    zero = _signed_zeros(rng, (W, 2))
    T = hjbdp.noise_thresholds(p)
    with hjbdp.ActuatorRollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=np.ones(D), r=[0.5, 0.25])
        ro.set_noise(off, p)
        for method in ("linear", "nearest"):
            ro.clear_actuator_noise()
            k16 = ro.run(X0, planes, method=method, keep_path=True)
            k25 = ro.run_noisy(X0, planes, seed=99, first_stream=5, method=method, keep_path=True)
            k28 = ro.run_campaign(X0[:, :40], planes, 5, seed=99, first_stream=5, method=method, cost_threshold=1.0, settle_tol=0.5)
            with pytest.raises(hjbdp.HjbError) as ei:
                ro.run_actuator(X0, planes)
            assert "before hjb_rollout_set_actuator_noise" in str(ei.value)
            # zero eps with a base: K25 under set_noise(base, weights)
            ro.set_actuator_noise(zero, p, off)
            _equal_runs(ro.run_actuator(X0, planes, seed=99, first_stream=5, method=method, keep_path=True), k25)
            # zero eps alone, or with a base of +-0: K16, and W_path still the drawn nodes
            for b in (None, _signed_zeros(rng, (D, W))):
                ro.set_actuator_noise(zero, p, b)
                flown = ro.run_actuator(X0, planes, seed=99, first_stream=5, method=method, keep_path=True)
                _equal_runs(flown, k16, ("X_final", "cost", "X_path", "U_path"))
                assert np.array_equal(flown["W_path"], hjbdp.noise_draw(T, 300, 9, seed=99, first_stream=5))
            # an object that holds an actuator set: run, run_noisy and run_campaign give the bits they gave before
            ro.set_actuator_noise(rng.uniform(-0.9, 0.9, size=(W, 2)), p, off)
            moved = ro.run_actuator(X0, planes, seed=99, first_stream=5, method=method, keep_path=True)
            assert not _same(moved["X_final"], k25["X_final"]) and np.array_equal(moved["W_path"], k25["W_path"])
            _equal_runs(ro.run(X0, planes, method=method, keep_path=True), k16, ("X_final", "cost", "X_path", "U_path"))
            _equal_runs(ro.run_noisy(X0, planes, seed=99, first_stream=5, method=method, keep_path=True), k25)
            again = ro.run_campaign(X0[:, :40], planes, 5, seed=99, first_stream=5, method=method, cost_threshold=1.0, settle_tol=0.5)
            assert _same(again["stats"], k28["stats"])


# ---- 3. consequence (ii): the same sampler, global streams ----------------------------------------------------------------------
def test_nodes_are_noise_draws_and_streams_count_through_the_call(built):
    import hjbdp
    rng = np.random.default_rng(38)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 2, 2, np.uint8, 12, 4)
    lo = np.array([k[0] for k in knots]) - 0.1
    hi = np.array([k[-1] for k in knots]) + 0.1
    X0 = rng.uniform(lo[:, None], hi[:, None], size=(2, 600))
    planes = rng.integers(0, 4, size=9)
    eps, p = rng.uniform(-0.8, 0.8, size=(9, 2)), rng.uniform(0.1, 1.0, size=9)
    nodes = rng.uniform(-0.3, 0.3, size=(2, 9))
    kw = dict(c=c, q=[1.0, 0.5], r=[0.1, 0.2])
    T = hjbdp.noise_thresholds(p)
    with hjbdp.ActuatorRollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, **kw)
        ro.set_actuator_noise(eps, p, nodes)
        ro.set_noise(nodes, p)
        whole = ro.run_actuator(X0, planes, seed=12, keep_path=True)
        _check_bits(whole, refs.rollout(knots, labels, ut, base, A, B, X0, planes, eps, p, nodes, 12, 0, "linear", **kw))
        assert np.array_equal(whole["W_path"], hjbdp.noise_draw(T, 600, 9, seed=12, first_stream=0))
        # common random numbers across plants: the additive flight of the same seed draws the same nodes
        assert np.array_equal(ro.run_noisy(X0, planes, seed=12, keep_path=True)["W_path"], whole["W_path"])
        for chunk in (64, 192, 1 << 20):
            ro.set_option("chunk", chunk)
            _equal_runs(ro.run_actuator(X0, planes, seed=12, keep_path=True), whole)
        # 600 at stream 0 = 300 at stream 0, then 300 at stream 300
        halves = [ro.run_actuator(X0[:, i:i + 300], planes, seed=12, first_stream=i, keep_path=True) for i in (0, 300)]
        for key in ("cost", "X_path", "U_path", "W_path"):
            assert _same(np.concatenate([h[key] for h in halves], axis=0), whole[key]), key
        assert _same(np.concatenate([h["X_final"] for h in halves], axis=1), whole["X_final"])
        # the stream's second counter word changes inside the call, in one launch and across chunks
        first = 2 ** 32 - 100
        ref = refs.rollout(knots, labels, ut, base, A, B, X0[:, :300], planes, eps, p, nodes, 12, first, "linear", **kw)
        far = ro.run_actuator(X0[:, :300], planes, seed=12, first_stream=first, keep_path=True)
        _check_bits(far, ref)
        ro.set_option("chunk", 64)
        _check_bits(ro.run_actuator(X0[:, :300], planes, seed=12, first_stream=first, keep_path=True), ref)
        ro.set_option("chunk", 1 << 20)
        assert not np.array_equal(far["W_path"], whole["W_path"][:300])
        big_seed = ro.run_actuator(X0[:, :40], planes, seed=2 ** 64 - 1, keep_path=True)
        _check_bits(big_seed, refs.rollout(knots, labels, ut, base, A, B, X0[:, :40], planes, eps, p, nodes, 2 ** 64 - 1, 0, "linear", **kw))
        assert np.array_equal(big_seed["W_path"], hjbdp.noise_draw(T, 40, 9, seed=2 ** 64 - 1))


# ---- 4. consequence (iii): one flown step lands on K32's query -------------------------------------------------------------------
def test_one_step_from_a_grid_node_lands_on_the_backups_query(built):
    import hjbdp
    from control_disturbance_refs import ControlDisturbedRef
    eps, w = np.array([-0.3, -0.1, 0.0, 0.05, 0.2]), np.array([0.125, 0.25, 0.25, 0.25, 0.125])
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N, ds.dx, ds.du = 3, 9, 7
    ds.actuator_noise = (eps, w, "expect")
    ds.run()
    # the two-stage policy of this problem is one control everywhere: fly a policy that uses all 7 (the contract holds for any
    # label l at x: the backup evaluates every candidate)
    ds.u_star_idxs = np.random.default_rng(32).integers(1, 8, size=(9, 9, 2)).astype(np.int32)
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    ut = np.asarray(ds._U_mesh, dtype=np.float64)
    base = np.array([[0.0, -0.0, 0.0, 0.0, -0.0], [0.01, -0.02, 0.0, 0.015, -0.005]])      # an additive set on the same nodes, axis 0 all zero
    off = hjbdp.actuator_nodes(ds.B, ut, eps, base=base)[0]                                 # [2, 5, 7]
    M = 64
    grid = np.stack([np.tile(s_r, 9), np.repeat(s_r, 9)])                                   # state i + 9 j, axis 0 fastest
    with hjbdp.ActuatorRollout([s_r, s_r], ds.u_star_idxs, ut, index_base=1) as ro:
        ro.set_model(ds.A, ds.B, q=np.diag(ds.Q), r=[ds.R])
        ro.set_actuator_noise(eps, w, base)
        out = ro.run_actuator(np.repeat(grid, M, axis=1), [0], seed=3, method="nearest", keep_path=True)
    states = np.repeat(np.arange(81), M)
    lab0 = np.asarray(ds.u_star_idxs)[:, :, 0].reshape(-1, order="F").astype(np.int64)[states] - 1
    assert np.array_equal(out["U_path"][:, 0, 0], ut[lab0])
    Wp = out["W_path"][:, 0]
    assert len(np.unique(Wp)) == 5 and len(np.unique(lab0)) == 7
    x0, x1, u = np.repeat(grid, M, axis=1)[0], np.repeat(grid, M, axis=1)[1], ut[lab0]
    for a in range(2):
        q = ds.A[a, 0] * x0 + ds.A[a, 1] * x1 + ds.B[a, 0] * u                              # the next-state terms, left to right
        assert _same(out["X_path"][:, a, 1], q + off[a, Wp, lab0]), a
    # ... and they are the points x_next + d_w(l) the backup's restatement forms for (x, l, w)
    spec = ds.build_spec()
    ref = ControlDisturbedRef(spec, off, w, "expect")
    _, q, _, _ = ref.locate(states, lab0)
    for a in range(2):
        want = np.stack([ref._node_query(q, a, wn, lab0) for wn in range(5)])[Wp, np.arange(states.size)]
        assert _same(out["X_path"][:, a, 1], want), a


# ---- 5. the LDS limit ----------------------------------------------------------------------------------------------------------------
def test_node_block_that_pushes_the_tables_past_the_lds_limit(built):
    """[knots | 1/dx | u_table] of 4008 doubles fit 32 KiB alone; the 128-node block (127 + 2 x 128 doubles) does not fit behind
    them: the library runs the global-memory form - the bits of the forced one (option "lds" = 0) and of the restatement.  With 9
    nodes (8 + 2 x 9 doubles: 4034 in all) the same object stays in LDS."""
    import hjbdp
    rng = np.random.default_rng(331)
    knots = [np.linspace(-1.0, 1.0, 4)]
    labels = rng.integers(0, 4000, size=(4, 2)).astype(np.int32)
    ut = rng.uniform(-1, 1, size=(4000, 1))
    X0 = rng.uniform(-1.1, 1.1, size=(1, 300))
    planes = [0, 1, 1, 0, 1]
    with hjbdp.ActuatorRollout(knots, labels, ut, index_base=0) as ro:
        ro.set_model([[0.5]], [[0.05]], q=[1.0], r=[1.0])
        for W in (128, 9):
            eps, nodes, p = rng.uniform(-0.9, 0.9, size=W), rng.uniform(-0.3, 0.3, size=(1, W)), rng.uniform(0.1, 1.0, size=W)
            ro.set_actuator_noise(eps, p, nodes)
            ref = refs.rollout(knots, labels, ut, 0, [[0.5]], [[0.05]], X0, planes, eps, p, nodes, 3, 0, "linear", q=[1.0], r=[1.0])
            out = ro.run_actuator(X0, planes, seed=3, keep_path=True)
            _check_bits(out, ref)
            ro.set_option("lds", 0)
            _equal_runs(ro.run_actuator(X0, planes, seed=3, keep_path=True), out)
            ro.set_option("lds", 1)


# ---- 6. consequence (iv): promised equals paid ---------------------------------------------------------------------------------------
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


def _fly_lattice(labels, weights, n_samples, seed):
    import hjbdp
    X0 = np.repeat(refs.LATTICE_STARTS, n_samples).reshape(1, -1)               # sample j of start i on stream i * n_samples + j
    with hjbdp.ActuatorRollout([refs.LATTICE_KNOTS], labels, refs.LATTICE_U, index_base=0) as ro:
        ro.set_model([[1.0]], [[1.0]], q=[1.0], r=[refs.LATTICE_R])
        ro.set_actuator_noise(refs.LATTICE_EPS, weights)
        out = ro.run_actuator(X0, np.arange(refs.LATTICE_STAGES), seed=seed)
    return out["cost"].reshape(refs.LATTICE_STARTS.size, n_samples)


def test_expected_cost_promised_is_the_cost_paid(lattice):
    J1, labels = lattice["expect"]
    starts = (refs.LATTICE_STARTS + 16).astype(np.int64)
    costs, prob, _ = refs.lattice_enumeration(labels)
    mean = costs @ prob
    assert np.array_equal(mean, J1[starts])                                     # the promise is the exact expectation
    sigma = np.sqrt(((costs - mean[:, None]) ** 2) @ prob)                      # exact, from the 3^6 sequences: never from samples
    assert sigma[4] == 0.0 and np.all(np.delete(sigma, 4) > 0)                  # from x = 0 the policy commands 0 throughout: no noise
    n = 1 << 16
    paid = _fly_lattice(labels, refs.LATTICE_P, n, seed=2033)
    assert all(np.isin(paid[i], costs[i]).all() for i in range(9))              # every paid cost is one of the enumerated costs
    err = np.abs(paid.mean(axis=1) - J1[starts])
    print("promised", J1[starts], "paid", paid.mean(axis=1), "err / (sigma / 2^8)", err / np.where(sigma > 0, sigma / 256.0, 1.0))
    assert np.all(err <= 6.0 * sigma / 256.0), (err, sigma)                     # six standard errors of a mean of 2^16; equality at x = 0


def test_worst_case_promised_is_the_worst_cost_paid(lattice):
    J1, labels = lattice["worst"]
    starts = (refs.LATTICE_STARTS + 16).astype(np.int64)
    costs, _, _ = refs.lattice_enumeration(labels)
    assert np.array_equal(costs.max(axis=1), J1[starts])
    assert J1[starts][0] == 26.5 and J1[starts][-1] == 26.5
    paid = _fly_lattice(labels, None, 1 << 16, seed=2034)                       # uniform over the three nodes
    assert np.all(paid <= J1[starts][:, None])
    assert np.array_equal(paid.max(axis=1), J1[starts])


# ---- 7. validation with a device ---------------------------------------------------------------------------------------------------
def test_validation_with_a_device_and_two_threads(built):
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(733)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 3, 2, np.int32, 9, 5)
    X0 = rng.uniform(-1.0, 1.0, size=(3, 2000))
    planes = rng.integers(0, 5, size=9)
    eps, p = rng.uniform(-0.5, 0.5, size=(5, 2)), rng.uniform(0.1, 1.0, size=5)
    nodes = rng.uniform(-0.2, 0.2, size=(3, 5))
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    with hjbdp.ActuatorRollout(knots, labels, ut, index_base=base) as ro:
        lib, h = ro.lib, ro._ro
        err = lambda: lib.hjb_rollout_last_error(h).decode()
        with pytest.raises(hjbdp.HjbError) as ei:                               # no model yet (check_run)
            ro.run_actuator(X0, planes)
        assert ei.value.status == _abi.HJB_E_INVALID and "hjb_rollout_set_model" in str(ei.value)
        ro.set_model(A, B, c=c, q=[1, 1, 1])
        ro.set_noise(nodes, p)                                                  # an additive set is not an actuator set
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_actuator(X0, planes)
        assert ei.value.status == _abi.HJB_E_INVALID and "before hjb_rollout_set_actuator_noise" in str(ei.value)
        ro.set_actuator_noise(eps, p, nodes)
        good = ro.run_actuator(X0, planes, seed=4, keep_path=True)
        epsF = np.ascontiguousarray(eps.reshape(-1))                            # [n_u, W] column-major
        nodF = np.ascontiguousarray(nodes.reshape(-1, order="F"))
        bad_eps, bad_nod = epsF.copy(), nodF.copy()
        bad_eps[2 * 3 + 1] = np.nan
        bad_nod[3 * 2 + 1] = np.inf
        for args, text in (((-1, dp(epsF), None, None), "n_nodes=-1"), ((129, dp(epsF), None, None), "n_nodes=129"),
                           ((5, None, dp(nodF), None), "null eps"),
                           ((5, dp(bad_eps), dp(nodF), None), "eps of input 1, node 3 is not finite"),
                           ((5, dp(epsF), dp(bad_nod), None), "base of axis 1, node 2 is not finite"),
                           ((5, dp(epsF), None, dp([1, 1, np.inf, 1, 1])), "weight 2 is not finite or is negative"),
                           ((5, dp(epsF), None, dp([1, -1, 1, 1, 1])), "weight 1 is not finite or is negative"),
                           ((5, dp(epsF), None, dp([0, 0, 0, 0, 0])), "weights sum to 0")):
            assert lib.hjb_rollout_set_actuator_noise(h, *args) == _abi.HJB_E_INVALID and text in err(), (err(), text)
            assert "hjb_rollout_set_actuator_noise" in err()
            # the node set is the one it was
            _equal_runs(ro.run_actuator(X0, planes, seed=4, keep_path=True), good)
        # run_actuator's refusals leave every output untouched
        Xc = np.ascontiguousarray(X0.T)
        ps = np.ascontiguousarray(planes, dtype=np.int32)
        pp = ps.ctypes.data_as(C.POINTER(C.c_int32))
        nt, K = X0.shape[1], len(ps)
        Xn = Xc.copy()
        Xn[17, 2] = np.inf
        far = np.array([0, 5] + [0] * (K - 2), dtype=np.int32)
        for call, text in ((dict(first=-1), "first_stream=-1 < 0"), (dict(first=2 ** 63 - 1000), "overflows"), (dict(method=7), "method 7"),
                           (dict(K=-1), "n_steps=-1"), (dict(pl=far.ctypes.data_as(C.POINTER(C.c_int32))), "plane_of_step[1] = 5"),
                           (dict(pl=None), "null plane_of_step"), (dict(X=dp(Xn)), "not finite"), (dict(X=None), "null X0")):
            outs = [np.full(m, 7.25) for m in (nt * 3, nt, nt * 3 * (K + 1), nt * 2 * K, nt * K)]
            ms = C.c_double(7.25)
            st = lib.hjb_rollout_run_actuator(h, call.get("method", 1), call.get("K", K), call.get("pl", pp), nt, call.get("X", dp(Xc)), 4,
                                              call.get("first", 0), *[dp(o) for o in outs], C.byref(ms))
            assert st == _abi.HJB_E_INVALID and text in err(), (call, err())
            assert all(np.all(o == 7.25) for o in outs) and ms.value == 7.25, call
        _equal_runs(ro.run_actuator(X0, planes, seed=4, keep_path=True), good)
        # two threads on the one object: the calls take turns
        par = [None, None]

        def work(t):
            for _ in range(3):
                par[t] = ro.run_actuator(X0, planes, seed=4 + t, first_stream=1000 * t, keep_path=True)
        ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        _equal_runs(par[0], good)
        _check_bits(par[1], refs.rollout(knots, labels, ut, base, A, B, X0, planes, eps, p, nodes, 5, 1000, "linear", c=c, q=[1, 1, 1]))
        ro.clear_actuator_noise()
        with pytest.raises(hjbdp.HjbError):
            ro.run_actuator(X0, planes)
        # the Python side's own checks
        for bad in (np.zeros((5, 3)), np.zeros((0,)), np.zeros((129,))):
            with pytest.raises(ValueError):
                ro.set_actuator_noise(bad)
        with pytest.raises(ValueError):
            ro.set_actuator_noise(eps, p, np.zeros((2, 5)))
    # a model other than the affine one
    k6, l6, u6, b6, _, _, _ = _random_problem(rng, 6, 3, np.uint8, 5, 2)
    with hjbdp.ActuatorRollout(k6, l6, u6, index_base=b6) as ro:
        ro.set_attitude_model([1.0, 2.0, 3.0], 0.01)
        ro.set_actuator_noise([0.1, -0.1])
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_actuator(np.zeros((6, 4)), [0, 1])
        assert ei.value.status == _abi.HJB_E_INVALID and "attitude model" in str(ei.value)


# ---- 8. the mirror -------------------------------------------------------------------------------------------------------------------
def test_dynamic_solver_actuator_flights(built):
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N, ds.dx, ds.du = 6, 9, 20
    eps, w = np.array([-0.2, -0.1, 0.0, 0.1, 0.2]), np.array([1.0, 4.0, 6.0, 4.0, 1.0])
    ds.actuator_noise = (eps, w, "expect")
    ds.run()
    X0s = np.array([[2.0, 0.5, -1.0], [1.0, -0.5, 0.25]])
    cost = ds.get_actuator_paths(X0s, 50, seed=6)
    assert cost.shape == (3, 50)
    assert ds.actuator_cost_mean.shape == ds.actuator_cost_std.shape == ds.actuator_cost_max.shape == (3,)
    assert np.array_equal(ds.actuator_cost_mean, cost.mean(axis=1)) and np.array_equal(ds.actuator_cost_max, cost.max(axis=1))
    assert np.all(ds.actuator_cost_std > 0)
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    ut = np.asarray(ds._U_mesh, dtype=np.float64)
    with hjbdp.ActuatorRollout([s_r, s_r], ds.u_star_idxs, ut, index_base=1) as ro:
        ro.set_model(ds.A, ds.B, q=np.diag(ds.Q), r=[ds.R])
        ro.set_actuator_noise(eps, w)
        for i in range(3):                                                      # sample j of start i on stream i * n_samples + j
            by_hand = ro.run_actuator(np.repeat(X0s[:, i:i + 1], 50, axis=1), np.arange(5), seed=6, first_stream=50 * i)
            assert _same(by_hand["cost"], cost[i])
    cmap = ds.actuator_cost_map(16, seed=6, cost_threshold=1.0)
    assert cmap["mean"].shape == (9, 9) and cmap["stats"].shape == (9, 9, 8) and cmap["n_exceed"].shape == (9, 9)
    grid = np.stack([np.tile(s_r, 9), np.repeat(s_r, 9)])
    assert np.array_equal(cmap["max"].reshape(-1, order="F"), ds.get_actuator_paths(grid, 16, seed=6).max(axis=1))
    ds.actuator_noise = (eps, None, "worst")                                    # a 'worst' set is sampled uniformly
    uniform = ds.get_actuator_paths(X0s, 50, seed=6)
    assert uniform.shape == (3, 50) and not np.array_equal(uniform, cost)
    # the three old flights still refuse while actuator_noise is set
    for fly in (lambda: ds.get_noisy_paths(X0s, 4), lambda: ds.get_lookahead_paths(X0s), lambda: ds.get_noisy_cost_statistics(X0s, 4)):
        with pytest.raises(RuntimeError, match="control-dependent noise"):
            fly()
    ds.actuator_noise = None
    for fly in (lambda: ds.get_actuator_paths(X0s, 5), lambda: ds.actuator_cost_map(4)):
        with pytest.raises(RuntimeError, match="actuator_noise"):
            fly()
