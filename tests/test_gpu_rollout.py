"""GPU tests of the batched closed-loop rollout (hjb_rollout_*, csrc/kernels_rollout.h; hjbdp.Rollout,
Dynamic_Solver.get_optimal_paths): the Kirk fixture path, bit-equality with tests/rollout_refs.py at every instantiation (LDS and
global-memory form), chunking, a real per-stage policy, and validation / concurrency with a device.  The global-memory form as the
library chooses it, label and placement edges and far label offsets: tests/test_gpu_rollout_forms.py."""
import threading
from pathlib import Path

import numpy as np
import pytest

import rollout_refs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _same(a, b):
    """bit for bit, except that a NaN equals any NaN (IEEE leaves the payload of an invalid operation's result open; a
    trajectory that leaves the grid far enough on an unstable loop overflows to inf and then NaN on both sides)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def _diff(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b)))
    return "%d differ, first at %s: %r vs %r" % (bad.size, np.unravel_index(bad[0], a.shape), a.flat[bad[0]], b.flat[bad[0]]) if bad.size else ""


def _check_bits(out, ref):
    Xf, cost, Xp, Up = ref
    assert _same(out["X_final"], Xf), _diff(out["X_final"], Xf)
    assert _same(out["cost"], cost), _diff(out["cost"], cost)
    if out["X_path"] is not None:
        assert _same(out["X_path"], Xp), _diff(out["X_path"], Xp)
        assert _same(out["U_path"], Up), _diff(out["U_path"], Up)


@pytest.fixture(scope="module")
def kirk(built):
    import hjbdp
    sols = {}
    for prec in ("double", "single"):
        ds = hjbdp.Dynamic_Solver(precision=prec)
        ds.N, ds.dx, ds.du = 130, 35, 100
        ds.run()
        sols[prec] = ds
    return sols


def test_kirk_fixture_path_on_the_gpu(kirk):
    ds = kirk["double"]
    g = np.load(ROOT / "tests" / "golden" / "obj_1.npz")
    X, U = ds.get_optimal_paths([[2.0], [1.0]])
    assert X.shape == (2, 130, 1) and U.shape == (130, 1) and U[129, 0] == 0.0
    assert np.max(np.abs(X[:, :, 0] - g["traj_X"])) <= 1e-9
    assert np.max(np.abs(U[:, 0] - np.asarray(g["traj_U"]).reshape(-1))) <= 1e-9
    Xh, Uh = ds.get_optimal_path(np.array([2.0, 1.0]))
    assert np.max(np.abs(X[:, :, 0] - Xh)) <= 1e-9 and np.max(np.abs(U[:, 0] - Uh)) <= 1e-9


def _kirk_starts(ds, n, seed):
    """inside the grid, on knots, at cell midpoints and out to 3 cell widths outside"""
    rng = np.random.default_rng(seed)
    k = np.asarray(ds.s_r, dtype=np.float64)
    h = k[1] - k[0]
    q = n // 4
    inside = rng.uniform(k[0], k[-1], size=(2, q))
    knots = k[rng.integers(0, len(k), size=(2, q))]
    mids = (k[:-1] + np.diff(k) / 2)[rng.integers(0, len(k) - 1, size=(2, q))]
    outside = rng.uniform(k[0] - 3 * h, k[-1] + 3 * h, size=(2, n - 3 * q))
    return np.concatenate([inside, knots, mids, outside], axis=1)


@pytest.mark.parametrize("prec", ["double", "single"])
def test_kirk_ten_thousand_starts_are_bit_equal_to_the_restatement(kirk, prec):
    import hjbdp
    ds = kirk[prec]
    X0 = _kirk_starts(ds, 10000, 11)
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    ut = np.asarray(ds._U_mesh).astype(ds.J_star.dtype).astype(np.float64)
    q, r = np.diag(ds.Q), [ds.R]
    n_st = ds.N - 1
    with hjbdp.Rollout([s_r, s_r], ds.u_star_idxs, ut, index_base=1) as ro:
        ro.set_model(ds.A, ds.B, q=q, r=r)
        for method in ("linear", "nearest"):
            for planes in (np.arange(n_st), np.full(n_st, 0), np.full(n_st, 63)):      # 'Nssu', 'ssu' 1 and 'ssu' 64
                out = ro.run(X0, planes, method=method, keep_path=True)
                ref = rollout_refs.rollout([s_r, s_r], ds.u_star_idxs, ut, 1, ds.A, ds.B, X0, planes, method, q=q, r=r)
                _check_bits(out, ref)
                assert np.isfinite(out["cost"]).mean() > 0.5       # starts far outside on Kirk's unstable loop may overflow
    # the solver's entry point runs the same object ('ssu' 64, linear)
    X, U = ds.get_optimal_paths(X0[:, :64], mode="ssu", ssu_num=64)
    ref = rollout_refs.rollout([s_r, s_r], ds.u_star_idxs, ut, 1, ds.A, ds.B, X0[:, :64], np.full(n_st, 63), "linear", q=q, r=r)
    assert _same(np.ascontiguousarray(X), np.ascontiguousarray(ref[2].transpose(1, 2, 0)))
    assert _same(np.ascontiguousarray(U[:n_st]), np.ascontiguousarray(ref[3][:, 0, :].T)) and not U[n_st].any()


def _random_problem(rng, D, nu, dtype, n_labels, n_planes):
    """random knots about 0, labels and table; A with spectral norm 0.5 and a small B: the closed loop stays bounded from
    starts up to 0.1 outside the grid (the linear lookup extrapolates as a degree-D polynomial there)"""
    n = [int(v) for v in rng.integers(2, 6 if D <= 4 else 4, size=D)]
    knots = []
    for m in n:
        k = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.0, size=m - 1))])
        knots.append(k - k[-1] / 2 + rng.uniform(-0.1, 0.1))
    nS = int(np.prod(n))
    base = int(rng.integers(0, 2))
    labels = rng.integers(base, base + n_labels, size=(nS, n_planes)).astype(dtype)
    ut = rng.uniform(-1.0, 1.0, size=(n_labels, nu))
    A = rng.uniform(-1.0, 1.0, size=(D, D))
    A *= 0.5 / np.linalg.norm(A, 2)
    B = rng.uniform(-0.02, 0.02, size=(D, nu))
    c = rng.uniform(-0.02, 0.02, size=D)
    return knots, labels, ut, base, A, B, c


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_every_instantiation_is_bit_equal_to_the_restatement(built, D, dtype):
    import hjbdp
    rng = np.random.default_rng(100 * D + np.dtype(dtype).itemsize)
    for nu in (1, 4):
        for base in (0, 1):
            knots, labels, ut, _, A, B, c = _random_problem(rng, D, nu, dtype, 7, 3)
            labels = (labels - labels.min() + base).astype(dtype)
            lo = np.array([k[0] for k in knots]) - 0.1
            hi = np.array([k[-1] for k in knots]) + 0.1
            X0 = rng.uniform(lo[:, None], hi[:, None], size=(D, 300))
            planes = rng.integers(0, 3, size=8)
            q = rng.uniform(0, 1, size=D)
            r = rng.uniform(0, 1, size=nu)
            with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
                ro.set_model(A, B, c=c if nu == 4 else None, q=q, r=r)
                for method in ("nearest", "linear"):
                    out = ro.run(X0, planes, method=method, keep_path=True)
                    ref = rollout_refs.rollout(knots, labels, ut, base, A, B, X0, planes, method, c=c if nu == 4 else None, q=q, r=r)
                    _check_bits(out, ref)
                    assert np.isfinite(out["cost"]).all()
                    # the same object's global-memory form (option "lds" = 0: the LDS = false instantiation): the twin's bits, the LDS form's bits
                    ro.set_option("lds", 0)
                    glob = ro.run(X0, planes, method=method, keep_path=True)
                    ro.set_option("lds", 1)
                    _check_bits(glob, ref)
                    _check_bits(glob, (out["X_final"], out["cost"], out["X_path"], out["U_path"]))


def test_chunking_and_batch_sizes(built):
    import hjbdp
    rng = np.random.default_rng(7)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 2, 2, np.uint16, 12, 4)
    planes = rng.integers(0, 4, size=9)
    lo = np.array([k[0] for k in knots]) - 0.2
    hi = np.array([k[-1] for k in knots]) + 0.2
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro, hjbdp.Rollout(knots, labels, ut, index_base=base) as ro64:
        ro.set_model(A, B, c=c, q=[1.0, 0.5], r=[0.1, 0.2])
        ro64.set_model(A, B, c=c, q=[1.0, 0.5], r=[0.1, 0.2])
        ro64.set_option("chunk", 64)
        for nt in (1, 63, 64, 65, 257):
            X0 = rng.uniform(lo[:, None], hi[:, None], size=(2, nt))
            ref = rollout_refs.rollout(knots, labels, ut, base, A, B, X0, planes, "linear", c=c, q=[1.0, 0.5], r=[0.1, 0.2])
            for r_ in (ro, ro64):
                out = r_.run(X0, planes, "linear", keep_path=True)
                _check_bits(out, ref)
                lean = r_.run(X0, planes, "linear", keep_path=False)
                assert lean["X_path"] is None and _same(lean["X_final"], out["X_final"]) and _same(lean["cost"], out["cost"])
        empty = ro.run(np.zeros((2, 0)), planes, "linear")
        assert empty["X_final"].shape == (2, 0) and empty["device_ms"] == 0.0
        # 10^6 trajectories in one launch and in chunks of 2^18, checked on a seeded sample
        X0 = rng.uniform(lo[:, None], hi[:, None], size=(2, 1000000))
        big = ro.run(X0, planes, "linear")
        ro64.set_option("chunk", 1 << 18)
        big_c = ro64.run(X0, planes, "linear")
        assert _same(big["X_final"], big_c["X_final"]) and _same(big["cost"], big_c["cost"]) and big["device_ms"] > 0
        pick = np.sort(np.random.default_rng(3).choice(X0.shape[1], 4096, replace=False))
        ref = rollout_refs.rollout(knots, labels, ut, base, A, B, X0[:, pick], planes, "linear", c=c, q=[1.0, 0.5], r=[0.1, 0.2])
        assert _same(np.ascontiguousarray(big["X_final"][:, pick]), ref[0]) and _same(big["cost"][pick], ref[1])


def test_real_per_stage_position_policy(built):
    import hjbdp
    sp = hjbdp.Solver_position()
    sp.n_mesh_x = sp.n_mesh_v = 60
    s_x, s_v = sp.build_spec(0)[1:]                 # before the run: simplified_run leaves n_mesh_* = the grid sizes (61)
    sp.simplified_run(n_stages=200, keep_policy=True)
    labels = sp.U_idx_stages[0]
    h = sp.h
    # the sweep's design model x+ = x + dx(v), v+ = v + dv(u): affine, dx(v) = a v and dv(u) = b u in exact arithmetic
    A = np.array([[1.0, sp._dx_of_v(1.0, h)], [0.0, 1.0]])
    B = np.array([[0.0], [sp._dv_of_u(1.0, h)]])
    rng = np.random.default_rng(9)
    X0 = np.stack([rng.uniform(-0.5, 0.5, 2000), rng.uniform(-0.5, 0.5, 2000)])
    planes = np.arange(200)                         # stage k_s + 1 at step k_s (plane k_s)
    with hjbdp.Rollout([s_x, s_v], labels, sp.U_vector, index_base=1) as ro:
        ro.set_model(A, B, q=[sp.Qx1, sp.Qv1], r=[sp.R1])
        out = ro.run(X0, planes, "nearest", keep_path=True)
    ref = rollout_refs.rollout([s_x, s_v], labels, sp.U_vector, 1, A, B, X0, planes, "nearest", q=[sp.Qx1, sp.Qv1], r=[sp.R1])
    _check_bits(out, ref)
    assert set(np.unique(out["U_path"])) <= set(sp.U_vector)


def test_validation_with_a_device_and_two_threads(built):
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(21)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 3, 2, np.int32, 9, 5)
    X0 = rng.uniform(-1.0, 2.0, size=(3, 5000))
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run(X0, [0, 1], "linear")
        assert ei.value.status == _abi.HJB_E_INVALID and "set_model" in str(ei.value)
        bad = A.copy()
        bad[1, 2] = np.inf
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.set_model(bad, B)
        assert ei.value.status == _abi.HJB_E_INVALID and "A is not finite" in str(ei.value)
        ro.set_model(A, B, c=c)
        for planes in ([0, 5], [-1], [4, 2, 7]):
            with pytest.raises(hjbdp.HjbError) as ei:
                ro.run(X0, planes, "linear")
            assert ei.value.status == _abi.HJB_E_INVALID and "plane_of_step" in str(ei.value)
        X0n = X0.copy()
        X0n[2, 17] = np.nan
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run(X0n, [0], "linear")
        assert ei.value.status == _abi.HJB_E_INVALID
        with pytest.raises(hjbdp.HjbError):
            ro.set_option("chunk", 0)
    # two objects on two threads = the same objects one after the other
    k2, l2, u2, b2, A2, B2, c2 = _random_problem(rng, 4, 3, np.uint8, 9, 5)
    X2 = rng.uniform(-1.0, 2.0, size=(4, 5000))
    planes = rng.integers(0, 5, size=40)
    objs = [hjbdp.Rollout(knots, labels, ut, index_base=base), hjbdp.Rollout(k2, l2, u2, index_base=b2)]
    objs[0].set_model(A, B, c=c, q=[1, 1, 1])
    objs[1].set_model(A2, B2, c=c2, r=[1, 2, 3])
    args = [(X0, planes, "linear"), (X2, planes, "nearest")]
    seq = [o.run(*a, keep_path=True) for o, a in zip(objs, args)]
    par = [None, None]

    def work(t):
        for _ in range(3):
            par[t] = objs[t].run(*args[t], keep_path=True)
    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for s, p in zip(seq, par):
        for key in ("X_final", "cost", "X_path", "U_path"):
            assert _same(s[key], p[key]), key
    for o in objs:
        o.close()
