"""GPU tests of the attitude rollout (hjb_rollout_run_attitude, K17 csrc/kernels_rollout_attitude.h; hjbdp.Rollout.run_attitude,
Solver_attitude.get_optimal_paths): the angles and every instantiation bit-equal to tests/attitude_rollout_refs.py, the reference's
policy against the host mirror over the whole horizon, chunking, threads, model switching and every refusal with a device."""
import threading

import numpy as np
import pytest

import attitude_rollout_refs as ar
import rollout_refs

pytestmark = pytest.mark.gpu


def _same(a, b):
    """bit for bit (a NaN equals any NaN)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def _diff(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b)))
    return "%d differ, first at %s: %r vs %r" % (bad.size, np.unravel_index(bad[0], a.shape), a.flat[bad[0]], b.flat[bad[0]]) if bad.size else ""


def _check_bits(out, ref):
    for key, r in zip(("X_final", "cost", "X_path", "U_path", "A_path"), ref):
        if out[key] is not None:
            assert _same(out[key], r), (key, _diff(out[key], r))


def _grid(rng, long_axis=0):
    """small non-uniform 6-D grid (w1, w2, w3, yaw, pitch, roll); long_axis > 0: axis 0 gets that many knots (the knots then
    exceed the 32 KiB LDS budget and the global-memory form runs)"""
    knots = []
    for a, (lo, hi) in enumerate([(-0.9, 0.9)] * 3 + [(-0.6, 0.6), (-0.4, 0.4), (-0.7, 0.7)]):
        m = long_axis if (a == 0 and long_axis) else int(rng.integers(3, 5))
        k = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.0, size=m - 1))])
        knots.append(lo + (hi - lo) * k / k[-1])
    return knots


def _starts(rng, n):
    """w mostly inside, one start in ten up to 0.2 outside the grid; attitudes from random rotations up to ~60 degrees (some
    outside the angle grid)"""
    X = np.empty((7, n))
    X[0:3] = rng.uniform(-0.8, 0.8, size=(3, n))
    X[0:3, ::10] = rng.uniform(-1.1, 1.1, size=(3, X[:, ::10].shape[1]))
    ax = rng.normal(size=(3, n))
    ax /= np.sqrt((ax ** 2).sum(axis=0))
    th = rng.uniform(0, 1.1, size=n)
    X[3:6] = ax * np.sin(th / 2)
    X[6] = np.cos(th / 2)
    return X


def _problem(rng, dtype, n_labels, n_planes=3, long_axis=0):
    knots = _grid(rng, long_axis)
    nS = int(np.prod([len(k) for k in knots]))
    base = int(rng.integers(0, 2))
    labels = rng.integers(base, base + n_labels, size=(nS, n_planes)).astype(dtype)
    ut = rng.uniform(-0.01, 0.01, size=(n_labels, 3))           # |u / J| <= 0.4: the loop stays near the grid for 50 steps
    return knots, labels, ut, base


INERTIA = [0.02852, 0.028317, 0.0245]


def test_angles_bit_equal_to_the_twin(built):
    import hjbdp
    rng = np.random.default_rng(1)
    n = 100000
    X = np.zeros((7, n))
    Q = rng.normal(size=(4, n))
    Q /= np.sqrt((Q ** 2).sum(axis=0))
    Q[:, : n // 4] *= rng.uniform(0.9, 1.1, size=n // 4)           # not normalised: |pitch argument| beyond 1 -> clamped
    # edge cases: components from {+-0, +-1, +-1/2, +-1/sqrt2} (signed zeros in atan2's arguments, pitch at +-90 degrees)
    vals = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, np.sqrt(0.5), -np.sqrt(0.5)])
    E = np.array(np.meshgrid(vals, vals, vals, vals, indexing="ij")).reshape(4, -1)
    E = E[:, np.abs(E).sum(axis=0) > 0]
    Q[:, -E.shape[1]:] = E
    X[3:7] = Q
    knots, labels, ut, base = _problem(rng, np.uint8, 20, n_planes=1)
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_attitude_model(INERTIA, 0.005)
        out = ro.run_attitude(X, [0], "nearest", keep_path=True)
    yaw, pitch, roll = ar.angles(X)
    A = out["A_path"][:, :, 0]
    assert _same(A[:, 0], yaw), _diff(A[:, 0], yaw)
    assert _same(A[:, 1], pitch), _diff(A[:, 1], pitch)
    assert _same(A[:, 2], roll), _diff(A[:, 2], roll)
    assert np.abs(pitch).max() == np.pi / 2


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_every_instantiation_is_bit_equal_to_the_twin(built, dtype):
    import hjbdp
    rng = np.random.default_rng(10 + np.dtype(dtype).itemsize)
    # LDS-staged tables, then the global-memory form (u16: 1,500 labels = 36 KB of u_table; u8 / i32: 2,100 knots on axis 0)
    for n_labels, long_axis in ((40, 0), (1500, 0) if dtype == np.uint16 else (40, 2100)):
        knots, labels, ut, base = _problem(rng, dtype, n_labels, long_axis=long_axis)
        X0 = _starts(rng, 4096)
        planes = rng.integers(0, 3, size=50)
        q = rng.uniform(0, 1, size=7)
        r = rng.uniform(0, 1, size=3)
        with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
            for integ in ("taylor", "RK4"):
                ro.set_attitude_model(INERTIA, 0.01, integ, q=q, r=r)
                for method in ("nearest", "linear"):
                    out = ro.run_attitude(X0, planes, method, keep_path=True)
                    ref = ar.rollout(knots, labels, ut, base, INERTIA, 0.01, integ, X0, planes, method, q=q, r=r)
                    _check_bits(out, ref)
                    # on the 2,100-knot axis 'linear' extrapolates with slopes of ~20 per unit: a start that drifts out of the
                    # grid there may overflow (bit-equal on both sides all the same); the short grids stay finite
                    assert np.isfinite(out["cost"]).mean() > (0.5 if long_axis else 0.999999)
                    if n_labels == 40 and not long_axis:        # the LDS-sized problem once more, forced into the global-memory form
                        ro.set_option("lds", 0)
                        glob = ro.run_attitude(X0, planes, method, keep_path=True)
                        ro.set_option("lds", 1)
                        _check_bits(glob, ref)
                        for key in ("X_final", "cost", "X_path", "U_path", "A_path"):
                            assert _same(glob[key], out[key]), key


@pytest.fixture(scope="module")
def attitude_solver(built):
    import hjbdp
    sa = hjbdp.Solver_attitude(11, 10)
    sa.run(n_stages=19)
    return sa


def _starts_ref(sa):
    from hjbdp.rollout import DEFAULT_X0_ATTITUDE, angle_to_quat
    X0 = [DEFAULT_X0_ATTITUDE]
    for (y, p, r, w) in ((10.0, -5.0, 20.0, 0.1), (-25.0, 15.0, -30.0, -0.2), (5.0, 18.0, 3.0, 0.3)):
        q = angle_to_quat(np.radians(y), np.radians(p), np.radians(r))          # scalar first
        X0.append(np.concatenate([[w, -w / 2, w / 3], q[::-1]]))
    return np.stack(X0, axis=1)


def test_reference_policy_against_the_host_mirror(attitude_solver):
    sa = attitude_solver
    X0 = _starts_ref(sa)
    X, U, XA = sa.get_optimal_paths(X0, "nearest")
    N = sa.N_stage
    assert X.shape == (7, N, 4) and U.shape == (3, N, 4) and XA.shape == (9, N, 4) and not U[:, N - 1].any()
    from hjbdp.rollout import quat_to_yaw_pitch_roll
    knots = sa.grid_vectors_full()
    mids = [(k[:-1] + k[1:]) / 2 for k in knots[3:]]
    for t in range(X0.shape[1]):
        Xh, Uh, XAh = sa.get_optimal_path(X0[:, t], "nearest")
        assert _same(X[:, :, t], Xh), _diff(X[:, :, t], Xh)
        assert _same(U[:, :, t], Uh), _diff(U[:, :, t], Uh)
        assert np.abs(XA[:, :, t] - XAh).max() <= 1e-13
        # the claim rests on a margin: no host angle lies within 1e-9 of a cell midpoint
        for k in range(N - 1):
            ang = quat_to_yaw_pitch_roll([Xh[6, k], Xh[5, k], Xh[4, k], Xh[3, k]])
            for a in range(3):
                assert np.abs(mids[a] - ang[a]).min() > 1e-9, (t, k, a)
    Xl, Ul, _ = sa.get_optimal_paths(X0, "linear", n_steps=200)
    for t in range(X0.shape[1]):
        Xh, Uh, _ = sa.get_optimal_path(X0[:, t], "linear", n_steps=200)
        assert np.abs(Xl[:, :, t] - Xh).max() <= 1e-9 and np.abs(Ul[:, :, t] - Uh).max() <= 1e-9


def test_chunking_threads_and_model_switching(built):
    import hjbdp
    rng = np.random.default_rng(5)
    knots, labels, ut, base = _problem(rng, np.uint16, 30)
    X0 = _starts(rng, 5000)
    planes = rng.integers(0, 3, size=30)
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro, hjbdp.Rollout(knots, labels, ut, index_base=base) as rc:
        for o in (ro, rc):
            o.set_attitude_model(INERTIA, 0.01, "RK4", q=np.ones(7), r=np.ones(3))
        rc.set_option("chunk", 1000)
        one, chunked = ro.run_attitude(X0, planes, "linear", keep_path=True), rc.run_attitude(X0, planes, "linear", keep_path=True)
        for key in ("X_final", "cost", "X_path", "U_path", "A_path"):
            assert _same(one[key], chunked[key]), key
        lean = ro.run_attitude(X0, planes, "linear")
        assert lean["X_path"] is None and lean["A_path"] is None and _same(lean["X_final"], one["X_final"])
        assert ro.run_attitude(np.zeros((7, 0)), planes)["X_final"].shape == (7, 0)
        # two objects on two threads = the same runs one after the other
        args = [(X0, planes, "linear"), (X0[:, :3000], planes, "nearest")]
        seq = [o.run_attitude(*a, keep_path=True) for o, a in zip((ro, rc), args)]
        par = [None, None]

        def work(t):
            for _ in range(3):
                par[t] = (ro, rc)[t].run_attitude(*args[t], keep_path=True)
        ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for s, p in zip(seq, par):
            for key in ("X_final", "cost", "X_path", "U_path", "A_path"):
                assert _same(s[key], p[key]), key
    # after the attitude model, set_model then hjb_rollout_run equals a fresh object
    rng = np.random.default_rng(6)
    A = rng.uniform(-1, 1, size=(6, 6))
    A *= 0.5 / np.linalg.norm(A, 2)
    B = rng.uniform(-0.02, 0.02, size=(6, 3))
    Xa = rng.uniform(-0.5, 0.5, size=(6, 500))
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro, hjbdp.Rollout(knots, labels, ut, index_base=base) as fresh:
        ro.set_attitude_model(INERTIA, 0.01)
        ro.run_attitude(X0[:, :100], planes)
        ro.set_model(A, B, q=np.ones(6))
        fresh.set_model(A, B, q=np.ones(6))
        got, want = ro.run(Xa, planes, "linear", keep_path=True), fresh.run(Xa, planes, "linear", keep_path=True)
        for key in ("X_final", "cost", "X_path", "U_path"):
            assert _same(got[key], want[key]), key
        ref = rollout_refs.rollout(knots, labels, ut, base, A, B, Xa, planes, "linear", q=np.ones(6))
        assert _same(got["X_final"], ref[0])


def test_refusals_with_a_device(built):
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(7)
    knots, labels, ut, base = _problem(rng, np.uint8, 12)
    X0 = _starts(rng, 64)

    def refused(fn, *needles):
        with pytest.raises(hjbdp.HjbError) as ei:
            fn()
        assert ei.value.status == _abi.HJB_E_INVALID, str(ei.value)
        for nd in needles:
            assert nd in str(ei.value), (nd, str(ei.value))

    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        refused(lambda: ro.run_attitude(X0, [0]), "set_attitude_model")
        refused(lambda: ro.set_attitude_model([0.02, 0.0, 0.02], 0.005), "J2")
        refused(lambda: ro.set_attitude_model([0.02, -1.0, 0.02], 0.005), "J2")
        refused(lambda: ro.set_attitude_model([np.nan, 0.02, 0.02], 0.005), "J1")
        refused(lambda: ro.set_attitude_model(INERTIA, 0.0), "h")
        refused(lambda: ro.set_attitude_model(INERTIA, np.inf), "h")
        refused(lambda: C_integ(ro, 2), "integrator")
        refused(lambda: ro.set_attitude_model(INERTIA, 0.005, q=[1, 1, 1, np.nan, 1, 1, 1]), "q")
        refused(lambda: ro.set_attitude_model(INERTIA, 0.005, r=[1, np.inf, 1]), "r is not finite")
        ro.set_model(np.eye(6), np.zeros((6, 3)))
        refused(lambda: ro.run_attitude(X0, [0]), "hjb_rollout_run")
        ro.set_attitude_model(INERTIA, 0.005)
        refused(lambda: ro.run(X0[:6], [0], "linear"), "hjb_rollout_run_attitude")
        for planes in ([0, 3], [-1]):
            refused(lambda: ro.run_attitude(X0, planes), "plane_of_step")
        Xz = X0.copy()
        Xz[3:7, 17] = [0.0, -0.0, 0.0, 0.0]
        refused(lambda: ro.run_attitude(Xz, [0]), "column 17", "quaternion")
        Xn = X0.copy()
        Xn[5, 3] = np.nan
        refused(lambda: ro.run_attitude(Xn, [0]), "not finite")
        refused(lambda: ro._check(ro.lib.hjb_rollout_run_attitude(ro._ro, 2, 0, None, 0, None, None, None, None, None, None, None)),
                "method")
    # the attitude model needs D = 6 and n_u = 3
    k = np.linspace(-1, 1, 3)
    with hjbdp.Rollout([k] * 5, np.ones(3 ** 5, np.uint8), np.zeros((1, 3)), index_base=1) as r5:
        refused(lambda: r5.set_attitude_model(INERTIA, 0.005), "D == 6")
    with hjbdp.Rollout([k] * 6, np.ones(3 ** 6, np.uint8), np.zeros((1, 2)), index_base=1) as r6:
        refused(lambda: r6.set_attitude_model(INERTIA, 0.005), "n_u == 3")


def C_integ(ro, integ):
    """hjb_rollout_set_attitude_model with a raw integrator code (the Python wrapper only passes 'taylor' / 'RK4')"""
    import ctypes as C
    J = np.ascontiguousarray(INERTIA, dtype=np.float64)
    ro._check(ro.lib.hjb_rollout_set_attitude_model(ro._ro, J.ctypes.data_as(C.POINTER(C.c_double)), 0.005, integ, None, None))
