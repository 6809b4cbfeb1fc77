"""GPU tests of the simplified attitude rollout (hjb_rollout_run_attitude_simplified, K20
csrc/kernels_rollout_attitude_simplified.h; hjbdp.Rollout.run_attitude_simplified, Solver_attitude.get_optimal_paths_simplified):
every instantiation bit-equal to tests/attitude_simplified_rollout_refs.py, the policies simplified_run leaves against the scalar
host loop over the whole horizon (stationary and per stage), chunking, threads, model switching, starts that overflow during the
run, the lifetime of the attached objects and every refusal that needs a device."""
import threading

import numpy as np
import pytest

import attitude_simplified_rollout_refs as ar
import rollout_refs

pytestmark = pytest.mark.gpu

KEYS = ("X_final", "cost", "X_path", "U_path", "A_path")
INERTIA = np.array([[0.02852, -0.0000837, 0.000014], [-0.0000837, 0.028317, -0.00029], [0.000014, -0.00029, 0.0245]])
SIZES = ((9, 7), (12, 5), (6, 11))                    # (n_w, n_t) of channels 1, 2, 3
W_MAX, T_MAX = 0.87, (0.52, 0.35, 0.61)
QW, QT, RW = [6.0, 5.0, 4.0], [3.0, 6.0, 2.0], [4.0, 1.0, 0.5]
H = 0.01


def _same(a, b):
    """bit for bit (a NaN equals any NaN)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def _diff(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return "shapes %r vs %r" % (a.shape, b.shape)
    bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).reshape(-1) & ~(np.isnan(a) & np.isnan(b)).reshape(-1))
    return "%d differ, first at %s: %r vs %r" % (bad.size, np.unravel_index(bad[0], a.shape), a.flat[bad[0]], b.flat[bad[0]]) if bad.size else ""


def _head(ref, n):
    """the first n trajectories of a twin result (trajectories are independent)"""
    Xf, cost, Xp, Up, Ap = ref
    return Xf[:, :n], cost[:n], Xp[:n], Up[:n], Ap[:n]


def _check_bits(out, ref, paths=True):
    for key, r in zip(KEYS, ref):
        if not paths and key.endswith("_path"):
            assert out[key] is None, key
        else:
            assert out[key] is not None and _same(out[key], r), (key, _diff(out[key], r))


def _channels(rng, dtype, n_planes=3, long_axis=0):
    """three channels of different sizes over (w_i, theta_i): channel 1's rate axis and channel 3's angle axis non-uniform, 3 / 5 / 3
    labels, index_base 0 / 1 / 1, random labels and torques; long_axis > 0: channel 1's rate axis gets that many knots (the tables
    then exceed the 32 KiB LDS budget and the global-memory form runs)"""
    chans = []
    for ch, (nw, nt) in enumerate(SIZES):
        nw = long_axis if (ch == 0 and long_axis) else nw
        s_w, s_t = np.linspace(-W_MAX, W_MAX, nw), np.linspace(-T_MAX[ch], T_MAX[ch], nt)
        if ch == 0:
            s_w = W_MAX * np.sign(s_w) * (np.abs(s_w) / W_MAX) ** 1.5
        if ch == 2:
            s_t = T_MAX[ch] * np.sign(s_t) * (np.abs(s_t) / T_MAX[ch]) ** 1.3
        n_labels, base = (3, 5, 3)[ch], (0, 1, 1)[ch]
        labels = rng.integers(base, base + n_labels, size=(nw * nt, n_planes)).astype(dtype)
        ut = rng.choice([-0.11, 0.0, 0.11], size=n_labels) * rng.uniform(0.6, 1.0, size=n_labels)
        ut[:2] = [0.11, -0.09]
        chans.append(([s_w, s_t], labels, ut.reshape(-1, 1), base))
    return chans


def _starts(rng, n):
    """rates and angles inside the grids, one start in eight just outside them"""
    X = np.empty((7, n))
    X[0:3] = rng.uniform(-W_MAX, W_MAX, size=(3, n))
    ang = np.stack([rng.uniform(-t, t, size=n) for t in T_MAX])
    out = np.arange(n) % 8 == 5
    m = int(out.sum())
    X[0:3, out] = rng.choice([-1.0, 1.0], size=(3, m)) * rng.uniform(W_MAX, 1.2 * W_MAX, size=(3, m))
    ang[:, out] = rng.choice([-1.0, 1.0], size=(3, m)) * np.stack([rng.uniform(t, 1.25 * t, size=m) for t in T_MAX])
    X[3:6] = np.sin(ang / 2)
    X[6] = np.sqrt(1.0 - (X[3:6] ** 2).sum(axis=0))
    return X


class _Three:
    """three hjbdp.Rollout objects (channels 1, 2, 3) as one context manager"""

    def __init__(self, chans):
        import hjbdp
        self.ros = []
        try:
            for knots, labels, ut, base in chans:
                self.ros.append(hjbdp.Rollout(knots, labels, ut, index_base=base))
        except Exception:
            self.close()
            raise

    def close(self):
        for r in self.ros:
            r.close()

    def __enter__(self):
        return self.ros

    def __exit__(self, *a):
        self.close()


def _set(r1, r2, r3, S=1, dyn="full", inertia=INERTIA, h=H):
    r1.set_attitude_simplified_model(r2, r3, inertia, h, S, dyn, qw=QW, qt=QT, r=RW)


def _twin(chans, S, dyn, X0, planes):
    return ar.rollout(chans, INERTIA, H, S, dyn, X0, planes, QW, QT, RW)


@pytest.mark.parametrize("long_axis", [0, 2100], ids=["lds", "global"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_every_instantiation_is_bit_equal_to_the_twin(built, dtype, long_axis):
    """label type x knots placement (2,100 knots on one axis: the global-memory form) x dynamics, 'full' at 1, 2 and 3 sub-steps;
    1, 255 and 257 trajectories (less than a block, one short of it, one more); with the paths and with every optional output
    NULL.  One twin run of 257 starts per model serves the three sizes."""
    rng = np.random.default_rng(200 + 8 * np.dtype(dtype).itemsize + (long_axis > 0))
    K = 40
    chans = _channels(rng, dtype, long_axis=long_axis)
    X0 = _starts(rng, 257)
    planes = rng.integers(0, 3, size=K)
    assert len(set(planes.tolist())) == 3 and K > 3              # planes are revisited
    with _Three(chans) as (r1, r2, r3):
        for S, dyn in ((1, "full"), (2, "full"), (3, "full"), (1, "diagonal")):
            ref = _twin(chans, S, dyn, X0, planes)
            changed = int((np.abs(np.diff(ref[3], axis=2)).sum(axis=(1, 2)) > 0).sum())
            assert 4 * changed >= 257, changed                   # at least a quarter of the trajectories change torque
            _set(r1, r2, r3, S, dyn)
            for n in (1, 255, 257):
                _check_bits(r1.run_attitude_simplified(X0[:, :n], planes, keep_path=True), _head(ref, n))
                _check_bits(r1.run_attitude_simplified(X0[:, :n], planes), _head(ref, n), paths=False)
            assert np.isfinite(ref[0]).all()
            if not long_axis:           # the LDS-sized problem once more, forced into the global-memory form (option "lds" of channel 1's object)
                staged = r1.run_attitude_simplified(X0, planes, keep_path=True)
                r1.set_option("lds", 0)
                glob = r1.run_attitude_simplified(X0, planes, keep_path=True)
                r1.set_option("lds", 1)
                _check_bits(glob, ref)
                for key in staged:
                    if key != "device_ms":
                        assert _same(glob[key], staged[key]), key


def _cost_null(ro, X0, planes):
    """the raw call with cost NULL as well: only X_final is written"""
    import ctypes as C
    X = np.ascontiguousarray(X0.T)
    Xf = np.empty_like(X)
    ps = np.ascontiguousarray(planes, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    st = ro.lib.hjb_rollout_run_attitude_simplified(ro._ro, int(ps.size), ps.ctypes.data_as(C.POINTER(C.c_int32)), X.shape[0], p(X), p(Xf),
                                                    None, None, None, None)
    assert st == 0, ro.lib.hjb_rollout_last_error(ro._ro)
    return Xf.T


@pytest.fixture(scope="module")
def solved(built):
    import hjbdp
    sa = hjbdp.Solver_attitude(n_mesh_t=61, n_mesh_w_simplified=201)
    sa.simplified_run()
    return sa


REAL_STARTS = np.array([[0.2, -0.15, 0.1, 0.09, -0.06, 0.1, 0.0], [-0.5, 0.4, 0.6, -0.12, 0.08, -0.15, 0.0]]).T


def _real_starts():
    from hjbdp.rollout import DEFAULT_X0_ATTITUDE
    X0 = np.concatenate([DEFAULT_X0_ATTITUDE.reshape(7, 1), REAL_STARTS], axis=1)
    X0[6, 1:] = np.sqrt(1.0 - (X0[3:6, 1:] ** 2).sum(axis=0))
    return X0


@pytest.mark.parametrize("dynamics", ["full", "diagonal"])
def test_real_policies_against_the_scalar_host_loop(solved, dynamics):
    """the policies simplified_run leaves (201 x 61 meshes), the whole horizon, the default X0 and two more starts: bit equal to
    attitude_optimal_path_simplified_fixed"""
    from hjbdp.rollout import attitude_optimal_path_simplified_fixed, quat_to_yaw_pitch_roll
    sa = solved
    X0 = _real_starts()
    N = sa.N_stage
    T, X, U, ANG = sa.get_optimal_paths_simplified(X0, dynamics=dynamics, keep_path=True)
    assert T.shape == (N,) and X.shape == (N, 7, 3) and U.shape == (N, 3, 3) and ANG.shape == (N, 3, 3)
    assert not U[N - 1].any() and not ANG[N - 1].any() and np.isfinite(X).all()
    Xf, cost = sa.get_optimal_paths_simplified(X0, dynamics=dynamics)
    assert _same(Xf, X[N - 1])
    for t in range(3):
        Th, Xh, Uh, THh, ch = attitude_optimal_path_simplified_fixed(sa, X0[:, t], dynamics=dynamics)
        assert _same(T, Th)
        assert _same(X[:, :, t], Xh), _diff(X[:, :, t], Xh)
        assert _same(U[:, :, t], Uh), _diff(U[:, :, t], Uh)
        assert _same(cost[t], ch), (cost[t], ch)
        assert (np.abs(np.diff(Uh[:N - 1], axis=0)).sum(axis=1) > 0).any()           # the controller acts and switches
        k = N // 3
        want = np.degrees(quat_to_yaw_pitch_roll([Xh[k, 6], Xh[k, 5], Xh[k, 4], Xh[k, 3]]))
        assert np.allclose(ANG[k, :, t], want, rtol=0, atol=1e-12)
    if dynamics == "diagonal":
        assert np.abs(np.sqrt((X[:, 3:7] ** 2).sum(axis=1)) - 1.0).max() < 1e-15


def test_per_stage_policies_against_the_scalar_host_loop(built):
    """step k reads the policy of stage k: simplified_run(n_stages=300, keep_policy=True), 300 stages"""
    import hjbdp
    from hjbdp.rollout import attitude_optimal_path_simplified_fixed
    sa = hjbdp.Solver_attitude(n_mesh_t=61, n_mesh_w_simplified=201)
    sa.simplified_run(n_stages=300, keep_policy=True)
    assert sa.U_idx_stages[0].shape == (201, 61, 300)
    assert any((sa.U_idx_stages[c][:, :, 0] != sa.U_idx_stages[c][:, :, 299]).any() for c in range(3))       # the planes differ
    X0 = _real_starts()
    T, X, U, ANG = sa.get_optimal_paths_simplified(X0, n_steps=300, per_stage=True, keep_path=True)
    assert X.shape == (301, 7, 3)
    for t in range(3):
        Th, Xh, Uh, THh, ch = attitude_optimal_path_simplified_fixed(sa, X0[:, t], n_steps=300, per_stage=True)
        assert _same(X[:, :, t], Xh), _diff(X[:, :, t], Xh)
        assert _same(U[:, :, t], Uh), _diff(U[:, :, t], Uh)
    with pytest.raises(ValueError, match="300 stages"):
        sa.get_optimal_paths_simplified(X0, n_steps=301, per_stage=True)


def test_chunking_threads_and_model_switching(built):
    import hjbdp
    rng = np.random.default_rng(5)
    chans = _channels(rng, np.uint16)
    X0 = _starts(rng, 5001)
    K = 30
    planes = rng.integers(0, 3, size=K)
    with _Three(chans) as (r1, r2, r3), _Three(chans) as (c1, c2, c3):
        _set(r1, r2, r3, 2)
        _set(c1, c2, c3, 2)
        c1.set_option("chunk", 1000)                          # 5,001 is not a multiple of the chunk
        one, chunked = r1.run_attitude_simplified(X0, planes, keep_path=True), c1.run_attitude_simplified(X0, planes, keep_path=True)
        _check_bits(one, _twin(chans, 2, "full", X0, planes))
        for key in KEYS:
            assert _same(one[key], chunked[key]), key
        c1.set_option("chunk", 1)
        single = c1.run_attitude_simplified(X0[:, :7], planes, keep_path=True)
        for key in KEYS:
            assert _same(single[key], one[key][..., :7] if key == "X_final" else one[key][:7]), key
        c1.set_option("chunk", 1000)
        assert _same(_cost_null(c1, X0, planes), one["X_final"])
        assert r1.run_attitude_simplified(np.zeros((7, 0)), planes)["X_final"].shape == (7, 0)
        short = r1.run_attitude_simplified(X0[:, :100], planes[:0], keep_path=True)           # no stages: X_final = X0
        assert _same(short["X_final"], X0[:, :100]) and short["X_path"].shape == (100, 7, 1) and not short["cost"].any()
        # two objects on two threads = the same runs one after the other
        args = [(X0, planes), (X0[:, :3000], planes[:20])]
        seq = [o.run_attitude_simplified(*a, keep_path=True) for o, a in zip((r1, c1), args)]
        par = [None, None]

        def work(t):
            for _ in range(3):
                par[t] = (r1, c1)[t].run_attitude_simplified(*args[t], keep_path=True)
        ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for s, p in zip(seq, par):
            for key in KEYS:
                assert _same(s[key], p[key]), key
        # model switching: simplified attitude -> affine -> simplified attitude ('diagonal', then 'full' again: the last set wins)
        A = np.array([[1.0, 0.0], [H, 1.0]])
        B = np.array([[H / 0.028], [0.0]])
        Xa = np.stack([rng.uniform(k[0], k[-1], 500) for k in chans[0][0]])
        r1.set_model(A, B, q=np.ones(2))
        got = r1.run(Xa, planes, "nearest", keep_path=True)
        ref = rollout_refs.rollout(chans[0][0], chans[0][1], chans[0][2], chans[0][3], A, B, Xa, planes, "nearest", q=np.ones(2))
        assert _same(got["X_final"], ref[0]) and _same(got["cost"], ref[1]) and _same(got["U_path"], ref[3])
        with pytest.raises(hjbdp.HjbError, match="set_model"):
            r1.run_attitude_simplified(X0[:, :10], planes)
        _set(r1, r2, r3, 1, "diagonal")
        _check_bits(r1.run_attitude_simplified(X0[:, :300], planes, keep_path=True), _twin(chans, 1, "diagonal", X0[:, :300], planes))
        _set(r1, r2, r3, 2)
        again = r1.run_attitude_simplified(X0, planes, keep_path=True)
        for key in KEYS:
            assert _same(again[key], one[key]), key
        with pytest.raises(hjbdp.HjbError, match="D == 6"):
            r1.set_attitude_model([0.02, 0.02, 0.02], 0.005)
        assert _same(r1.run_attitude_simplified(X0[:, :50], planes)["X_final"], one["X_final"][:, :50])
        # channels 2 and 3 are ordinary objects throughout: channel 2 runs its own affine loop while attached
        r2.set_model(A, B)
        X2 = np.stack([rng.uniform(k[0], k[-1], 100) for k in chans[1][0]])
        g2 = r2.run(X2, planes, "nearest")
        assert _same(g2["X_final"], rollout_refs.rollout(chans[1][0], chans[1][1], chans[1][2], chans[1][3], A, B, X2, planes, "nearest")[0])
        assert _same(r1.run_attitude_simplified(X0[:, :50], planes)["X_final"], one["X_final"][:, :50])
    # one-plane channels (a stationary policy)
    chans1 = _channels(rng, np.uint8, n_planes=1)
    with _Three(chans1) as (r1, r2, r3):
        _set(r1, r2, r3)
        _check_bits(r1.run_attitude_simplified(X0[:, :300], np.zeros(K, int), keep_path=True), _twin(chans1, 1, "full", X0[:, :300], np.zeros(K, int)))


@pytest.mark.parametrize("dynamics", ["full", "diagonal"])
def test_starts_that_overflow_during_the_run(built, dynamics):
    """finite starts that leave double range on their own (rates of 1e200: w x (J w) overflows in the first stage and the rates
    become inf / NaN): the outputs are non-finite or clamped exactly as the twin's (NaN = NaN), the status is OK and the ordinary
    starts beside them are untouched.  Ordinary arithmetic: find_cell clamps every query and sends NaN to cell 0, so no read leaves
    the label arrays."""
    rng = np.random.default_rng(11)
    chans = _channels(rng, np.uint8)
    X0 = _starts(rng, 256)
    X0[0:3, 3] = [1e200, -1e200, 1e200]
    X0[1, 4] = -1e308
    X0[0:3, 5] = [1e160, 1e160, -1e160]
    X0[3, 6] = 5.0                                             # a quaternion component beyond asin's domain: clamped
    X0[3:7, 7] = [1e200, 0.0, -1e300, 1.0]
    K = 12
    planes = rng.integers(0, 3, size=K)
    hot = [3, 4, 5, 6, 7]
    with _Three(chans) as (r1, r2, r3):
        _set(r1, r2, r3, 1, dynamics)
        out = r1.run_attitude_simplified(X0, planes, keep_path=True)
        clean = r1.run_attitude_simplified(np.delete(X0, hot, axis=1), planes, keep_path=True)
    _check_bits(out, _twin(chans, 1, dynamics, X0, planes))
    assert not np.isfinite(out["X_final"][:, 3]).all()
    keep = np.delete(np.arange(256), hot)
    assert np.isfinite(out["X_final"][:, keep]).all() and np.isfinite(out["cost"][keep]).all()
    assert _same(out["X_path"][keep], clean["X_path"]) and _same(out["cost"][keep], clean["cost"])


def test_attached_objects_may_be_destroyed(built):
    """the lifetime rule of include/hjbdp.h: the model keeps what it reads of rollout_2 and rollout_3 alive, so closing them while
    attached is safe and changes nothing; new objects created meanwhile do not disturb it"""
    import hjbdp
    rng = np.random.default_rng(12)
    chans = _channels(rng, np.int32)
    X0 = _starts(rng, 2000)
    K = 25
    planes = rng.integers(0, 3, size=K)
    ref = _twin(chans, 1, "full", X0, planes)
    with _Three(chans) as (r1, r2, r3):
        _set(r1, r2, r3)
        r2.close()
        r3.close()
        other = _channels(rng, np.int32)
        with _Three(other) as (o1, o2, o3):                    # fresh allocations where the closed objects' would have been freed
            _set(o1, o2, o3)
            o1.run_attitude_simplified(X0, planes)
            _check_bits(r1.run_attitude_simplified(X0, planes, keep_path=True), ref)
        _check_bits(r1.run_attitude_simplified(X0, planes, keep_path=True), ref)
        with pytest.raises(hjbdp.HjbError, match="null handle"):
            _set(r1, r2, r3)                                   # closed objects are NULL handles
        _check_bits(r1.run_attitude_simplified(X0, planes, keep_path=True), ref)       # ... and the refusal changed nothing


def test_refusals_with_a_device(built):
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(13)
    chans = _channels(rng, np.uint8)
    X0 = _starts(rng, 64)

    def refused(fn, *needles):
        with pytest.raises(hjbdp.HjbError) as ei:
            fn()
        assert ei.value.status == _abi.HJB_E_INVALID, str(ei.value)
        for nd in needles:
            assert nd in str(ei.value), (nd, str(ei.value))

    with _Three(chans) as (r1, r2, r3):
        refused(lambda: r1.run_attitude_simplified(X0, [0]), "set_attitude_simplified_model")
        refused(lambda: _set(r1, r1, r3), "same object")
        refused(lambda: _set(r1, r2, r2), "same object")
        refused(lambda: _set(r1, r2, r1), "same object")
        refused(lambda: r1.run_attitude_simplified(X0, [0]), "set_attitude_simplified_model")     # a refused set leaves no model behind
        # label types must agree; D = 2 and n_u = 1 on all three
        k, lab, ut, base = chans[1]
        with hjbdp.Rollout(k, lab.astype(np.uint16), ut, index_base=base) as y16:
            refused(lambda: _set(r1, y16, r3), "rollout_2", "label")
            refused(lambda: _set(r1, r2, y16), "rollout_3", "label")
            refused(lambda: _set(y16, r2, r3), "label")
        with hjbdp.Rollout(k, lab, np.concatenate([ut, ut], axis=1), index_base=base) as y2:
            refused(lambda: _set(r1, y2, r3), "n_u == 1", "rollout_2")
            refused(lambda: _set(y2, r2, r3), "n_u == 1", "rollout_1")
        k3 = np.linspace(-1, 1, 3)
        with hjbdp.Rollout([k3] * 3, np.ones(27, np.uint8), np.zeros((1, 1)), index_base=1) as d3:
            refused(lambda: _set(r1, r2, d3), "D == 2", "rollout_3")
        # the argument refusals, through the Python wrapper this time
        refused(lambda: _set(r1, r2, r3, inertia=np.zeros((3, 3))), "inertia is singular")
        refused(lambda: _set(r1, r2, r3, h=0.0), "h =")
        refused(lambda: _set(r1, r2, r3, S=0), "substeps")
        refused(lambda: _set(r1, r2, r3, S=2, dyn="diagonal"), "substeps")
        refused(lambda: r1.set_attitude_simplified_model(r2, r3, INERTIA, H, qt=[1.0, np.nan, 1.0]), "qt")
        _set(r1, r2, r3)
        assert r1.run_attitude_simplified(X0, [0] * 5)["X_final"].shape == (7, 64)
        for planes in ([0, 3], [-1]):
            refused(lambda: r1.run_attitude_simplified(X0, planes), "plane_of_step")
        Xn = X0.copy()
        Xn[4, 3] = np.nan
        refused(lambda: r1.run_attitude_simplified(Xn, [0]), "not finite")
        Xn[4, 3] = np.inf
        refused(lambda: r1.run_attitude_simplified(Xn, [0]), "not finite")
        # every other run on a K20 object, and this run on any other object
        refused(lambda: r1.run(X0[:2], [0], "nearest"), "hjb_rollout_run_attitude_simplified")
        refused(lambda: r1.run_attitude(X0, [0]), "hjb_rollout_run_attitude_simplified")
        refused(lambda: r1.run_pos_att(np.ones((13, 2)), [0]), "hjb_rollout_run_attitude_simplified")
        refused(lambda: r1.run_position(np.ones((6, 2)), [0]), "hjb_rollout_run_attitude_simplified")
        refused(lambda: r2.run_attitude_simplified(X0, [0]), "set_attitude_simplified_model")     # the model lives on rollout_1 alone
        r2.set_model(np.eye(2), np.ones((2, 1)))
        refused(lambda: r2.run_attitude_simplified(X0, [0]), "hjb_rollout_run")
        n_sub, table = np.ones(2, np.int32), np.ones((2, 1, 32))
        r2.set_position_model(r1, r3, n_sub, table)            # the position model on the same kind of object (D = 2, n_u = 1)
        refused(lambda: r2.run_attitude_simplified(X0, [0]), "hjb_rollout_run_position")
        _set(r2, r1, r3)                                       # ... and replaced: the last model set wins
        assert r2.run_attitude_simplified(X0, [0, 1])["X_final"].shape == (7, 64)
        refused(lambda: r2.run_position(np.ones((6, 2)), [0]), "hjb_rollout_run_attitude_simplified")
        # plane_of_step indexes the planes of all three channels: with a one-plane channel 3 only plane 0 is left
        kz, labz, utz, basez = chans[2]
        with hjbdp.Rollout(kz, labz[:, :1], utz, index_base=basez) as z1:
            _set(r1, r2, z1)
            refused(lambda: r1.run_attitude_simplified(X0, [0, 1]), "plane_of_step[1] = 1", "[0, 1)")
            assert r1.run_attitude_simplified(X0, [0, 0])["X_final"].shape == (7, 64)
