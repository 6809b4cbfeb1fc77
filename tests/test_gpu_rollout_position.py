"""GPU tests of the position rollout (hjb_rollout_run_position, K19 csrc/kernels_rollout_position.h; hjbdp.Rollout.run_position,
Solver_position.get_optimal_paths): every instantiation bit-equal to tests/position_rollout_refs.py, the policies simplified_run
leaves against the two host loops, the off-schedule path, chunking, threads, model switching, the lifetime of the attached objects
and every refusal that needs a device."""
import threading

import numpy as np
import pytest

import position_rollout_refs as pr
import rollout_refs

pytestmark = pytest.mark.gpu

KEYS = ("X_final", "X_path", "A_path", "off_schedule")
H, K_TABLE = 0.005, 200
EPS = float(np.finfo(np.float64).eps)


def _same(a, b):
    """bit for bit (a NaN equals any NaN)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind in "iu" or b.dtype.kind in "iu":
        return a.dtype == b.dtype and np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def _diff(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return "shapes %r vs %r" % (a.shape, b.shape)
    bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).reshape(-1) & ~(np.isnan(a) & np.isnan(b)).reshape(-1))
    return "%d differ, first at %s: %r vs %r" % (bad.size, np.unravel_index(bad[0], a.shape), a.flat[bad[0]], b.flat[bad[0]]) if bad.size else ""


def _check_bits(out, ref):
    for key, r in zip(KEYS, ref):
        assert out[key] is not None and _same(out[key], r), (key, _diff(out[key], r))


@pytest.fixture(scope="module")
def table():
    from hjbdp.rollout import position_rkf45_table
    return position_rkf45_table(K_TABLE, H)


def _channels(rng, dtype, n_labels, n_planes=2, long_axis=0):
    """three channels on small non-uniform sym_linspace grids (x, v), random labels and acceleration tables; long_axis > 0:
    channel x's position axis gets that many knots (the tables then exceed the 32 KiB LDS budget and the global-memory form runs)"""
    from hjbdp.matlab_compat import sym_linspace_pos_att
    chans = []
    for ch in range(3):
        nx = long_axis if (ch == 0 and long_axis) else int(rng.integers(20, 40))
        knots = [sym_linspace_pos_att(-0.5, 0.5, nx), sym_linspace_pos_att(-0.5, 0.5, int(rng.integers(20, 40)))]
        nS = int(np.prod([len(k) for k in knots]))
        base = int(rng.integers(0, 2))
        labels = rng.integers(base, base + n_labels, size=(nS, n_planes)).astype(dtype)
        ut = rng.choice([0.0, 0.26, -0.26], size=(n_labels, 1)) * rng.uniform(0.5, 1.0, size=(n_labels, 1))
        chans.append((knots, labels, ut, base))
    return chans


def _starts(rng, n):
    """positions and velocities mostly inside the grids, one start in eight outside them (the reference's own start is)"""
    X = np.concatenate([rng.uniform(-0.45, 0.45, size=(3, n)), rng.uniform(-0.45, 0.45, size=(3, n))])
    m = X[:, ::8].shape[1]
    X[0:3, ::8] = rng.uniform(-1.5, 1.5, size=(3, m))
    X[3:6, ::8] = rng.uniform(-0.9, 0.9, size=(3, m))
    return X


class _Three:
    """three hjbdp.Rollout objects (channels x, y, z) as one context manager"""

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


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_every_instantiation_is_bit_equal_to_the_twin(built, table, dtype):
    rng = np.random.default_rng(190 + np.dtype(dtype).itemsize)
    n_sub, tab = table
    K = K_TABLE
    # LDS-staged tables, then the global-memory form (u16: 4,200 labels; u8 / i32: 2,100 knots on an axis)
    for n_labels, long_axis in ((40, 0), (4200, 0) if dtype == np.uint16 else (40, 2100)):
        chans = _channels(rng, dtype, n_labels, long_axis=long_axis)
        X0 = _starts(rng, 384)
        planes = rng.integers(0, 2, size=K)
        with _Three(chans) as (rx, ry, rz):
            rx.set_position_model(ry, rz, n_sub, tab)
            out = rx.run_position(X0, planes, keep_path=True)
            glob = None
            if n_labels == 40 and not long_axis:                # the LDS-sized problem once more, forced into the global-memory form
                rx.set_option("lds", 0)                         # channel x's object: the one the loop is run on
                glob = rx.run_position(X0, planes, keep_path=True)
                rx.set_option("lds", 1)
        ref = pr.rollout(chans, n_sub, tab, 1e-8, X0, planes)
        _check_bits(out, ref)
        if glob is not None:
            _check_bits(glob, ref)
            for key in KEYS:
                assert _same(glob[key], out[key]), key
        assert out["off_schedule"].dtype == np.int32 and (out["off_schedule"] == -1).all() and np.isfinite(out["X_final"]).all()
        assert len({out["A_path"][i].tobytes() for i in range(0, 384, 6)}) > 32         # the starts do not fire alike


@pytest.fixture(scope="module")
def position_solver(built):
    import hjbdp
    sp = hjbdp.Solver_position()
    sp.n_mesh_x = sp.n_mesh_v = 60
    sp.simplified_run(n_stages=200)
    return sp


def test_reference_policies_against_the_host_loops(position_solver):
    """the real thing: the policies simplified_run leaves on the reduced 61 x 61 grid, 1,024 starts inside and outside the grid plus
    the reference's start (-1 km: outside, clamped).  Every start bit-equal to position_optimal_path_fixed over 200 stages; the
    reference's start over 400 stages equal to get_optimal_path (the adaptive loop) within the CPU test's cap
    2 N n_sub eps max|X| with every acceleration column equal."""
    from hjbdp.rollout import position_optimal_path_fixed, position_rkf45_table
    sp = position_solver
    rng = np.random.default_rng(7)
    n, K = 1025, 200
    X0 = np.concatenate([rng.uniform(-0.6, 0.6, size=(3, n)), rng.uniform(-0.3, 0.3, size=(3, n))])
    X0[:, 0] = [-1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    T, X, F = sp.get_optimal_paths(X0, n_steps=K, keep_path=True)
    assert T.shape == (K + 1,) and X.shape == (6, K + 1, n) and F.shape == (3, K + 1, n)
    assert (sp.off_schedule == -1).all() and sp.off_schedule.dtype == np.int32 and sp.off_schedule_recomputed == 0
    assert not F[:, K].any() and np.isfinite(X).all() and set(np.unique(F)) <= set(sp.U_vector) | {0.0}
    assert len({F[:, :, i].tobytes() for i in range(n)}) > 16                  # the starts do not fire alike
    lean = sp.get_optimal_paths(X0[:, :65], n_steps=K)
    assert _same(lean, X[:, K, :65])
    tab = position_rkf45_table(K, sp.h, *sp.get_target_R0V0())
    for i in range(n):
        Th, Xh, Fh, off = position_optimal_path_fixed(sp, y0=X0[:, i], n_steps=K, table=tab)
        assert off == -1 and _same(T, Th)
        assert _same(X[:, :, i], Xh), (i, _diff(X[:, :, i], Xh))
        assert _same(F[:, :, i], Fh), (i, _diff(F[:, :, i], Fh))
    # the reference's start, no y0s: against the adaptive loop
    K = 400
    T, X, F = sp.get_optimal_paths(n_steps=K, keep_path=True)
    Tr, Xr, Fr = sp.get_optimal_path(n_steps=K)
    assert X.shape == (6, K + 1, 1) and _same(T, Tr) and sp.off_schedule.tolist() == [-1]
    cols_equal = int((F[:, :, 0] == Fr).all(axis=0).sum())
    dX = float(np.abs(X[:, :, 0] - Xr).max())
    cap = 2 * K * 5 * EPS * float(np.abs(Xr).max())
    print("reference start, %d stages: %d of %d acceleration columns equal, max |dX| = %.3g (cap %.3g)" % (K, cols_equal, K + 1, dX, cap))
    assert cols_equal == K + 1, cols_equal
    assert dX <= cap, (dX, cap)
    Th, Xh, Fh, off = position_optimal_path_fixed(sp, n_steps=K)
    assert off == -1 and _same(X[:, :, 0], Xh) and _same(F[:, :, 0], Fh)


def test_flag_path(position_solver, table):
    """tol = 1e-30: no error test leaves rkf45 its fourfold growth, so every start is flagged at stage 0 and get_optimal_paths
    returns the scalar get_optimal_path result for each"""
    sp = position_solver
    rng = np.random.default_rng(8)
    n, K = 8, 6
    X0 = np.concatenate([rng.uniform(-0.6, 0.6, size=(3, n)), rng.uniform(-0.3, 0.3, size=(3, n))])
    for keep in (True, False):
        got = sp.get_optimal_paths(X0, n_steps=K, keep_path=keep, tol=1e-30)
        assert sp.off_schedule.tolist() == [0] * n and sp.off_schedule_recomputed == n
        for i in range(n):
            Tr, Xr, Fr = sp.get_optimal_path(n_steps=K, y0=X0[:, i])
            if keep:
                assert _same(got[0], Tr) and _same(got[1][:, :, i], Xr) and _same(got[2][:, :, i], Fr), i
            else:
                assert _same(got[:, i], Xr[:, K]), i
    # the entry point itself: flagged at 0, and the run still completes on the schedule with tol = 1e-8's states
    from hjbdp.rollout import position_channels
    chans = [(k, l, t, 1) for k, l, t in position_channels(sp)]
    n_sub, tab = table
    with _Three(chans) as (rx, ry, rz):
        rx.set_position_model(ry, rz, n_sub, tab, 1e-30)
        flagged = rx.run_position(X0, np.zeros(K, int), keep_path=True)
        rx.set_position_model(ry, rz, n_sub, tab, 1e-8)
        clean = rx.run_position(X0, np.zeros(K, int), keep_path=True)
    assert (flagged["off_schedule"] == 0).all() and (clean["off_schedule"] == -1).all()
    assert _same(flagged["X_path"], clean["X_path"]) and _same(flagged["A_path"], clean["A_path"])
    _check_bits(flagged, pr.rollout(chans, n_sub, tab, 1e-30, X0, np.zeros(K, int)))
    # a start that overflows in the first stage: flagged there or in the next stage, exactly as the twin; not recomputed
    Xb = X0.copy()
    Xb[0, 2] = Xb[3, 2] = 1.7e308
    with _Three(chans) as (rx, ry, rz):
        rx.set_position_model(ry, rz, n_sub, tab)
        out = rx.run_position(Xb, np.zeros(K, int), keep_path=True)
    _check_bits(out, pr.rollout(chans, n_sub, tab, 1e-8, Xb, np.zeros(K, int)))
    assert 0 <= out["off_schedule"][2] <= 1 and (np.delete(out["off_schedule"], 2) == -1).all()
    assert not np.isfinite(out["X_final"][:, 2]).all() and _same(np.delete(out["X_path"], 2, axis=0), clean["X_path"][np.arange(n) != 2])
    Xf = sp.get_optimal_paths(Xb, n_steps=K)
    assert sp.off_schedule_recomputed == 0 and sp.off_schedule[2] >= 0 and _same(Xf, out["X_final"])


def test_chunking_threads_and_model_switching(built, table):
    import hjbdp
    rng = np.random.default_rng(5)
    chans = _channels(rng, np.uint16, 30)
    X0 = _starts(rng, 5001)
    n_sub, tab = table
    K = 30
    planes = rng.integers(0, 2, size=K)
    with _Three(chans) as (rx, ry, rz), _Three(chans) as (cx, cy, cz):
        rx.set_position_model(ry, rz, n_sub, tab)
        cx.set_position_model(cy, cz, n_sub, tab)
        cx.set_option("chunk", 1000)                          # 5,001 is not a multiple of the chunk
        one, chunked = rx.run_position(X0, planes, keep_path=True), cx.run_position(X0, planes, keep_path=True)
        for key in KEYS:
            assert _same(one[key], chunked[key]), key
        _check_bits(one, pr.rollout(chans, n_sub, tab, 1e-8, X0, planes))
        cx.set_option("chunk", 1)
        single = cx.run_position(X0[:, :7], planes, keep_path=True)
        for key in KEYS:
            assert _same(single[key], one[key][..., :7] if key == "X_final" else one[key][:7]), key
        cx.set_option("chunk", 1000)
        lean = rx.run_position(X0, planes)
        assert lean["X_path"] is None and lean["A_path"] is None and _same(lean["X_final"], one["X_final"])
        assert _same(lean["off_schedule"], one["off_schedule"])
        assert rx.run_position(np.zeros((6, 0)), planes)["X_final"].shape == (6, 0)
        short = rx.run_position(X0[:, :100], planes[:0], keep_path=True)            # no stages: X_final = X0
        assert _same(short["X_final"], X0[:, :100]) and short["X_path"].shape == (100, 6, 1) and (short["off_schedule"] == -1).all()
        # plane_of_step None: every stage of the table on plane 0
        whole = rx.run_position(X0[:, :64], keep_path=True)
        assert whole["X_path"].shape == (64, 6, K_TABLE + 1)
        assert _same(whole["X_final"], rx.run_position(X0[:, :64], np.zeros(K_TABLE, int))["X_final"])
        # two object triples on two threads = the same runs one after the other
        args = [(X0, planes), (X0[:, :3000], planes[:20])]
        seq = [o.run_position(*a, keep_path=True) for o, a in zip((rx, cx), args)]
        par = [None, None]

        def work(t):
            for _ in range(3):
                par[t] = (rx, cx)[t].run_position(*args[t], keep_path=True)
        ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for s, p in zip(seq, par):
            for key in KEYS:
                assert _same(s[key], p[key]), key
        # model switching: position -> affine -> position; the attitude and pos-att models are refused (D = 2) and change nothing
        A = np.array([[1.0, H], [0.0, 1.0]])
        B = np.array([[0.0], [H]])
        Xa = np.stack([rng.uniform(k[0], k[-1], 500) for k in chans[0][0]])
        rx.set_model(A, B, q=np.ones(2))
        got = rx.run(Xa, planes, "nearest", keep_path=True)
        ref = rollout_refs.rollout(chans[0][0], chans[0][1], chans[0][2], chans[0][3], A, B, Xa, planes, "nearest", q=np.ones(2))
        assert _same(got["X_final"], ref[0]) and _same(got["cost"], ref[1]) and _same(got["U_path"], ref[3])
        with pytest.raises(hjbdp.HjbError, match="set_model"):
            rx.run_position(X0[:, :10], planes)
        rx.set_position_model(ry, rz, n_sub, tab)
        again = rx.run_position(X0, planes, keep_path=True)
        for key in KEYS:
            assert _same(again[key], one[key]), key
        with pytest.raises(hjbdp.HjbError, match="D == 6"):
            rx.set_attitude_model([0.02, 0.02, 0.02], 0.005)
        with pytest.raises(hjbdp.HjbError, match="D == 4"):
            rx.set_pos_att_model(ry, rz, np.eye(3), 4.0, 0.1, H, np.eye(3), np.ones((3, 5)), 1)
        assert _same(rx.run_position(X0[:, :50], planes)["X_final"], one["X_final"][:, :50])
        # y and z are ordinary objects throughout: channel y runs its own affine loop while attached
        ry.set_model(A, B)
        Xy = np.stack([rng.uniform(k[0], k[-1], 100) for k in chans[1][0]])
        gy = ry.run(Xy, planes, "nearest")
        assert _same(gy["X_final"], rollout_refs.rollout(chans[1][0], chans[1][1], chans[1][2], chans[1][3], A, B, Xy, planes, "nearest")[0])
        assert _same(rx.run_position(X0[:, :50], planes)["X_final"], one["X_final"][:, :50])


def test_attached_objects_may_be_destroyed(built, table):
    """the lifetime rule of include/hjbdp.h: the model keeps what it reads of rollout_y and rollout_z alive, so closing them while
    attached is safe and changes nothing; new objects created meanwhile do not disturb it"""
    import hjbdp
    rng = np.random.default_rng(12)
    chans = _channels(rng, np.int32, 20)
    X0 = _starts(rng, 2000)
    n_sub, tab = table
    planes = rng.integers(0, 2, size=25)
    ref = pr.rollout(chans, n_sub, tab, 1e-8, X0, planes)
    with _Three(chans) as (rx, ry, rz):
        rx.set_position_model(ry, rz, n_sub, tab)
        ry.close()
        rz.close()
        other = _channels(rng, np.int32, 20)
        with _Three(other) as (ox, oy, oz):                    # fresh allocations where the closed objects' would have been freed
            ox.set_position_model(oy, oz, n_sub, tab)
            ox.run_position(X0, planes)
            _check_bits(rx.run_position(X0, planes, keep_path=True), ref)
        _check_bits(rx.run_position(X0, planes, keep_path=True), ref)
        with pytest.raises(hjbdp.HjbError, match="null handle"):
            rx.set_position_model(ry, rz, n_sub, tab)                                  # closed objects are NULL handles
        _check_bits(rx.run_position(X0, planes, keep_path=True), ref)                  # ... and the refusal changed nothing


def test_refusals_with_a_device(built, table):
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(13)
    chans = _channels(rng, np.uint8, 12)
    X0 = _starts(rng, 64)
    n_sub, tab = table
    K = 6
    model = (n_sub[:K], tab[:K])

    def refused(fn, *needles):
        with pytest.raises(hjbdp.HjbError) as ei:
            fn()
        assert ei.value.status == _abi.HJB_E_INVALID, str(ei.value)
        for nd in needles:
            assert nd in str(ei.value), (nd, str(ei.value))

    with _Three(chans) as (rx, ry, rz):
        refused(lambda: rx.run_position(X0, [0]), "set_position_model")
        refused(lambda: rx.set_position_model(rx, rz, *model), "same object")
        refused(lambda: rx.set_position_model(ry, ry, *model), "same object")
        refused(lambda: rx.run_position(X0, [0]), "set_position_model")               # a refused set leaves no model behind
        # label types must agree; D = 2 and n_u = 1 on all three
        k, lab, ut, base = chans[1]
        with hjbdp.Rollout(k, lab.astype(np.uint16), ut, index_base=base) as y16:
            refused(lambda: rx.set_position_model(y16, rz, *model), "rollout_y", "label")
            refused(lambda: rx.set_position_model(ry, y16, *model), "rollout_z", "label")
            refused(lambda: y16.set_position_model(ry, rz, *model), "label")
        with hjbdp.Rollout(k, lab, np.hstack([ut, ut]), index_base=base) as y2:
            refused(lambda: rx.set_position_model(y2, rz, *model), "n_u == 1", "rollout_y")
            refused(lambda: y2.set_position_model(ry, rz, *model), "n_u == 1", "rollout_x")
        k3 = np.linspace(-1, 1, 3)
        with hjbdp.Rollout([k3] * 3, np.ones(27, np.uint8), np.zeros((1, 1)), index_base=1) as d3:
            refused(lambda: rx.set_position_model(ry, d3, *model), "D == 2", "rollout_z")
            refused(lambda: d3.set_position_model(ry, rz, *model), "D == 2", "rollout_x")
        # the argument refusals, through the Python wrapper this time
        refused(lambda: rx.set_position_model(ry, rz, *model, tol=0.0), "tol")
        refused(lambda: rx.set_position_model(ry, rz, np.full(K, 6), tab[:K]), "n_sub[0] = 6")
        bad = tab[:K].copy()
        bad[3, 1, 0] = np.nan
        refused(lambda: rx.set_position_model(ry, rz, n_sub[:K], bad), "table element", "not finite")
        with pytest.raises(ValueError):
            rx.set_position_model(ry, rz, n_sub[:K], tab[:K + 1])
        rx.set_position_model(ry, rz, *model)
        refused(lambda: rx.run_position(X0, [0] * (K + 1)), "n_steps", "table covers %d stages" % K)
        assert rx.run_position(X0, [0] * K)["X_final"].shape == (6, 64)
        for planes in ([0, 2], [-1]):
            refused(lambda: rx.run_position(X0, planes), "plane_of_step")
        Xn = X0.copy()
        Xn[4, 3] = np.nan
        refused(lambda: rx.run_position(Xn, [0]), "X0 element %d is not finite" % (6 * 3 + 4))
        Xn[4, 3] = -np.inf
        refused(lambda: rx.run_position(Xn, [0]), "not finite")
        refused(lambda: rx.run(X0[:2], [0], "nearest"), "hjb_rollout_run_position")
        refused(lambda: rx.run_attitude(np.ones((7, 2)), [0]), "hjb_rollout_run_position")
        refused(lambda: rx.run_pos_att(np.ones((13, 2)), [0]), "hjb_rollout_run_position")
        refused(lambda: ry.run_position(X0, [0]), "set_position_model")               # the model lives on rollout_x alone
        # plane_of_step indexes the planes of all three channels: with a one-plane channel z only plane 0 is left
        kz, labz, utz, basez = chans[2]
        with hjbdp.Rollout(kz, labz[:, :1], utz, index_base=basez) as z1:
            rx.set_position_model(ry, z1, *model)
            refused(lambda: rx.run_position(X0, [0, 1]), "plane_of_step[1] = 1", "[0, 1)")
            assert rx.run_position(X0, [0, 0])["X_final"].shape == (6, 64)
