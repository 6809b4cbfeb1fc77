"""GPU tests of the pos-att rollout (hjb_rollout_run_pos_att, K18 csrc/kernels_rollout_pos_att.h; hjbdp.Rollout.run_pos_att,
Solver_pos_att.get_optimal_paths): every instantiation bit-equal to tests/pos_att_rollout_refs.py, the policies simplified_run
leaves against the fixed-step host loop over the whole horizon (nominal and failure channel), chunking, threads, model switching,
starts that overflow during the run, the lifetime of the attached objects and every refusal that needs a device."""
import threading

import numpy as np
import pytest

import pos_att_rollout_refs as pr
import rollout_refs

pytestmark = pytest.mark.gpu

KEYS = ("X_final", "X_path", "F_path", "FM_path")
INERTIA = np.array([[0.02852, -0.0000837, 0.000014], [-0.0000837, 0.028317, -0.00029], [0.000014, -0.00029, 0.0245]])
MASS, T_DIST = 4.16, 9.65e-2


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


def _check_bits(out, ref):
    for key, r in zip(KEYS, ref):
        assert out[key] is not None and _same(out[key], r), (key, _diff(out[key], r))


def _channels(rng, dtype, n_labels, n_planes=3, long_axis=0):
    """three channels on small non-uniform sym_linspace grids (x, v, theta, w), random labels and thruster tables; long_axis > 0:
    channel x's position axis gets that many knots (the tables then exceed the 32 KiB LDS budget and the global-memory form runs)"""
    from hjbdp.matlab_compat import sym_linspace_pos_att
    chans = []
    for ch, tmax in enumerate((0.09, 0.10, 0.12)):
        nx = long_axis if (ch == 0 and long_axis) else int(rng.integers(5, 9))
        knots = [sym_linspace_pos_att(-0.2, 0.2, nx), sym_linspace_pos_att(-0.1, 0.1, int(rng.integers(4, 8))),
                 sym_linspace_pos_att(-tmax, tmax, int(rng.integers(4, 8))), sym_linspace_pos_att(-0.035, 0.035, int(rng.integers(4, 8)))]
        nS = int(np.prod([len(k) for k in knots]))
        base = int(rng.integers(0, 2))
        labels = rng.integers(base, base + n_labels, size=(nS, n_planes)).astype(dtype)
        ut = rng.choice([0.0, 0.13, -0.13], size=(n_labels, 4)) * rng.uniform(0.5, 1.0, size=(n_labels, 4))
        chans.append((knots, labels, ut, base))
    return chans


def _starts(rng, n):
    """offsets and rates mostly inside the grids, one start in ten outside them; attitudes of a few degrees"""
    X = np.empty((13, n))
    X[0:3] = rng.uniform(-0.18, 0.18, size=(3, n))
    X[3:6] = rng.uniform(-0.09, 0.09, size=(3, n))
    ang = rng.uniform(-0.08, 0.08, size=(3, n))
    X[10:13] = rng.uniform(-0.03, 0.03, size=(3, n))
    m = X[:, ::10].shape[1]
    X[0:3, ::10] = rng.uniform(-0.5, 0.5, size=(3, m))
    X[3:6, ::10] = rng.uniform(-0.3, 0.3, size=(3, m))
    ang[:, ::10] = rng.uniform(-0.4, 0.4, size=(3, m))
    X[10:13, ::10] = rng.uniform(-0.1, 0.1, size=(3, m))
    X[6:9] = np.sin(ang / 2)
    X[9] = np.sqrt(1.0 - (X[6:9] ** 2).sum(axis=0))
    return X


def _orbit(n_steps, h, S):
    from hjbdp.rollout import pos_att_orbit_table
    return pos_att_orbit_table(n_steps, h, S)


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
def test_every_instantiation_is_bit_equal_to_the_twin(built, dtype):
    rng = np.random.default_rng(180 + np.dtype(dtype).itemsize)
    h, K = 0.01, 64
    # LDS-staged tables, then the global-memory form (u16: 1,500 labels = 48 KB of thruster table; u8 / i32: 2,100 knots on an axis)
    for n_labels, long_axis in ((40, 0), (1500, 0) if dtype == np.uint16 else (40, 2100)):
        chans = _channels(rng, dtype, n_labels, long_axis=long_axis)
        X0 = _starts(rng, 4096)
        planes = rng.integers(0, 3, size=K)
        with _Three(chans) as (rx, ry, rz):
            for S in (1, 3):
                rsw, coef = _orbit(K, h, S)
                rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, h, rsw, coef, S)
                out = rx.run_pos_att(X0, planes, keep_path=True)
                ref = pr.rollout(chans, INERTIA, MASS, T_DIST, h, S, rsw, coef, X0, planes)
                _check_bits(out, ref)
                assert np.isfinite(out["X_final"]).all()
                assert len({out["F_path"][i].tobytes() for i in range(0, 4096, 64)}) > 32      # the starts do not fire alike
                if n_labels == 40 and not long_axis:            # the LDS-sized problem once more, forced into the global-memory form
                    rx.set_option("lds", 0)                     # channel x's object: the one the loop is run on
                    glob = rx.run_pos_att(X0, planes, keep_path=True)
                    rx.set_option("lds", 1)
                    _check_bits(glob, ref)
                    for key in KEYS:
                        assert _same(glob[key], out[key]), key


@pytest.fixture(scope="module")
def pos_att_solver(built):
    import hjbdp
    pa = hjbdp.Solver_pos_att()
    pa.simplified_run()
    return pa


@pytest.mark.parametrize("channel_x", ["channel_x_controller_1", "channel_x_controller_1_failure"])
def test_reference_policies_against_the_fixed_step_host_loop(pos_att_solver, channel_x):
    """the real thing: the policies simplified_run leaves, 1,024 starts around the default X0 plus the default X0 itself, all
    N_stage - 1 stages with the paths kept: bit-equal to pos_att_optimal_path_fixed for the default X0 and 7 more, to the twin for all"""
    from hjbdp.rollout import pos_att_channels, pos_att_default_X0, pos_att_optimal_path_fixed, pos_att_orbit_table
    pa = pos_att_solver
    rng = np.random.default_rng(7)
    n = 1025
    X0 = np.tile(pos_att_default_X0().reshape(13, 1), (1, n))
    X0[0:3, 1:] += rng.uniform(-0.05, 0.05, size=(3, n - 1))
    X0[3:6, 1:] += rng.uniform(-0.02, 0.02, size=(3, n - 1))
    ang = 2 * np.arcsin(X0[6:9, 1:]) + rng.uniform(-0.03, 0.03, size=(3, n - 1))
    X0[6:9, 1:] = np.sin(ang / 2)
    X0[9, 1:] = np.sqrt(1.0 - (X0[6:9, 1:] ** 2).sum(axis=0))
    X0[10:13, 1:] += rng.uniform(-0.01, 0.01, size=(3, n - 1))
    N = pa.N_stage
    T, X, F, FM = pa.get_optimal_paths(X0, channel_x=channel_x, keep_path=True)
    assert T.shape == (N,) and X.shape == (N, 13, n) and F.shape == (N, 12, n) and FM.shape == (N, 6, n)
    assert not F[N - 1].any() and not FM[N - 1].any() and np.isfinite(X).all()
    if channel_x.endswith("failure"):
        assert not F[:, 0].any()                                          # thruster 0 never fires
    else:
        assert F[:, :2].any()
    lean = pa.get_optimal_paths(X0[:, :65], channel_x=channel_x)
    assert _same(lean, X[N - 1, :, :65])
    for t in range(8):
        Th, Xh, Fh, FMh = pos_att_optimal_path_fixed(pa, X0[:, t], channel_x=channel_x)
        assert _same(T, Th)
        assert _same(X[:, :, t], Xh), _diff(X[:, :, t], Xh)
        assert _same(F[:, :, t], Fh), _diff(F[:, :, t], Fh)
        assert _same(FM[:, :, t], FMh), _diff(FM[:, :, t], FMh)
    chans = [(k, l, t, 1) for k, l, t in pos_att_channels(pa, channel_x)]
    rsw, coef = pos_att_orbit_table(N - 1, pa.h, 1)
    Xf, Xp, Fp, FMp = pr.rollout(chans, pa.InertiaM, pa.Mass, pa.T_dist, pa.h, 1, rsw, coef, X0, np.zeros(N - 1, int))
    assert _same(X.transpose(2, 1, 0), Xp), _diff(X.transpose(2, 1, 0), Xp)
    assert _same(F[:N - 1].transpose(2, 1, 0), Fp), _diff(F[:N - 1].transpose(2, 1, 0), Fp)
    assert _same(FM[:N - 1].transpose(2, 1, 0), FMp), _diff(FM[:N - 1].transpose(2, 1, 0), FMp)


def test_chunking_threads_and_model_switching(built):
    import hjbdp
    rng = np.random.default_rng(5)
    chans = _channels(rng, np.uint16, 30)
    X0 = _starts(rng, 5001)
    h, K, S = 0.01, 30, 2
    planes = rng.integers(0, 3, size=K)
    rsw, coef = _orbit(K, h, S)
    model = (INERTIA, MASS, T_DIST, h, rsw, coef, S)
    with _Three(chans) as (rx, ry, rz), _Three(chans) as (cx, cy, cz):
        rx.set_pos_att_model(ry, rz, *model)
        cx.set_pos_att_model(cy, cz, *model)
        cx.set_option("chunk", 1000)                          # 5,001 is not a multiple of the chunk
        one, chunked = rx.run_pos_att(X0, planes, keep_path=True), cx.run_pos_att(X0, planes, keep_path=True)
        for key in KEYS:
            assert _same(one[key], chunked[key]), key
        cx.set_option("chunk", 1)
        single = cx.run_pos_att(X0[:, :7], planes, keep_path=True)
        for key in KEYS:
            assert _same(single[key], one[key][..., :7] if key == "X_final" else one[key][:7]), key
        cx.set_option("chunk", 1000)
        lean = rx.run_pos_att(X0, planes)
        assert lean["X_path"] is None and lean["F_path"] is None and lean["FM_path"] is None and _same(lean["X_final"], one["X_final"])
        assert rx.run_pos_att(np.zeros((13, 0)), planes)["X_final"].shape == (13, 0)
        short = rx.run_pos_att(X0[:, :100], planes[:0], keep_path=True)           # no stages: X_final = X0
        assert _same(short["X_final"], X0[:, :100]) and short["X_path"].shape == (100, 13, 1)
        # plane_of_step None: every stage of the table on plane 0
        whole = rx.run_pos_att(X0[:, :64], keep_path=True)
        assert whole["X_path"].shape == (64, 13, K + 1)
        assert _same(whole["X_final"], rx.run_pos_att(X0[:, :64], np.zeros(K, int))["X_final"])
        # two objects on two threads = the same runs one after the other
        args = [(X0, planes), (X0[:, :3000], planes[:20])]
        seq = [o.run_pos_att(*a, keep_path=True) for o, a in zip((rx, cx), args)]
        par = [None, None]

        def work(t):
            for _ in range(3):
                par[t] = (rx, cx)[t].run_pos_att(*args[t], keep_path=True)
        ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for s, p in zip(seq, par):
            for key in KEYS:
                assert _same(s[key], p[key]), key
        # model switching, all three directions: pos-att -> affine -> pos-att -> attitude is refused (D = 4) and changes nothing
        A = np.array([[1, h, 0, 0], [0, 1, 0, 0], [0, 0, 1, h], [0, 0, 0, 1]], dtype=np.float64)
        B = rng.uniform(-0.02, 0.02, size=(4, 4))
        Xa = np.stack([rng.uniform(k[0], k[-1], 500) for k in chans[0][0]])
        rx.set_model(A, B, q=np.ones(4))
        got = rx.run(Xa, planes, "nearest", keep_path=True)
        ref = rollout_refs.rollout(chans[0][0], chans[0][1], chans[0][2], chans[0][3], A, B, Xa, planes, "nearest", q=np.ones(4))
        assert _same(got["X_final"], ref[0]) and _same(got["cost"], ref[1]) and _same(got["U_path"], ref[3])
        with pytest.raises(hjbdp.HjbError, match="set_model"):
            rx.run_pos_att(X0[:, :10], planes)
        rx.set_pos_att_model(ry, rz, *model)
        again = rx.run_pos_att(X0, planes, keep_path=True)
        for key in KEYS:
            assert _same(again[key], one[key]), key
        with pytest.raises(hjbdp.HjbError, match="D == 6"):
            rx.set_attitude_model([0.02, 0.02, 0.02], 0.005)
        assert _same(rx.run_pos_att(X0[:, :50], planes)["X_final"], one["X_final"][:, :50])
        # y and z are ordinary objects throughout: channel y runs its own affine loop while attached
        ry.set_model(A, B)
        Xy = np.stack([rng.uniform(k[0], k[-1], 100) for k in chans[1][0]])
        gy = ry.run(Xy, planes, "nearest")
        assert _same(gy["X_final"], rollout_refs.rollout(chans[1][0], chans[1][1], chans[1][2], chans[1][3], A, B, Xy, planes, "nearest")[0])
        assert _same(rx.run_pos_att(X0[:, :50], planes)["X_final"], one["X_final"][:, :50])
    # a 6-D object: attitude model -> pos-att is refused, the attitude model stays
    k3 = np.linspace(-1, 1, 3)
    with hjbdp.Rollout([k3] * 6, np.ones(3 ** 6, np.uint16), np.zeros((1, 3)), index_base=1) as r6, _Three(chans) as (rx, ry, rz):
        r6.set_attitude_model([0.02, 0.02, 0.02], 0.005)
        with pytest.raises(hjbdp.HjbError, match="D == 4"):
            r6.set_pos_att_model(ry, rz, *model)
        Xq = np.zeros((7, 4))
        Xq[6] = 1.0
        assert r6.run_attitude(Xq, [0, 0])["X_final"].shape == (7, 4)


def test_starts_that_overflow_during_the_run(built):
    """finite starts that leave double range on their own (position 1e300, rate 1e200: w x (J w) overflows in the first stage):
    the outputs are non-finite or clamped exactly as the twin's (NaN = NaN), the status is OK and the ordinary starts beside them
    are untouched.  Ordinary arithmetic: find_cell clamps every query and sends NaN to cell 0, so no read leaves the label arrays."""
    rng = np.random.default_rng(11)
    chans = _channels(rng, np.uint8, 25)
    X0 = _starts(rng, 256)
    X0[0, 3] = 1e300
    X0[1, 4] = -1e300
    X0[10:13, 5] = [1e200, -1e200, 1e200]
    X0[3, 6] = 1e308
    X0[6, 7] = 5.0                                             # a quaternion component beyond asin's domain: clamped
    h, K, S = 0.01, 12, 1
    planes = rng.integers(0, 3, size=K)
    rsw, coef = _orbit(K, h, S)
    with _Three(chans) as (rx, ry, rz):
        rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, h, rsw, coef, S)
        out = rx.run_pos_att(X0, planes, keep_path=True)
        clean = rx.run_pos_att(np.delete(X0, [3, 4, 5, 6, 7], axis=1), planes, keep_path=True)
    ref = pr.rollout(chans, INERTIA, MASS, T_DIST, h, S, rsw, coef, X0, planes)
    _check_bits(out, ref)
    assert not np.isfinite(out["X_final"][:, 5]).all()
    keep = np.delete(np.arange(256), [3, 4, 5, 6, 7])
    assert np.isfinite(out["X_final"][:, keep]).all() and _same(out["X_path"][keep], clean["X_path"])


def test_attached_objects_may_be_destroyed(built):
    """the lifetime rule of include/hjbdp.h: the model keeps what it reads of rollout_y and rollout_z alive, so closing them while
    attached is safe and changes nothing; new objects created meanwhile do not disturb it"""
    import hjbdp
    rng = np.random.default_rng(12)
    chans = _channels(rng, np.int32, 20)
    X0 = _starts(rng, 2000)
    h, K, S = 0.01, 25, 1
    planes = rng.integers(0, 3, size=K)
    rsw, coef = _orbit(K, h, S)
    ref = pr.rollout(chans, INERTIA, MASS, T_DIST, h, S, rsw, coef, X0, planes)
    with _Three(chans) as (rx, ry, rz):
        rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, h, rsw, coef, S)
        ry.close()
        rz.close()
        other = _channels(rng, np.int32, 20)
        with _Three(other) as (ox, oy, oz):                    # fresh allocations where the closed objects' would have been freed
            ox.set_pos_att_model(oy, oz, INERTIA, MASS, T_DIST, h, rsw, coef, S)
            ox.run_pos_att(X0, planes)
            _check_bits(rx.run_pos_att(X0, planes, keep_path=True), ref)
        _check_bits(rx.run_pos_att(X0, planes, keep_path=True), ref)
        with pytest.raises(hjbdp.HjbError, match="null handle"):
            rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, h, rsw, coef, S)       # closed objects are NULL handles
        _check_bits(rx.run_pos_att(X0, planes, keep_path=True), ref)                   # ... and the refusal changed nothing


def test_refusals_with_a_device(built):
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(13)
    chans = _channels(rng, np.uint8, 12)
    X0 = _starts(rng, 64)
    h, K, S = 0.01, 6, 2
    rsw, coef = _orbit(K, h, S)
    model = (INERTIA, MASS, T_DIST, h, rsw, coef, S)

    def refused(fn, *needles):
        with pytest.raises(hjbdp.HjbError) as ei:
            fn()
        assert ei.value.status == _abi.HJB_E_INVALID, str(ei.value)
        for nd in needles:
            assert nd in str(ei.value), (nd, str(ei.value))

    with _Three(chans) as (rx, ry, rz):
        refused(lambda: rx.run_pos_att(X0, [0]), "set_pos_att_model")
        refused(lambda: rx.set_pos_att_model(rx, rz, *model), "same object")
        refused(lambda: rx.set_pos_att_model(ry, ry, *model), "same object")
        refused(lambda: rx.set_pos_att_model(ry, rx, *model), "same object")
        refused(lambda: rx.run_pos_att(X0, [0]), "set_pos_att_model")                 # a refused set leaves no model behind
        # label types must agree; D = 4 and n_u = 4 on all three
        k, lab, ut, base = chans[1]
        with hjbdp.Rollout(k, lab.astype(np.uint16), ut, index_base=base) as y16:
            refused(lambda: rx.set_pos_att_model(y16, rz, *model), "rollout_y", "label")
            refused(lambda: rx.set_pos_att_model(ry, y16, *model), "rollout_z", "label")
            refused(lambda: y16.set_pos_att_model(ry, rz, *model), "label")
        with hjbdp.Rollout(k, lab, ut[:, :3], index_base=base) as y3:
            refused(lambda: rx.set_pos_att_model(y3, rz, *model), "n_u == 4", "rollout_y")
            refused(lambda: y3.set_pos_att_model(ry, rz, *model), "n_u == 4", "rollout_x")
        k3 = np.linspace(-1, 1, 3)
        with hjbdp.Rollout([k3] * 3, np.ones(27, np.uint8), np.zeros((1, 4)), index_base=1) as d3:
            refused(lambda: rx.set_pos_att_model(ry, d3, *model), "D == 4", "rollout_z")
        # the argument refusals, through the Python wrapper this time
        refused(lambda: rx.set_pos_att_model(ry, rz, np.zeros((3, 3)), MASS, T_DIST, h, rsw, coef, S), "inertia is singular")
        refused(lambda: rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, h, np.ones((3, 3)), coef, S), "rsw2eci is singular")
        refused(lambda: rx.set_pos_att_model(ry, rz, INERTIA, np.nan, T_DIST, h, rsw, coef, S), "mass")
        refused(lambda: rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, h, rsw, coef, 0), "substeps")
        refused(lambda: rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, h, rsw, coef[:-1], S), "n_nodes")
        refused(lambda: rx.set_pos_att_model(ry, rz, INERTIA, MASS, T_DIST, h, rsw, coef, 5), "n_nodes")
        rx.set_pos_att_model(ry, rz, *model)
        refused(lambda: rx.run_pos_att(X0, [0] * (K + 1)), "n_steps", "orbit table")
        assert rx.run_pos_att(X0, [0] * K)["X_final"].shape == (13, 64)
        for planes in ([0, 3], [-1]):
            refused(lambda: rx.run_pos_att(X0, planes), "plane_of_step")
        Xn = X0.copy()
        Xn[8, 3] = np.nan
        refused(lambda: rx.run_pos_att(Xn, [0]), "not finite")
        Xn[8, 3] = np.inf
        refused(lambda: rx.run_pos_att(Xn, [0]), "not finite")
        refused(lambda: rx.run(X0[:4], [0], "nearest"), "hjb_rollout_run_pos_att")
        refused(lambda: rx.run_attitude(np.ones((7, 2)), [0]), "hjb_rollout_run_pos_att")
        refused(lambda: ry.run_pos_att(X0, [0]), "set_pos_att_model")                 # the model lives on rollout_x alone
        # plane_of_step indexes the planes of all three channels: with a one-plane channel z only plane 0 is left
        kz, labz, utz, basez = chans[2]
        with hjbdp.Rollout(kz, labz[:, :1], utz, index_base=basez) as z1:
            rx.set_pos_att_model(ry, z1, *model)
            refused(lambda: rx.run_pos_att(X0, [0, 1]), "plane_of_step[1] = 1", "[0, 1)")
            assert rx.run_pos_att(X0, [0, 0])["X_final"].shape == (13, 64)
