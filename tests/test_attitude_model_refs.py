"""CPU tests of HJB_MODEL_QUAT_EULER321 at its branch points (no GPU): the edge problems of tests/attitude_model_refs.py reach every
branch of canon_atan2f / canon_asinf, the twin's two functions hold at their own edges, and the twin's whole model agrees with the
same kinematics in float64.  tests/test_gpu_attitude_model.py then holds the stage kernels to the twin bit for bit on these problems."""
import numpy as np
import pytest

import attitude_model_refs as amr

f32 = np.float32
FORMS = tuple(amr.FORMS)
# The twin's read-out stages against the float64 truth, max over the states with |s| <= 0.99 and the three angles, measured on
# the edge problems: k15 9.13e-07, k3w 8.08e-07, k3 8.24e-07 rad (pitch each time; yaw / roll <= 6.3e-07).  Asserted: 4 x the
# largest.  A wrong sign, a swapped component or a wrong quadrant moves an angle by >= 1e-2 rad on thousands of states.
READOUT_MEASURED = 9.13e-07
READOUT_BOUND = 4 * READOUT_MEASURED


@pytest.fixture(scope="module")
def orc(built):
    from hjbdp import _abi
    from oracle import c_oracle
    return _abi, c_oracle


_READOUTS = {}


def _readouts(orc, form):
    """(zero-cost spec, the twin's three read-out stages [3, nS], their labels), computed once per module and never written to."""
    if form not in _READOUTS:
        _abi, c_oracle = orc
        z = amr.edge_model_problem(form, costs=False)
        got = [c_oracle.backup_stage(_abi, z, amr.readout_terminal(z, a)) for a in range(3)]
        J, idx = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
        J.setflags(write=False)
        idx.setflags(write=False)
        _READOUTS[form] = (z, J, idx)
    return _READOUTS[form]


@pytest.mark.parametrize("form", FORMS)
def test_edge_problems_reach_every_class(form):
    """>= 20 states in every branch class of each of the three calls; |s| > 1 with either sign; the tables as the issue asks."""
    spec = amr.edge_model_problem(form)
    counts = amr.assert_classes(spec)
    assert set(counts["yaw"]) - {"x_neg_zero"} == set(amr.ATAN2_CLASSES) and set(counts["pitch"]) == set(amr.ASIN_CLASSES)
    assert min(counts["pitch"]["s_above_one"], counts["pitch"]["s_below_minus_one"]) >= amr.CLASS_FLOOR
    assert spec.model["kind"] == "quat_euler321" and spec.n[:3] == amr.FORMS[form]["n_ang"] and min(spec.n[:3]) >= 8
    pitch = np.asarray(spec.knots[1]).astype(f32)
    assert pitch[0] == -amr.HALF_PI and pitch[-1] == amr.HALF_PI and np.any(pitch == 0)
    assert spec.knots[0][0] == f32(-3.1) and spec.knots[0][-1] == f32(3.1) and spec.knots[2][-1] == f32(3.1)
    nrm = np.sqrt(sum(np.asarray(t, dtype=np.float64) ** 2 for t in spec.model["tables"]))
    assert nrm.min() >= 0.9 * (1 - 1e-6) and nrm.max() <= 1.1 * (1 + 1e-6) and np.count_nonzero(np.abs(nrm - 1) > 0.01) >= 100


def test_the_reference_grid_reaches_none_of_them(orc):
    """Why the edge problems exist: on Solver_attitude's own grid (angles within +-35 degrees) no atan2 argument is swapped,
    negative in x, zero in x or equal in magnitude, and every asin argument lies below 0.5 - the classifier says so.  (Only the
    tan(pi/8) reduction is reached there: yaw and roll pass 22.5 degrees.)"""
    import hjbdp
    sa = hjbdp.Solver_attitude(n_mesh_w=6, n_mesh_q=8)
    c = amr.classify(*amr.model_inputs(sa.build_spec_model()))
    for call in ("yaw", "roll"):
        assert all(c[call][k] == 0 for k in ("swap", "x_neg", "x_zero", "den_zero", "ay_eq_ax")), c[call]
    assert all(c["pitch"][k] == 0 for k in ("a_above_half", "a_eq_one", "s_above_one", "s_below_minus_one")), c["pitch"]


def test_the_tabulated_mirror_clips_likewise():
    """Solver_attitude.build_spec_full with a pitch axis from -90 to 90 degrees: wherever the restated pitch argument exceeds 1 in
    magnitude (a hundred states of this small grid) the tabulated next pitch is +-float32(pi/2), not NaN - the same function as
    the on-the-fly model's."""
    import hjbdp
    sa = hjbdp.Solver_attitude(n_mesh_w=3, n_mesh_q=9)
    sa.pitch_min, sa.pitch_max = -90.0, 90.0
    s = np.transpose(amr.arguments_f32(*amr.model_inputs(sa.build_spec_model()))["s"], (3, 4, 5, 0, 1, 2))      # (w1, w2, w3 | angles)
    over = np.abs(s) > 1
    assert np.count_nonzero(s > 1) >= amr.CLASS_FLOOR and np.count_nonzero(s < -1) >= amr.CLASS_FLOOR
    with np.errstate(invalid="raise"):
        pitch_n = np.asarray(sa.build_spec_full().next_terms[4][0].data)
    assert pitch_n.shape == s.shape and np.all(np.isfinite(pitch_n))
    assert np.array_equal(pitch_n[over], np.where(s[over] > 0, amr.HALF_PI, -amr.HALF_PI))
    assert np.array_equal(pitch_n[~over], np.arcsin(s[~over]))


def _ulps(got, ref64):
    return np.abs(got.astype(np.float64) - ref64) / np.spacing(np.abs(ref64).astype(f32)).astype(np.float64)


def test_the_twins_atan2_at_its_edges(orc):
    """canon_atan2f on both float32 neighbours of |y| = |x| and of r = tan(pi/8), on |y| == |x|, on both arguments zero and on
    every sign combination of zeros: < 4 ulp of float64 libm (the bound of test_host_solvers.py), except where it departs by
    contract (include/hjbdp.h) - a zero of either sign counts as positive."""
    _abi, c_oracle = orc
    up, dn = (lambda v: np.nextafter(f32(v), f32(np.inf))), (lambda v: np.nextafter(f32(v), f32(0)))
    T = amr.TAN_PI_8
    pairs = []
    for m in (f32(1), f32(0.3), f32(7.5), f32(3e-12), f32(2e9)):
        pairs += [(m, m), (up(m), m), (dn(m), m), (m, up(m)), (m, dn(m))]                    # the swap decision and |y| == |x|
        pairs += [(T * m, m), (up(T * m), m), (dn(T * m), m), (m, T * m), (m, up(T * m)), (m, dn(T * m))]      # r about tan(pi/8)
        pairs += [(f32(0), m), (m, f32(0)), (f32(1e-30) * m, m), (m, f32(1e-30) * m)]          # zeros and r that underflows
    pairs += [(f32(0), f32(0))]                                                                  # den == 0
    mag = np.array(pairs, dtype=f32)
    sgn = np.array([(sy, sx) for sy in (1, -1) for sx in (1, -1)], dtype=f32)
    yx = (mag[:, None, :] * sgn[None, :, :]).reshape(-1, 2)                                  # -1 * 0 = -0: every sign of zero
    y, x = np.ascontiguousarray(yx[:, 0]), np.ascontiguousarray(yx[:, 1])
    r1 = (np.minimum(np.abs(y), np.abs(x)) / np.maximum(np.abs(y), np.abs(x)).clip(f32(1e-37))).astype(f32)
    assert np.count_nonzero(r1 > T) >= 40 and np.count_nonzero((r1 <= T) & (r1 > f32(0.4))) >= 40     # both sides are there
    assert np.count_nonzero((y == 0) & (x == 0)) == 4 and np.count_nonzero(np.signbit(y) & (y == 0)) >= 10
    got = c_oracle.canon_eval(_abi, "atan2", y, x)
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    yz, xz = y == 0, x == 0
    dep_pi = yz & np.signbit(y) & (x < 0)                       # libm: -pi
    dep_zero = yz & xz & np.signbit(x)                          # libm: +-pi
    assert np.count_nonzero(dep_pi) == 5 and np.count_nonzero(dep_zero) == 2
    assert np.all(got[dep_pi] == amr.PI) and np.all(ref[dep_pi] == -np.pi)
    assert np.all(got[dep_zero] == 0) and np.all(np.abs(ref[dep_zero]) == np.pi)
    rest = ~(dep_pi | dep_zero)
    assert _ulps(got[rest], ref[rest]).max() < 4
    assert not np.any(np.signbit(got[yz]))                      # y = -0 never gives a negative result (libm: -0 / -pi)
    assert np.all(got[yz & (x < 0)] == amr.PI) and np.all(got[xz & (y > 0)] == amr.HALF_PI) and np.all(got[xz & (y < 0)] == -amr.HALF_PI)
    # odd in y, and reflected about pi / 2 in x, bit for bit, wherever y is not a zero
    nz = ~yz
    assert np.array_equal(c_oracle.canon_eval(_abi, "atan2", -y[nz], x[nz]), -got[nz])
    eq = np.abs(y) == np.abs(x)
    assert np.all(np.abs(got[eq & nz & (x > 0)]) == f32(0.78539816339744831))


def test_the_twins_asin_at_its_edges(orc):
    """canon_asinf on both neighbours of 0.5, at +-0.5, +-0, +-1 and below 1: < 4 ulp of float64 libm.  The model's pitch call
    (clamped) equals it wherever |s| <= 1 and gives +-float32(pi/2) exactly at 1 + 1 ulp and 1 + 2 ulp."""
    _abi, c_oracle = orc
    one_up = np.nextafter(f32(1), f32(2))
    mags = [f32(0), f32(1e-30), f32(1e-4), f32(0.25), np.nextafter(f32(0.5), f32(0)), f32(0.5), np.nextafter(f32(0.5), f32(1)),
            f32(0.75), f32(0.99), np.nextafter(np.nextafter(f32(1), f32(0)), f32(0)), np.nextafter(f32(1), f32(0)), f32(1)]
    v = np.array([s * m for m in mags for s in (f32(1), f32(-1))], dtype=f32)
    got = c_oracle.canon_eval(_abi, "asin", v)
    ref = np.arcsin(v.astype(np.float64))
    assert _ulps(got, ref).max() < 4
    assert got[v == 1] == amr.HALF_PI and got[v == -1] == -amr.HALF_PI and np.all(got[v == 0] == 0)
    assert np.array_equal(got[0::2], -got[1::2])                                     # odd, bit for bit
    rng = np.random.default_rng(5)
    u = np.concatenate([v, rng.uniform(-1, 1, 20000).astype(f32)])
    assert np.array_equal(c_oracle.canon_eval(_abi, "pitch", u).view(np.uint32), c_oracle.canon_eval(_abi, "asin", u).view(np.uint32))
    over = np.array([one_up, np.nextafter(one_up, f32(2)), f32(1.5), -one_up, -np.nextafter(one_up, f32(2)), f32(-1.5)], dtype=f32)
    assert over[0] - 1 == np.spacing(f32(1)) and over[1] - 1 == 2 * np.spacing(f32(1))
    assert np.array_equal(c_oracle.canon_eval(_abi, "pitch", over), np.array([amr.HALF_PI] * 3 + [-amr.HALF_PI] * 3, dtype=f32))


@pytest.mark.parametrize("form", FORMS)
def test_the_restatement_is_what_the_twin_evaluates(orc, form):
    """The classifier speaks about the twin's own arguments: the twin's functions applied to the restated arguments give, on EVERY
    state, the twin's read-out stage up to the rounding of one interpolation weight and one lerp.  The weight t = (q - k) * rdx
    carries four roundings and v1 - v0 a fifth: |t| W 5 u with u = 2^-24, |t| <= 1.1 (the angles reach +-pi, the knots +-3.1), cell
    width W <= 0.886; the lerp's own rounding is half an ulp of a result below 4: 2.9e-7 + 1.2e-7 < 4.2e-7 rad."""
    _abi, c_oracle = orc
    z, J, idx = _readouts(orc, form)
    a = amr.arguments_f32(*amr.model_inputs(z))
    flat = lambda v: np.ascontiguousarray(v.reshape(-1, order="F"))
    ang = [c_oracle.canon_eval(_abi, "atan2", flat(a["yaw"][0]), flat(a["yaw"][1])), c_oracle.canon_eval(_abi, "pitch", flat(a["s"])),
           c_oracle.canon_eval(_abi, "atan2", flat(a["roll"][0]), flat(a["roll"][1]))]
    assert max(float(np.diff(np.asarray(z.knots[k])).max()) for k in range(3)) <= 0.886
    for k in range(3):
        assert np.all(np.isfinite(J[k])), (k, np.count_nonzero(~np.isfinite(J[k])))
        err = np.abs(J[k].astype(np.float64) - ang[k].astype(np.float64))
        print(form, "angle", k, "max |read-out - restated angle| = %.3g" % err.max())
        assert err.max() < 4.2e-7, (k, err.max(), int(err.argmax()))
    assert np.all(idx == 1)                                       # zero costs: every control ties, the first one wins


@pytest.mark.parametrize("form", FORMS)
def test_kinematics_against_float64(orc, form):
    """The twin's next angles (read-out stages: zero costs, J_next = the knot of one angle axis) against the same kinematics in
    float64 with numpy's arctan2 / arcsin, on the states whose float64 |s| <= 0.99 (beyond, asin and the gimbal-locked atan2 are
    ill-conditioned; the bit comparisons cover those states).  Yaw and roll are compared modulo 2 pi: at y = +-0, x < 0 the
    result +pi for libm's -pi is the contract's departure, and the same angle.  Measured: READOUT_MEASURED (above) = 9.13e-07
    rad; asserted 4 x that = 3.65e-06 < 1e-4."""
    assert READOUT_BOUND < 1e-4
    z, J, _ = _readouts(orc, form)
    truth = amr.truth_f64(*amr.model_inputs(z))
    ok = (np.abs(truth[3]) <= 0.99).reshape(-1, order="F")
    assert ok.sum() > 0.75 * z.nS
    for k in range(3):
        e = J[k].astype(np.float64) - truth[k].reshape(-1, order="F")
        if k != 1:
            e = (e + np.pi) % (2 * np.pi) - np.pi
        worst = np.abs(e[ok]).max()
        print(form, "angle", k, "max |twin - float64| = %.3g" % worst)
        assert worst < READOUT_BOUND, (k, worst)
