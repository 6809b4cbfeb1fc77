"""GPU tests of the linear attitude controller's batched rollout (hjb_attitude_linear_response, K21
csrc/kernels_rollout_attitude_linear.h; hjbdp.attitude_linear_response, Solver_attitude.linear_control_responses): every
instantiation bit-equal to tests/attitude_linear_rollout_refs.py with and without each optional output, the reference's constants
against the host mirror over the whole horizon, the same plant and the same cost as K17 and K20 sum, chunking, threads and a call
after a refusal."""
import ctypes as C
import threading

import numpy as np
import pytest

import attitude_linear_rollout_refs as al

pytestmark = pytest.mark.gpu

KEYS = ("X_final", "cost", "X_path", "U_path", "A_path")
INERTIA = np.array([0.02852, 0.028317, 0.0245])
H = 0.01
# full gains with off-diagonal terms, an error quaternion that mixes all four components
K_FULL = np.array([[0.21, -0.03, 0.02], [0.04, 0.18, -0.05], [-0.01, 0.06, 0.25]])
C_FULL = np.array([[0.9, 0.1, -0.2], [-0.15, 1.1, 0.05], [0.07, -0.12, 0.8]])
QC = np.array([[0.98, 0.1, -0.05, 0.12], [-0.1, 0.97, 0.15, -0.08], [0.05, -0.15, 0.99, 0.03], [0.3, 0.2, 0.1, 0.9]])
LIMIT = np.array([0.11, 0.07, 0.2])
WEIGHTS = np.array([6.0, 5.0, 4.0, 3.0, 6.0, 2.0, 4.0, 1.0, 0.5, 0.25])


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
        return "shapes %s and %s" % (a.shape, b.shape)
    bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b)))
    return "%d differ, first at %s: %r vs %r" % (bad.size, np.unravel_index(bad[0], a.shape), a.flat[bad[0]], b.flat[bad[0]]) if bad.size else ""


def _check_bits(out, ref, what=""):
    for key, r in zip(KEYS, ref):
        if out[key] is not None:
            assert _same(out[key], r), (what, key, _diff(out[key], r))


def _starts(n, seed):
    """rates to +-0.8 rad/s; rotations up to ~70 degrees about random axes; every third quaternion scaled to a norm between 0.5 and
    2; every fifth negated (negative q4: the same attitude); the last start's rates are 1e200 (they overflow in the first step)."""
    rng = np.random.default_rng(seed)
    X = np.empty((7, n))
    X[0:3] = rng.uniform(-0.8, 0.8, size=(3, n))
    ax = rng.normal(size=(3, n))
    ax /= np.sqrt((ax ** 2).sum(axis=0))
    th = rng.uniform(0, 1.2, size=n)
    X[3:6] = ax * np.sin(th / 2)
    X[6] = np.cos(th / 2)
    X[3:7, ::3] *= rng.uniform(0.5, 2.0, size=X[3:7, ::3].shape[1])
    X[3:7, ::5] *= -1.0
    if n > 1:
        X[0:3, n - 1] = [1e200, -1e200, 1e200]
    return X


def _raw(X0, n_steps, integrator, cost_form, K=K_FULL, Cg=C_FULL, qc=QC, u_limit=None, weights=WEIGHTS, outputs=KEYS[1:], chunk=0, h=H,
         inertia=INERTIA):
    """hjb_attitude_linear_response through ctypes with exactly the optional outputs named in `outputs`; the others are null
    pointers and come back as None."""
    import hjbdp
    from hjbdp import _abi
    lib = hjbdp.load_library()
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    col = lambda m: np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(-1, order="F"))
    X = np.ascontiguousarray(np.asarray(X0, dtype=np.float64).reshape(7, -1).T)
    nt, N = X.shape[0], int(n_steps)
    Xf = np.full((nt, 7), 7.0)
    bufs = {"cost": np.full(nt, 7.0), "X_path": np.full(nt * 7 * (N + 1), 7.0), "U_path": np.full(nt * 3 * N, 7.0), "A_path": np.full(nt * 3 * N, 7.0)}
    bufs = {k: (v if k in outputs else None) for k, v in bufs.items()}
    lim = None if u_limit is None else np.ascontiguousarray(u_limit, dtype=np.float64)
    wt = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    J = np.ascontiguousarray(inertia, dtype=np.float64)
    ms = C.c_double(-1.0)
    st = lib.hjb_attitude_linear_response(0, p(J), float(h), {"taylor": 0, "RK4": 1}[integrator], p(col(K)), p(col(Cg)),
                                          None if qc is None else p(col(qc)), p(lim), {"quat": 0, "angle": 1}[cost_form], p(wt), N, nt, p(X),
                                          p(Xf), p(bufs["cost"]), p(bufs["X_path"]), p(bufs["U_path"]), p(bufs["A_path"]), int(chunk),
                                          C.byref(ms))
    assert st == _abi.HJB_OK, (st, lib.hjb_rollout_last_error(None).decode())
    assert ms.value >= 0.0
    path = lambda a, rows, cols: None if a is None else a.reshape((nt, rows, cols), order="F")
    return {"X_final": Xf.T, "cost": bufs["cost"], "X_path": path(bufs["X_path"], 7, N + 1), "U_path": path(bufs["U_path"], 3, N),
            "A_path": path(bufs["A_path"], 3, N)}


@pytest.mark.parametrize("cost_form", ["quat", "angle"])
@pytest.mark.parametrize("integrator", ["taylor", "RK4"])
def test_every_instantiation_is_bit_equal_to_the_twin(built, integrator, cost_form):
    """integrator x cost form, each without a limit and with one that clips at least one torque on each side; 257 starts (two
    blocks, the second with one thread) x 37 steps with every subset of the optional outputs that leaves one out, none and all;
    1, 255 and 257 starts x 0, 1 and 37 steps; 257 starts in chunks of 100 (three launches, a remainder of 57)."""
    X0 = _starts(257, 31)
    free = al.control(X0, K_FULL, C_FULL, QC)
    for u_limit in (None, LIMIT):
        if u_limit is not None:                               # the limit clips on both sides already in the first step
            ok = np.isfinite(free).all(axis=0)
            assert (free[:, ok] > LIMIT[:, None]).any() and (free[:, ok] < -LIMIT[:, None]).any()
        refs = {N: al.rollout(INERTIA, H, integrator, K_FULL, C_FULL, X0, N, QC, u_limit, cost_form, WEIGHTS) for N in (0, 1, 37)}
        ref = refs[37]
        assert np.isnan(ref[0][:, 256]).any() and np.isfinite(ref[0][:, :256]).all() and np.isfinite(ref[1][:256]).all()
        if u_limit is not None:
            assert np.abs(ref[3][:256]).max(axis=(0, 2)).tolist() == LIMIT.tolist()
        subsets = [KEYS[1:], ()] + [tuple(k for k in KEYS[1:] if k != drop) for drop in KEYS[1:]]
        for outputs in subsets:
            out = _raw(X0, 37, integrator, cost_form, u_limit=u_limit, outputs=outputs)
            assert [k for k in KEYS[1:] if out[k] is not None] == list(outputs)
            _check_bits(out, ref, outputs)
        for nt in (1, 255, 257):
            for N in (0, 1, 37):
                out = _raw(X0[:, :nt], N, integrator, cost_form, u_limit=u_limit)
                r = refs[N]
                _check_bits(out, (r[0][:, :nt], r[1][:nt], r[2][:nt], r[3][:nt], r[4][:nt]), (nt, N))
        chunked = _raw(X0, 37, integrator, cost_form, u_limit=u_limit, chunk=100)
        _check_bits(chunked, ref, "chunk 100")
    # the defaults of the entry: qc NULL is the identity, weights NULL are zeros
    out = _raw(X0, 5, integrator, cost_form, qc=None, weights=None)
    _check_bits(out, al.rollout(INERTIA, H, integrator, K_FULL, C_FULL, X0, 5, np.eye(4), None, cost_form, None), "defaults")
    assert not out["cost"][:256].any()


def _reference_starts(n):
    """the reference's start, then n - 1 more: rates to +-0.8 rad/s, rotations up to ~70 degrees, unit quaternions"""
    from hjbdp.rollout import DEFAULT_X0_ATTITUDE
    rng = np.random.default_rng(21)
    X0 = np.empty((7, n))
    X0[0:3] = rng.uniform(-0.8, 0.8, size=(3, n))
    ax = rng.normal(size=(3, n))
    ax /= np.sqrt((ax ** 2).sum(axis=0))
    th = rng.uniform(0, 1.2, size=n)
    X0[3:6] = ax * np.sin(th / 2)
    X0[6] = np.cos(th / 2)
    X0[:, 0] = DEFAULT_X0_ATTITUDE
    return X0


def test_reference_constants_against_the_host_mirror(built):
    """Solver_attitude.linear_control_responses with every default (K = 0.2 I, C = I, qc = I, RK4, no limit, N = 6,000) from the
    reference's start and 63 more against hjbdp.rollout.linear_control_response, one start at a time: X and U with np.array_equal
    over all 6,000 steps, the angles (the library's fixed atan2 / asin against libm's, tested to <= 2 ulp of libm; 2 ulp at pi is
    8.9e-16) within 2e-15 rad.  The scalar mirror takes most of this test's time: 64 x 6,000 steps at about 1.5e4 steps/s."""
    import hjbdp
    from hjbdp.rollout import linear_control_response
    sa = hjbdp.Solver_attitude()
    X0 = _reference_starts(64)
    X, U, A = sa.linear_control_responses(X0)
    assert X.shape == (7, 6001, 64) and U.shape == (3, 6000, 64) and A.shape == (3, 6000, 64)
    assert np.abs(U).max() > 0.5                              # beyond the DP controllers' 0.11 N m: why the limit exists
    worst = 0.0
    for i in range(64):
        Xh, Uh, Ah = linear_control_response(sa, X0[:, i])
        assert np.array_equal(X[:, :, i], Xh), (i, _diff(X[:, :, i], Xh))
        assert np.array_equal(U[:, :, i], Uh), (i, _diff(U[:, :, i], Uh))
        worst = max(worst, float(np.abs(A[:, :, i] - Ah).max()))
    print("max |angle difference| over 64 x 6,000 steps = %.3g rad" % worst)
    assert worst <= 2e-15, worst
    # the lean form returns the same end states
    Xf, cost = sa.linear_control_responses(X0, keep_path=False)
    assert _same(Xf, X[:, -1, :]) and not cost.any()


def _k17_problem(rng):
    """a small 6-D grid with random labels into an all-zero torque table"""
    knots = []
    for lo, hi in [(-0.9, 0.9)] * 3 + [(-0.6, 0.6), (-0.4, 0.4), (-0.7, 0.7)]:
        knots.append(np.linspace(lo, hi, int(rng.integers(3, 5))))
    nS = int(np.prod([len(k) for k in knots]))
    return knots, rng.integers(1, 6, size=(nS, 1)).astype(np.uint8), np.zeros((5, 3))


def test_same_plant_and_same_cost_as_the_policy_kernels(built):
    """K = C = 0 against the policy kernels flying a policy that is zero everywhere, 257 starts x 300 steps, X_final and cost bit
    for bit: K17 (hjb_rollout_run_attitude, both integrators, q [7] and r [3]) with HJB_ATTL_COST_QUAT, and K20
    (hjb_rollout_run_attitude_simplified, 'diagonal', qw, qt, r) with HJB_ATTL_COST_ANGLE.  Then the two weightings
    Solver_attitude.linear_control_responses offers against the twin."""
    import hjbdp
    rng = np.random.default_rng(41)
    X0 = _starts(258, 43)[:, :257]                            # no overflowing start: every rate stays non-zero and finite
    Z = np.zeros((3, 3))
    q, r = WEIGHTS[:7], WEIGHTS[7:]
    planes = np.zeros(300, np.int32)
    knots, labels, ut = _k17_problem(rng)
    with hjbdp.Rollout(knots, labels, ut, index_base=1) as ro:
        for integ in ("taylor", "RK4"):
            ro.set_attitude_model(INERTIA, H, integ, q=q, r=r)
            want = ro.run_attitude(X0, planes, "nearest")
            got = hjbdp.attitude_linear_response(INERTIA, H, Z, Z, X0, 300, integrator=integ, cost_form="quat", weights=WEIGHTS)
            assert np.isfinite(want["cost"]).all() and want["cost"].min() > 0
            assert _same(got["X_final"], want["X_final"]), (integ, _diff(got["X_final"], want["X_final"]))
            assert _same(got["cost"], want["cost"]), (integ, _diff(got["cost"], want["cost"]))
    ros = []
    try:
        for n_w, n_t in ((9, 7), (12, 5), (6, 11)):
            kn = [np.linspace(-0.87, 0.87, n_w), np.linspace(-0.5, 0.5, n_t)]
            ros.append(hjbdp.Rollout(kn, rng.integers(1, 4, size=(n_w * n_t, 1)).astype(np.uint8), np.zeros((3, 1)), index_base=1))
        qw, qt, rr = WEIGHTS[0:3], WEIGHTS[3:6], WEIGHTS[6:9]
        ros[0].set_attitude_simplified_model(ros[1], ros[2], np.diag(INERTIA), H, 1, "diagonal", qw=qw, qt=qt, r=rr)
        want = ros[0].run_attitude_simplified(X0, planes)
    finally:
        for o in ros:
            o.close()
    got = hjbdp.attitude_linear_response(INERTIA, H, Z, Z, X0, 300, integrator="RK4", cost_form="angle", weights=WEIGHTS)
    assert np.isfinite(want["cost"]).all() and want["cost"].min() > 0
    assert _same(got["X_final"], want["X_final"]), _diff(got["X_final"], want["X_final"])
    assert _same(got["cost"], want["cost"]), _diff(got["cost"], want["cost"])
    # Solver_attitude's two weightings, with a limit and the taylor step, 100 steps
    sa = hjbdp.Solver_attitude()
    J = [sa.J1, sa.J2, sa.J3]
    Xu = _reference_starts(33)
    for cost, form, w in (("run", "quat", np.concatenate(sa.run_cost_weights())),
                          ("simplified", "angle", [sa.Q1, sa.Q2, sa.Q3, sa.Qt1, sa.Qt2, sa.Qt3, sa.R1, sa.R2, sa.R3, 0.0])):
        Xf, c = sa.linear_control_responses(Xu, T_final=0.5, u_limit=0.11, integrator="taylor", cost=cost, keep_path=False)
        ref = al.rollout(J, sa.h, "taylor", 0.2 * np.eye(3), np.eye(3), Xu, 100, None, [0.11] * 3, form, w)
        assert _same(Xf, ref[0]) and _same(c, ref[1]) and c.min() > 0, cost


def test_two_threads_and_a_call_after_a_refusal(built):
    """the entry is stateless: two host threads calling at once get what each call gives alone, and a refused call (here a
    negative limit, then an all-zero quaternion) leaves nothing behind for the next one."""
    import hjbdp
    from hjbdp import _abi
    X0 = _starts(3000, 51)
    args = [dict(X0=X0, n_steps=40, integrator="RK4", cost_form="quat", u_limit=LIMIT),
            dict(X0=X0[:, :1111], n_steps=25, integrator="taylor", cost_form="angle", chunk=500)]
    seq = [_raw(**a) for a in args]
    par = [None, None]
    errs = []

    def work(t):
        try:
            for _ in range(3):
                par[t] = _raw(**args[t])
        except BaseException as e:                            # an assertion in a thread would otherwise be lost
            errs.append(e)
    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for s, p in zip(seq, par):
        for key in KEYS:
            assert _same(s[key], p[key]), key
    for bad in (dict(u_limit=[0.1, -0.1, 0.1]), dict(X0=np.zeros((7, 2)))):
        with pytest.raises(hjbdp.HjbError) as ei:
            hjbdp.attitude_linear_response(INERTIA, H, K_FULL, C_FULL, bad.get("X0", X0), 40, qc=QC, u_limit=bad.get("u_limit", LIMIT))
        assert ei.value.status == _abi.HJB_E_INVALID, str(ei.value)
        again = _raw(**args[0])
        for key in KEYS:
            assert _same(seq[0][key], again[key]), key
    # the Python wrapper gives what the raw call gives
    out = hjbdp.attitude_linear_response(INERTIA, H, K_FULL, C_FULL, X0, 40, qc=QC, u_limit=LIMIT, integrator="RK4", cost_form="quat",
                                         weights=WEIGHTS, keep_path=True)
    for key in KEYS:
        assert _same(seq[0][key], out[key]), key
    assert out["device_ms"] > 0
