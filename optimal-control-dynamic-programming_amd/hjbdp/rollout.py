"""Closed-loop rollouts of the attitude, pos-att and position solvers with the policies the sweeps leave.

Host-side, scalar, O(N_stage) - the reference's own forward simulators restated without their plots:

  attitude-control/Solver_attitude.m   spacecraft_dynamics_list :600-620, next_stage_states :670-696,
                                       linear_control_response :508-591, get_optimal_path :744-833,
                                       get_optimal_path_simplified_testode45 :835-925
  pos-att/Solver_pos_att.m             get_thruster_on_off_optimal :404-449, get_optimal_path :452-730,
                                       get_target_R0V0 :734-753, update_RV_target :755-782,
                                       to_Moments_Forces :804-823, ECI2body :825-829, RSW2ECI :831-847
  position-control/Solver_position.m   get_optimal_path :189-311 on private/rkf45.m's schedule (position_optimal_path_fixed)
  attitude-control/test/test_simplified.m   "test on REAL SYSTEM DYNAMICS" :188-218 (attitude_optimal_path_simplified_fixed)

State conventions of the reference: the attitude state is X = [w1 w2 w3 q1 q2 q3 q4] with q4 the scalar part; the
pos-att state is X = [x(3) v(3) q(4) w(3)].  MATLAB's ode45 is Dormand-Prince 5(4) with RelTol 1e-3 / AbsTol 1e-6:
scipy's RK45 with the same tolerances is the same method (step-size control differs in detail, so trajectories agree to
the integrator tolerance, not bit for bit; no reference artefact exists for them - tests pin invariants instead).
"""
from __future__ import annotations

import math

import numpy as np

from .orbit import MU_EARTH, R_EARTH, propagate_kepler, state_from_elements


# ---- rigid body + quaternion kinematics (scalar-last quaternion) -----------------------------------------------------
def quat_rates(q, w):
    """Solver_attitude.m:617-620 / Solver_pos_att.m ode_eq: q_dot for q = [q1 q2 q3 q4], q4 scalar."""
    q1, q2, q3, q4 = q
    w1, w2, w3 = w
    return 0.5 * np.array([w3 * q2 - w2 * q3 + w1 * q4,
                           -w3 * q1 + w1 * q3 + w2 * q4,
                           w2 * q1 - w1 * q2 + w3 * q4,
                           -w1 * q1 - w2 * q2 - w3 * q3])


def rigid_body_rates_full(w, inertia, torque):
    """w_dot = J \\ (U - w x (J w)) with the full inertia matrix (Solver_attitude.m:913, Solver_pos_att.m ode_eq)."""
    w = np.asarray(w, dtype=np.float64)
    return np.linalg.solve(inertia, np.asarray(torque, dtype=np.float64) - np.cross(w, inertia @ w))


def quat_to_yaw_pitch_roll(qs_first):
    """MATLAB quat2angle (default 'ZYX') for a scalar-FIRST quaternion [q0 q1 q2 q3] -> (yaw, pitch, roll)."""
    q0, q1, q2, q3 = qs_first
    yaw = math.atan2(2.0 * (q1 * q2 + q0 * q3), q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3)
    s = -2.0 * (q1 * q3 - q0 * q2)
    pitch = math.asin(max(-1.0, min(1.0, s)))
    roll = math.atan2(2.0 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3)
    return yaw, pitch, roll


def angle_to_quat(yaw, pitch, roll):
    """MATLAB angle2quat (default 'ZYX') -> scalar-FIRST quaternion."""
    cy, sy = math.cos(yaw / 2), math.sin(yaw / 2)
    cp, sp = math.cos(pitch / 2), math.sin(pitch / 2)
    cr, sr = math.cos(roll / 2), math.sin(roll / 2)
    return np.array([cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr,
                     cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr])


def _ode45_step(rates, t0, t1, y0):
    """One [t0, t1] integration the way the reference calls ode45 inside its stage loop."""
    from scipy.integrate import solve_ivp
    sol = solve_ivp(rates, (t0, t1), np.asarray(y0, dtype=np.float64), method="RK45", rtol=1e-3, atol=1e-6)
    if not sol.success:
        raise RuntimeError("ode45 step failed: " + sol.message)
    return sol.y[:, -1]


# ---- Solver_attitude ---------------------------------------------------------------------------------------------------
DEFAULT_X0_ATTITUDE = np.array([0.0, 0.0, 0.0, 0.0501511024391496, 0.0833950587800888, -0.0818761044636256,
                                0.991880252153991])      # Solver_attitude.m:160-164


def spacecraft_dynamics_list(sa, X, U):
    """Solver_attitude.m:600-620: x_dot = f(X, u), diagonal inertia (J1, J2, J3)."""
    x1, x2, x3, x4, x5, x6, x7 = X
    u1, u2, u3 = U
    return np.array([(sa.J2 - sa.J3) / sa.J1 * x2 * x3 + u1 / sa.J1,
                     (sa.J3 - sa.J1) / sa.J2 * x3 * x1 + u2 / sa.J2,
                     (sa.J1 - sa.J2) / sa.J3 * x1 * x2 + u3 / sa.J3,
                     0.5 * (x3 * x5 - x2 * x6 + x1 * x7),
                     0.5 * (-x3 * x4 + x1 * x6 + x2 * x7),
                     0.5 * (x2 * x4 - x1 * x5 + x3 * x7),
                     0.5 * (-x1 * x4 - x2 * x5 - x3 * x6)])


def next_stage_states(sa, X1, U, h, mode="RK4"):
    """Solver_attitude.m:670-696: one step of the 7-state dynamics, then renormalise the quaternion."""
    X1 = np.asarray(X1, dtype=np.float64)
    k1 = spacecraft_dynamics_list(sa, X1, U)
    if mode == "RK4":
        k2 = spacecraft_dynamics_list(sa, X1 + k1 * h / 2, U)
        k3 = spacecraft_dynamics_list(sa, X1 + k2 * h / 2, U)
        k4 = spacecraft_dynamics_list(sa, X1 + k3 * h, U)
        X2 = X1 + h * (k1 + 2 * k2 + 2 * k3 + k4) / 6
    elif mode == "taylor":
        X2 = X1 + h * k1
    else:
        raise ValueError("mode must be 'RK4' or 'taylor'")
    X2[3:7] /= math.sqrt(float(np.sum(X2[3:7] ** 2)))
    return X2


def linear_control_response(sa, X0=None, T_final=None, dt=None):
    """Solver_attitude.m:508-591: the PD reference controller U = -K qe(1:3) - C w (K = 0.2 I, C = I) rolled out with
    RK4 steps.  Returns (X [7, N+1], U [3, N], angles [3, N] = yaw, pitch, roll).  Many starts at once on the GPU:
    Solver_attitude.linear_control_responses (K21), whose X and U equal this loop's."""
    X0 = DEFAULT_X0_ATTITUDE if X0 is None else np.asarray(X0, dtype=np.float64)
    T_final = sa.T_final if T_final is None else T_final
    dt = sa.h if dt is None else dt
    N = int(round(T_final / dt))
    X = np.zeros((7, N + 1))
    U = np.zeros((3, N))
    ang = np.zeros((3, N))
    X[:, 0] = X0
    for k in range(N):
        q, w = X[3:7, k], X[0:3, k]
        U[:, k] = -0.2 * q[0:3] - w
        X[:, k + 1] = next_stage_states(sa, X[:, k], U[:, k], dt)
        ang[:, k] = quat_to_yaw_pitch_roll([X[6, k], X[5, k], X[4, k], X[3, k]])      # quat2angle([X7 X6 X5 X4])
    return X, U, ang


def attitude_optimal_path(sa, X0=None, method="nearest", n_steps=None):
    """Solver_attitude.m:744-833 after `run`: at every stage convert the quaternion to (yaw, pitch, roll), look the
    three torques up in the 6-D policy tables U{1,2,3}_Opt over (w1, w2, w3, yaw, pitch, roll), take one first-order
    ('taylor') step.  Returns (X [7, N], U [3, N], X_ANGLES [9, N])."""
    from .matlab_compat import interp_linear_point, interp_nearest_point
    if sa.U1_Opt is None or np.ndim(sa.U1_Opt) != 6:
        raise RuntimeError("run() first")
    X0 = DEFAULT_X0_ATTITUDE if X0 is None else np.asarray(X0, dtype=np.float64)
    N = sa.N_stage if n_steps is None else min(sa.N_stage, int(n_steps) + 1)
    knots = sa.grid_vectors_full()
    look = interp_nearest_point if method == "nearest" else interp_linear_point
    X = np.zeros((7, N))
    U = np.zeros((3, N))
    XA = np.zeros((9, N))
    X[:, 0] = X0
    for k in range(N - 1):
        yaw, pitch, roll = quat_to_yaw_pitch_roll([X[6, k], X[5, k], X[4, k], X[3, k]])
        p = (X[0, k], X[1, k], X[2, k], yaw, pitch, roll)
        U[:, k] = [float(look(knots, T, p)) for T in (sa.U1_Opt, sa.U2_Opt, sa.U3_Opt)]
        X[:, k + 1] = next_stage_states(sa, X[:, k], U[:, k], sa.h, "taylor")
        XA[:, k] = [X[0, k], X[1, k], X[2, k], math.degrees(roll), math.degrees(pitch), math.degrees(yaw), *U[:, k]]
    return X, U, XA


def attitude_optimal_path_simplified(sa, X0=None, n_steps=None):
    """Solver_attitude.m:835-925 after `simplified_run`: the three 2-D (w_i, theta_i) 'nearest' policies drive the FULL
    rigid body (full inertia matrix), integrated with ode45 over each stage.  Returns (T [N], X [N, 7], U [N, 3])."""
    if sa.U1_Opt is None or not callable(sa.U1_Opt):
        raise RuntimeError("simplified_run() first")
    X0 = DEFAULT_X0_ATTITUDE if X0 is None else np.asarray(X0, dtype=np.float64)
    N = sa.N_stage if n_steps is None else min(sa.N_stage, int(n_steps) + 1)
    X = np.zeros((N, 7))
    U = np.zeros((N, 3))
    X[0] = X0
    for k in range(N - 1):
        xs = X[k]
        u = np.array([float(sa.U1_Opt(xs[0], 2 * math.asin(xs[3]))), float(sa.U2_Opt(xs[1], 2 * math.asin(xs[4]))),
                      float(sa.U3_Opt(xs[2], 2 * math.asin(xs[5])))])
        U[k] = u

        def rates(t, y, u=u):
            return np.concatenate([rigid_body_rates_full(y[0:3], sa.InertiaM, u), quat_rates(y[3:7], y[0:3])])
        X[k + 1] = _ode45_step(rates, k * sa.h, (k + 1) * sa.h, xs)
    return np.arange(N) * sa.h, X, U


# ---- Solver_pos_att ----------------------------------------------------------------------------------------------------
def target_R0V0():
    """Solver_pos_att.m:734-753: the target's initial state (perigee altitude 300 km, e = 0.1, equatorial, at perigee)."""
    rp, e = R_EARTH + 300.0, 0.1
    ra = rp * (1.0 + e) / (1.0 - e)
    h_ = math.sqrt(2.0 * MU_EARTH * rp * ra / (ra + rp))
    return state_from_elements(h_, e, 0.0, 0.0, 0.0, 0.0, MU_EARTH)


def RSW2ECI(pos, vel):
    """Solver_pos_att.m:831-847: columns R, S, W."""
    pos, vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    R = pos / np.linalg.norm(pos)
    c = np.cross(pos, vel)
    W = c / np.linalg.norm(c)
    S = np.cross(W, R)
    return np.column_stack([R, S, W])


def _orbit_scalars(R, V, mu):
    """What the relative-motion right-hand side (:695-715) needs of the target's state: [2mu/|R|^3 + H^2/|R|^4, 2 (R.V) H/|R|^4,
    2H/|R|^2, mu/|R|^3 - H^2/|R|^4, mu/|R|^3] with H = |R x V|."""
    nR = math.sqrt(float(R @ R))
    RdV = float(R @ V)
    H = float(np.linalg.norm(np.cross(R, V)))
    return [2 * mu / nR ** 3 + H * H / nR ** 4, 2 * RdV / nR ** 4 * H, 2 * H / nR ** 2, mu / nR ** 3 - H * H / nR ** 4, mu / nR ** 3]


def ECI2body(q):
    """Solver_pos_att.m:825-829 (scalar-last quaternion)."""
    q1, q2, q3, q4 = q
    return np.array([[1 - 2 * (q2 * q2 + q3 * q3), 2 * (q1 * q2 + q3 * q4), 2 * (q1 * q3 - q2 * q4)],
                     [2 * (q2 * q1 - q3 * q4), 1 - 2 * (q1 * q1 + q3 * q3), 2 * (q2 * q3 + q1 * q4)],
                     [2 * (q3 * q1 + q2 * q4), 2 * (q3 * q2 - q1 * q4), 1 - 2 * (q1 * q1 + q2 * q2)]])


def to_Moments_Forces(pa, f, R0, V0, q):
    """Solver_pos_att.m:804-823: thruster levels f[0..11] -> body moments U_M [x, y, z] and the acceleration in the RSW
    frame (body-frame thrust sums rotated back through ECI2body and RSW2ECI)."""
    f = np.asarray(f, dtype=np.float64)
    U_M = np.array([(f[4] - f[5] + f[10] - f[11]) * pa.T_dist,       # x
                    (f[0] - f[1] + f[6] - f[7]) * pa.T_dist,         # y
                    (f[2] - f[3] + f[8] - f[9]) * pa.T_dist])        # z
    a_body = np.array([f[0] + f[1] + f[6] + f[7], f[2] + f[3] + f[8] + f[9], f[4] + f[5] + f[10] + f[11]]) / pa.Mass
    acc = np.linalg.solve(RSW2ECI(R0, V0), np.linalg.solve(ECI2body(q), a_body))
    return U_M, acc


def thruster_policies(pa):
    """set_controller (:849-884) for the three channels from the controllers simplified_run left in memory:
    12 'nearest' policies over (x, v, theta, w), indexed by thruster number."""
    from .solver_position import NearestPolicy
    names = {"x": (0, 1, 6, 7), "y": (2, 3, 8, 9), "z": (4, 5, 10, 11)}
    pol = [None] * 12
    for ch, thr in names.items():
        c = pa.controllers["channel_%s_controller_1" % ch]
        idx = np.asarray(c["U_Optimal_id"], dtype=np.int64) - 1
        for key, t in zip(("f0_allcomb", "f1_allcomb", "f6_allcomb", "f7_allcomb"), thr):
            pol[t] = NearestPolicy(c["GridVectors"], np.asarray(c[key])[idx])
    return pol


def get_thruster_on_off_optimal(pol, x, v, t, w, R0, V0, q):
    """Solver_pos_att.m:404-449: rotate the relative position / velocity RSW -> ECI -> body, then per channel look up
    its four thrusters at (x_i, v_i, theta, w): channel x uses the angle / rate about y, y about z, z about x."""
    M = ECI2body(q) @ RSW2ECI(R0, V0)
    xb, vb = M @ np.asarray(x, dtype=np.float64), M @ np.asarray(v, dtype=np.float64)
    f = np.zeros(12)
    for (thr, i, ax) in (((0, 1, 6, 7), 0, 1), ((2, 3, 8, 9), 1, 2), ((4, 5, 10, 11), 2, 0)):
        for tn in thr:
            f[tn] = float(pol[tn](xb[i], vb[i], t[ax], w[ax]))
    return f


def pos_att_optimal_path(pa, X0=None, n_steps=None):
    """Solver_pos_att.m:452-730 without the plots: 13-state closed loop.  Per stage: thruster levels from the policies,
    forces / moments held over the stage, ode45 of the relative-motion equations about the Kepler-propagated target
    plus the rigid body with the full inertia matrix.  Returns (T [N], X [N, 13], F_Th_Opt [N, 12], Force_Moment [N, 6])."""
    if not pa.controllers:
        raise RuntimeError("simplified_run() first")
    if X0 is None:
        X0 = pos_att_default_X0()                                                              # :457-466
    pol = thruster_policies(pa)
    N = pa.N_stage if n_steps is None else min(pa.N_stage, int(n_steps) + 1)
    X = np.zeros((N, 13))
    F = np.zeros((N, 12))
    FM = np.zeros((N, 6))
    X[0] = X0
    R0, V0 = target_R0V0()
    mu = MU_EARTH
    for k in range(N - 1):
        xs = X[k]
        t_stage = 2.0 * np.arcsin(xs[6:9])
        f = get_thruster_on_off_optimal(pol, xs[0:3], xs[3:6], t_stage, xs[10:13], R0, V0, xs[6:10])
        U_M, acc = to_Moments_Forces(pa, f, R0, V0, xs[6:10])
        F[k] = f
        FM[k] = np.concatenate([acc, U_M])

        def rates(t, y, acc=acc, U_M=U_M):
            c0, c1, c2, c3, c4 = _orbit_scalars(*propagate_kepler(R0, V0, t, mu), mu)
            x1, x2, x3, v1, v2, v3 = y[0:6]
            return np.concatenate([
                [v1, v2, v3,
                 c0 * x1 - c1 * x2 + c2 * v2 + acc[0],
                 -c3 * x2 + c1 * x1 - c2 * v1 + acc[1],
                 -c4 * x3 + acc[2]],
                quat_rates(y[6:10], y[10:13]),
                rigid_body_rates_full(y[10:13], pa.InertiaM, U_M)])
        X[k + 1] = _ode45_step(rates, k * pa.h, (k + 1) * pa.h, xs)
    return np.arange(N) * pa.h, X, F, FM


# ---- Solver_pos_att, fixed step: the arithmetic of the GPU loop (K18, csrc/kernels_rollout_pos_att.h) -----------------
# At h = 0.005 s a classical RK4 step per stage and ode45 both sit at round-off (tests/test_rollout_pos_att_abi.py holds the
# two loops together to 1e-12 over the whole horizon), so this is the reference's simulator in a form that can be batched
# and pinned: every operation below is one IEEE double operation in the kernel's order.
def pos_att_default_X0():
    """Solver_pos_att.m:457-466."""
    q0 = angle_to_quat(math.radians(0.0), math.radians(3.0), math.radians(0.0))[::-1]
    return np.concatenate([[-0.1, 0.0, 0.0], [0.0, 0.0, 0.0], q0, [0.0, 0.0, 0.0]])


def pos_att_orbit_table(n_steps, h, substeps=1, R0=None, V0=None, mu=MU_EARTH):
    """What the pos-att right-hand side (:695-715) needs of the target's orbit, at the times a fixed-step integrator asks:
    node j = 0 .. 2 * substeps * n_steps at t_j = j * h / (2 * substeps).  Returns (rsw2eci [3, 3] = RSW2ECI(R0, V0),
    coef [n_nodes, 5]) with coef[j] = [2mu/|R|^3 + H^2/|R|^4, 2 (R.V) H/|R|^4, 2H/|R|^2, mu/|R|^3 - H^2/|R|^4, mu/|R|^3]
    from propagate_kepler(R0, V0, t_j).  R0, V0 None: the reference's target (:734-753)."""
    if R0 is None or V0 is None:
        R0, V0 = target_R0V0()
    S = int(substeps)
    if S < 1 or int(n_steps) < 0:
        raise ValueError("pos_att_orbit_table needs substeps >= 1 and n_steps >= 0")
    n_nodes = 2 * S * int(n_steps) + 1
    coef = np.empty((n_nodes, 5))
    for j in range(n_nodes):
        coef[j] = _orbit_scalars(*propagate_kepler(R0, V0, j * h / (2 * S), mu), mu)
    return RSW2ECI(R0, V0), coef


def canon_asin(x):
    """The library's asin (csrc/kernels_rollout_attitude.h canon_asin): fdlibm's e_asin.c in + - * /, sqrt, comparisons and
    selects, |x| <= 1; within 2 ulp of libm."""
    x = float(x)
    ax = abs(x)

    def pq(t):
        p = t * (1.66666666666666657415e-01 + t * (-3.25565818622400915405e-01 + t * (2.01212532134862925881e-01 +
                 t * (-4.00555345006794114027e-02 + t * (7.91534994289814532176e-04 + t * 3.47933107596021167570e-05)))))
        q = 1.0 + t * (-2.40339491173441421878e+00 + t * (2.02094576023350569471e+00 + t * (-6.88283971605453293030e-01 +
                       t * 7.70381505559019352791e-02)))
        return p, q
    if ax < 0.5:
        p, q = pq(ax * ax)
        v = ax + ax * (p / q)
    else:
        t = (1.0 - ax) * 0.5
        p, q = pq(t)
        s = math.sqrt(t) if t >= 0.0 else math.nan
        if ax >= 0.975:
            v = 1.57079632679489655800e+00 - (2.0 * (s + s * (p / q)) - 6.12323399573676603587e-17)
        else:
            cs = s * 134217729.0
            sh = cs - (cs - s)
            c = (t - sh * sh) / (s + sh)
            pp = 2.0 * s * (p / q) - (6.12323399573676603587e-17 - 2.0 * c)
            qq = 7.85398163397448278999e-01 - 2.0 * sh
            v = 7.85398163397448278999e-01 - (pp - qq)
    return -v if math.copysign(1.0, x) < 0 else v


def inv3_adjugate(m):
    """3 x 3 inverse as the adjugate over the determinant, in the library's operation order (pa_inv3)."""
    m = [float(v) for v in np.asarray(m, dtype=np.float64).reshape(9)]
    c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4]
    c10, c11, c12 = m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5]
    c20, c21, c22 = m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]
    det = (m[0] * c00 + m[1] * c10) + m[2] * c20
    with np.errstate(all="ignore"):
        return (np.array([c00, c01, c02, c10, c11, c12, c20, c21, c22]) / np.float64(det)).reshape(3, 3)


def _mul3(m, v0, v1, v2):
    return [(m[r][0] * v0 + m[r][1] * v1) + m[r][2] * v2 for r in range(3)]


def _eci2body_list(q1, q2, q3, q4):
    return [[1.0 - 2.0 * (q2 * q2 + q3 * q3), 2.0 * (q1 * q2 + q3 * q4), 2.0 * (q1 * q3 - q2 * q4)],
            [2.0 * (q2 * q1 - q3 * q4), 1.0 - 2.0 * (q1 * q1 + q3 * q3), 2.0 * (q2 * q3 + q1 * q4)],
            [2.0 * (q3 * q1 + q2 * q4), 2.0 * (q3 * q2 - q1 * q4), 1.0 - 2.0 * (q1 * q1 + q2 * q2)]]


def _nearest_index(k, x):
    """Index of the knot nearest to x: the cell by bisection, clamped to the grid (NaN: cell 0), then the upper knot when
    x - k[cell] >= k[cell + 1] - x (the library's find_cell and 'nearest' rule)."""
    lo, hi = 0, len(k) - 1
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if k[mid] <= x:
            lo = mid
        else:
            hi = mid
    return lo + 1 if (x - k[lo]) >= (k[lo + 1] - x) else lo


def pos_att_channels(pa, channel_x="channel_x_controller_1"):
    """The three channel policies simplified_run left, as the GPU loop takes them: per channel (knots [4], labels as stored
    (1-based, [n_x, n_v, n_t, n_w]), thruster table [n_comb, 4] = [f0 f1 f6 f7]_allcomb)."""
    if not pa.controllers:
        raise RuntimeError("simplified_run() first")
    out = []
    for name in (channel_x, "channel_y_controller_1", "channel_z_controller_1"):
        c = pa.controllers[name]
        knots = [np.ascontiguousarray(g, dtype=np.float64) for g in c["GridVectors"]]
        table = np.stack([np.asarray(c[key], dtype=np.float64) for key in ("f0_allcomb", "f1_allcomb", "f6_allcomb", "f7_allcomb")], axis=1)
        out.append((knots, np.asarray(c["U_Optimal_id"]), table))
    return out


def _stage_angles(x, first):
    """theta_j = 2 canon_asin(clamp(x[first + j], -1, 1)), j = 0..2: the angles a stage looks its policies up at."""
    return [2.0 * canon_asin(1.0 if x[first + j] > 1.0 else -1.0 if x[first + j] < -1.0 else x[first + j]) for j in range(3)]


def _rk4_step(rates, x, hs, c_first, c_mid, c_last):
    """One classical RK4 step of size hs in the kernels' operation order (HJB_ROLLOUT_RK4_STEP); rates(c, y) gets c_first at the
    start of the step, c_mid at both midpoints and c_last at its end."""
    n = range(len(x))
    r = rates(c_first, x)
    acc = r
    xt = [x[i] + (r[i] * hs) / 2.0 for i in n]
    r = rates(c_mid, xt)
    acc = [acc[i] + 2.0 * r[i] for i in n]
    xt = [x[i] + (r[i] * hs) / 2.0 for i in n]
    r = rates(c_mid, xt)
    acc = [acc[i] + 2.0 * r[i] for i in n]
    xt = [x[i] + r[i] * hs for i in n]
    r = rates(c_last, xt)
    return [x[i] + (hs * (acc[i] + r[i])) / 6.0 for i in n]


def _pos_att_rates(Jm, Ji, a, um, c, y):
    """The 13-state right-hand side (:695-715) with the five orbit scalars c, the RSW acceleration a and the body moments um held."""
    c0, c1, c2, c3, c4 = c
    q1, q2, q3, q4, w1, w2, w3 = y[6:13]
    jw = _mul3(Jm, w1, w2, w3)
    t = [um[0] - (w2 * jw[2] - w3 * jw[1]), um[1] - (w3 * jw[0] - w1 * jw[2]), um[2] - (w1 * jw[1] - w2 * jw[0])]
    return [y[3], y[4], y[5],
            ((c0 * y[0] - c1 * y[1]) + c2 * y[4]) + a[0],
            ((c1 * y[0] - c3 * y[1]) - c2 * y[3]) + a[1],
            a[2] - c4 * y[2],
            0.5 * (((w3 * q2) - (w2 * q3)) + (w1 * q4)),
            0.5 * (((w1 * q3) - (w3 * q1)) + (w2 * q4)),
            0.5 * (((w2 * q1) - (w1 * q2)) + (w3 * q4)),
            0.5 * (((-(w1 * q1)) - (w2 * q2)) - (w3 * q3))] + _mul3(Ji, t[0], t[1], t[2])


def _pos_att_stages(pa, chans, X0, N, substeps, mask, f_at, s_at, pos_tol, att_tol):
    """The stage loop of pos_att_optimal_path_fixed and pos_att_fault_path_fixed, in the operation order of K18 / K23: chans the
    channels x, y, z and, when s_at < N - 1, the failure controller of channel x; from stage f_at on the thrusters of mask apply
    +0.0, from stage s_at on channel x is looked up in chans[3].  Returns pos_att_fault_path_fixed's six results."""
    S = int(substeps)
    rsw, coef = pos_att_orbit_table(N - 1, pa.h, S)
    rsw = [[float(v) for v in row] for row in rsw]
    rswi = [[float(v) for v in row] for row in inv3_adjugate(rsw)]
    Jm = [[float(v) for v in row] for row in np.asarray(pa.InertiaM, dtype=np.float64)]
    Ji = [[float(v) for v in row] for row in inv3_adjugate(Jm)]
    mass, d, hs = float(pa.Mass), float(pa.T_dist), float(pa.h) / S
    p2, a2 = float(pos_tol) * float(pos_tol), float(att_tol) * float(att_tol)
    coef = coef.tolist()
    kn = [[k.tolist() for k in ch[0]] for ch in chans]
    lab = [np.asarray(ch[1]) for ch in chans]
    tab = [ch[2].tolist() for ch in chans]
    slots = ((0, 1, 6, 7), (2, 3, 8, 9), (4, 5, 10, 11))
    axis = (1, 2, 0)                                   # channel x uses the angle / rate about y, y about z, z about x

    def inside(y):
        return ((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]) <= p2 and ((y[6] * y[6] + y[7] * y[7]) + y[8] * y[8]) <= a2

    X = np.zeros((N, 13))
    F = np.zeros((N, 12))
    FM = np.zeros((N, 6))
    X[0] = X0
    x = [float(v) for v in X0]
    imp = 0.0
    last_outside = -1 if inside(x) else 0
    with np.errstate(all="ignore"):
        for k in range(N - 1):
            th = _stage_angles(x, 6)
            E = _eci2body_list(x[6], x[7], x[8], x[9])
            M = [[(E[r][0] * rsw[0][c] + E[r][1] * rsw[1][c]) + E[r][2] * rsw[2][c] for c in range(3)] for r in range(3)]
            xb, vb = _mul3(M, x[0], x[1], x[2]), _mul3(M, x[3], x[4], x[5])
            f = [0.0] * 12
            for ch in range(3):
                src = 3 if (ch == 0 and s_at <= k) else ch              # the failure controller has taken over channel x
                p = (xb[ch], vb[ch], th[axis[ch]], x[10 + axis[ch]])
                idx = tuple(_nearest_index(kn[src][a], p[a]) for a in range(4))
                row = tab[src][int(lab[src][idx]) - 1]
                for s_, v in zip(slots[ch], row):
                    f[s_] = v
            if f_at <= k:                                               # what the plant gets
                f = [0.0 if (mask >> j) & 1 else f[j] for j in range(12)]
            sk = abs(f[0]) + abs(f[1])
            for j in range(2, 12):
                sk = sk + abs(f[j])
            imp = imp + sk
            um = [(((f[4] - f[5]) + f[10]) - f[11]) * d, (((f[0] - f[1]) + f[6]) - f[7]) * d, (((f[2] - f[3]) + f[8]) - f[9]) * d]
            ab = [(((f[0] + f[1]) + f[6]) + f[7]) / mass, (((f[2] + f[3]) + f[8]) + f[9]) / mass, (((f[4] + f[5]) + f[10]) + f[11]) / mass]
            Ei = inv3_adjugate(E).tolist()
            ae = _mul3(Ei, ab[0], ab[1], ab[2])
            a = _mul3(rswi, ae[0], ae[1], ae[2])
            F[k] = f
            FM[k] = a + um

            def rates(c, y, a=a, um=um):
                return _pos_att_rates(Jm, Ji, a, um, c, y)
            for s in range(S):
                j = 2 * (S * k + s)
                x = _rk4_step(rates, x, hs, coef[j], coef[j + 1], coef[j + 2])
            X[k + 1] = x
            if not inside(x):
                last_outside = k + 1
    return np.arange(N) * pa.h, X, F, FM, imp * float(pa.h), last_outside + 1


def pos_att_optimal_path_fixed(pa, X0=None, n_steps=None, substeps=1, channel_x="channel_x_controller_1"):
    """pos_att_optimal_path with `substeps` classical RK4 steps of h / substeps per stage in place of ode45, forces and moments
    held over the stage: the scalar host loop in the operation order of the GPU kernel (K18), which it equals bit for bit.
    Returns what pos_att_optimal_path returns: (T [N], X [N, 13], F_Th_Opt [N, 12], Force_Moment [N, 6])."""
    chans = pos_att_channels(pa, channel_x)
    X0 = pos_att_default_X0() if X0 is None else np.asarray(X0, dtype=np.float64).reshape(13)
    N = pa.N_stage if n_steps is None else min(pa.N_stage, int(n_steps) + 1)
    return _pos_att_stages(pa, chans, X0, N, substeps, 0, 0, N - 1, math.inf, math.inf)[:4]


def pos_att_fault_path_fixed(pa, X0, fault_mask, fault_stage, switch_stage, n_steps=None, substeps=1, pos_tol=math.inf,
                             att_tol=math.inf):
    """pos_att_optimal_path_fixed with a thruster fault in the plant and a hand-over of channel x to channel_x_controller_1_failure
    (:235-240): the scalar host loop in the operation order of the GPU kernel (K23, csrc/kernels_rollout_pos_att_faults.h), which it
    equals bit for bit.  From stage fault_stage (None: 0) on, the thrusters whose bit is set in fault_mask (None or 0: no fault)
    apply +0.0 whatever was commanded; from stage switch_stage (None: never) on, channel x is looked up in the failure controller.
    Returns (T [N], X [N, 13], F_applied [N, 12], Force_Moment [N, 6], impulse, settle_stage): impulse = h * the sum over stages
    of ((|fa0| + |fa1|) + ...) + |fa11|; settle_stage the smallest s such that rows s .. N - 1 of X all have
    (x0^2 + x1^2) + x2^2 <= pos_tol^2 and (q1^2 + q2^2) + q3^2 <= att_tol^2, N when the last row has not.  With no fault and no
    hand-over the four arrays are pos_att_optimal_path_fixed's (one stage loop, _pos_att_stages, serves both)."""
    chans = pos_att_channels(pa)
    mask = 0 if fault_mask is None else int(fault_mask)
    f_at = 0 if fault_stage is None else int(fault_stage)
    X0 = pos_att_default_X0() if X0 is None else np.asarray(X0, dtype=np.float64).reshape(13)
    N = pa.N_stage if n_steps is None else min(pa.N_stage, int(n_steps) + 1)
    s_at = N - 1 if switch_stage is None else int(switch_stage)
    if mask < 0 or mask >> 12 or f_at < 0 or s_at < 0:
        raise ValueError("fault_mask has twelve bits and the stages are >= 0")
    if s_at < N - 1:
        chans = chans + pos_att_channels(pa, "channel_x_controller_1_failure")[:1]
    return _pos_att_stages(pa, chans, X0, N, substeps, mask, f_at, s_at, pos_tol, att_tol)


# ---- Solver_attitude, simplified policies on the rigid body: the arithmetic of the GPU loop (K20, --------------------------------
# csrc/kernels_rollout_attitude_simplified.h) ---------------------------------------------------------------------------------------
def attitude_simplified_channels(sa, per_stage=False):
    """The three channel policies simplified_run left, as the GPU loop takes them: per channel (knots [s_w, s_t], labels as stored
    (1-based; [n_w, n_t]: the stationary plane of sa.U_idx, or with per_stage [n_w, n_t, n_stages] from sa.U_idx_stages, which
    simplified_run(keep_policy=True) leaves: step k reads plane k as attitude-control/test/test_simplified.m:137-139 indexes
    U_Opt(:,:,k_stage)), torque table [n_u, 1] = U_vector)."""
    if getattr(sa, "U_idx", None) is None or sa.U1_Opt is None or not callable(sa.U1_Opt) or any(i is None for i in sa.U_idx):
        raise RuntimeError("simplified_run() first")
    if per_stage and getattr(sa, "U_idx_stages", None) is None:
        raise RuntimeError("simplified_run() first (keep_policy=True for per_stage)")
    ut = np.asarray(sa.U_vector, dtype=np.float64).reshape(-1, 1)
    src = sa.U_idx_stages if per_stage else sa.U_idx
    return [([np.ascontiguousarray(g, dtype=np.float64) for g in getattr(sa, "U%d_Opt" % (ch + 1)).GridVectors], np.asarray(src[ch]), ut)
            for ch in range(3)]


def attitude_optimal_path_simplified_fixed(sa, X0=None, n_steps=None, substeps=1, dynamics="full", per_stage=False):
    """attitude_optimal_path_simplified with the stage integrator fixed: the scalar host loop in the operation order of the GPU
    kernel (K20), which it equals bit for bit.  Per stage theta_i = 2 canon_asin(clamp(X[3+i], -1, 1)), the three 'nearest'
    torques at (w_i, theta_i), the stage cost (Q_i w_i^2 + Qt_i theta_i^2) + R_i u_i^2 of the 2-D sweeps, then
      dynamics 'full' (Solver_attitude.m:835-925): `substeps` classical RK4 steps of h / substeps of the full-inertia rigid body
        in place of ode45, quaternion not renormalised.  NOT round-off: the gap to the ode45 loop is RK4's truncation error
        against Dormand-Prince's 5th-order solution, measured on the default grids with a switching policy as max |dX| = 4.9e-13
        over 5,999 stages (2.1e-12 over 2,000 stages from a fast tumbling start) with substeps = 1 and 1.4e-14 (1.4e-13) with
        substeps = 2, every torque equal (tests/test_rollout_attitude_simplified_abi.py);
      dynamics 'diagonal' (test/test_simplified.m:188-218): next_stage_states(., 'RK4') - diagonal inertia, one RK4 step,
        q / |q| - the reference's own arithmetic; substeps must be 1.
    per_stage: step k reads plane k of sa.U_idx_stages (simplified_run(keep_policy=True)).
    Returns (T [N], X [N, 7], U [N, 3], TH [N, 3] (the theta_i looked up at), cost); the last U / TH row is zero."""
    chans = attitude_simplified_channels(sa, per_stage)
    if dynamics not in ("full", "diagonal"):
        raise ValueError("dynamics must be 'full' or 'diagonal'")
    S = int(substeps)
    if S < 1 or (dynamics == "diagonal" and S != 1):
        raise ValueError("substeps must be >= 1, and 1 with dynamics='diagonal'")
    X0 = DEFAULT_X0_ATTITUDE if X0 is None else np.asarray(X0, dtype=np.float64).reshape(7)
    N = sa.N_stage if n_steps is None else min(sa.N_stage, int(n_steps) + 1)
    if per_stage and N - 1 > chans[0][1].shape[2]:
        raise ValueError("%d steps, the stored policy has %d stages" % (N - 1, chans[0][1].shape[2]))
    kn = [[k.tolist() for k in ch[0]] for ch in chans]
    lab = [ch[1] for ch in chans]
    tab = [ch[2][:, 0].tolist() for ch in chans]
    Jm = [[float(v) for v in row] for row in np.asarray(sa.InertiaM, dtype=np.float64)]
    Ji = [[float(v) for v in row] for row in inv3_adjugate(Jm)]
    J1, J2, J3 = Jm[0][0], Jm[1][1], Jm[2][2]
    c1, c2, c3 = (J2 - J3) / J1, (J3 - J1) / J2, (J1 - J2) / J3
    qw = [float(sa.Q1), float(sa.Q2), float(sa.Q3)]
    qt = [float(sa.Qt1), float(sa.Qt2), float(sa.Qt3)]
    rr = [float(sa.R1), float(sa.R2), float(sa.R3)]
    h = float(sa.h)
    hs = h / S

    def full(u, y):
        w1, w2, w3, q1, q2, q3, q4 = y
        jw = _mul3(Jm, w1, w2, w3)
        t = [u[0] - (w2 * jw[2] - w3 * jw[1]), u[1] - (w3 * jw[0] - w1 * jw[2]), u[2] - (w1 * jw[1] - w2 * jw[0])]
        return _mul3(Ji, t[0], t[1], t[2]) + [0.5 * (((w3 * q2) - (w2 * q3)) + (w1 * q4)),
                                              0.5 * (((w1 * q3) - (w3 * q1)) + (w2 * q4)),
                                              0.5 * (((w2 * q1) - (w1 * q2)) + (w3 * q4)),
                                              0.5 * (((-(w1 * q1)) - (w2 * q2)) - (w3 * q3))]

    def diag(u, y):
        x1, x2, x3, x4, x5, x6, x7 = y
        return [((c1 * x2) * x3) + u[0] / J1, ((c2 * x3) * x1) + u[1] / J2, ((c3 * x1) * x2) + u[2] / J3,
                0.5 * (((x3 * x5) - (x2 * x6)) + (x1 * x7)), 0.5 * (((-x3 * x4) + (x1 * x6)) + (x2 * x7)),
                0.5 * (((x2 * x4) - (x1 * x5)) + (x3 * x7)), 0.5 * (((-x1 * x4) - (x2 * x5)) - (x3 * x6))]

    X = np.zeros((N, 7))
    U = np.zeros((N, 3))
    TH = np.zeros((N, 3))
    X[0] = X0
    x = [float(v) for v in X0]
    cost = 0.0
    with np.errstate(all="ignore"):
        for k in range(N - 1):
            th = _stage_angles(x, 3)
            u = []
            for ch in range(3):
                idx = (_nearest_index(kn[ch][0], x[ch]), _nearest_index(kn[ch][1], th[ch]))
                u.append(tab[ch][int(lab[ch][idx + (k,)] if per_stage else lab[ch][idx]) - 1])
            g = [(qw[j] * (x[j] * x[j]) + qt[j] * (th[j] * th[j])) + rr[j] * (u[j] * u[j]) for j in range(3)]
            cost = cost + ((g[0] + g[1]) + g[2])
            U[k] = u
            TH[k] = th
            if dynamics == "full":
                for _ in range(S):
                    x = _rk4_step(full, x, hs, u, u, u)
            else:
                x = _rk4_step(diag, x, h, u, u, u)
                nrm = np.float64(math.sqrt(((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) + x[6] * x[6]))
                x = x[:3] + [float(np.float64(v) / nrm) for v in x[3:]]       # numpy's division: 0 / 0 is NaN, not an exception
            X[k + 1] = x
    return np.arange(N) * sa.h, X, U, TH, cost


# ---- Solver_position, RKF45 on its schedule: the arithmetic of the GPU loop (K19, csrc/kernels_rollout_position.h) ------------
# Solver_position.get_optimal_path integrates each stage with orbit.rkf45.  At h = 0.005 s its error tests pass with a ratio
# allowed / (err + eps) of some 1e7 where fourfold growth needs 4^5 = 1024, so every step is accepted and grows fourfold: the
# steps of a stage follow from its t0 and tf alone (position_rkf45_schedule).  A classical RK4 stage does NOT reproduce the loop:
# rkf45 clips an accepted step to the end of the interval after forming its stage derivatives with the unclipped step, so a
# stage's last sub-step is no consistent Runge-Kutta step, and the loop below keeps that.  Every operation is one IEEE double
# operation in the kernel's order; a sub-step whose error test does not leave rkf45 its fourfold growth is flagged.
POSITION_MAX_SUB = 8                  # sub-steps per stage the table may hold (csrc HJB_POS_MAX_SUB)
POSITION_GROWTH_MARGIN = 1100.0       # > 4^5 = 1024: room for the rounding of rkf45's pow(., 0.2)


def position_rkf45_schedule(t0, tf):
    """The steps orbit.rkf45 takes from t0 to tf when every step is accepted and grows fourfold, in its own double arithmetic:
    [(t_i, h_form, h_apply)], h_form the step the six stage derivatives are formed with, h_apply = min(h_form, tf - t_i) the
    step that is applied."""
    t = float(t0)
    h = (tf - t0) / 100.0
    out = []
    while t < tf:
        ha = min(h, tf - t)
        out.append((t, h, ha))
        t = t + ha
        h = 4.0 * ha
    return out


def position_rkf45_table(n_steps, h, R0=None, V0=None, mu=MU_EARTH):
    """What K19 reads: (n_sub [n_steps] int32, table [n_steps, max_sub, 32]).  Stage k runs from k*h to (k+1)*h on
    position_rkf45_schedule; row (k, s) = [h_form, h_apply, then for each of Fehlberg's six times t_s + a_j*h_form the five orbit
    scalars of pos_att_orbit_table from propagate_kepler(R0, V0, t)]; rows beyond n_sub[k] are zero.  R0, V0 None: the
    reference's target.  More than POSITION_MAX_SUB sub-steps in a stage are refused."""
    from .orbit import _A
    if R0 is None or V0 is None:
        R0, V0 = target_R0V0()
    K = int(n_steps)
    if K < 0:
        raise ValueError("position_rkf45_table needs n_steps >= 0")
    sched = [position_rkf45_schedule(k * h, (k + 1) * h) for k in range(K)]
    n_sub = np.array([len(s) for s in sched], dtype=np.int32)
    if K and (n_sub.max() > POSITION_MAX_SUB or n_sub.min() < 1):
        k = int(np.argmax((n_sub > POSITION_MAX_SUB) | (n_sub < 1)))
        raise ValueError("stage %d takes %d sub-steps (1..%d supported)" % (k, n_sub[k], POSITION_MAX_SUB))
    table = np.zeros((K, int(n_sub.max()) if K else 1, 32))
    for k, steps in enumerate(sched):
        for s, (t, hf, ha) in enumerate(steps):
            row = table[k, s]
            row[0], row[1] = hf, ha
            for j in range(6):
                row[2 + 5 * j:7 + 5 * j] = _orbit_scalars(*propagate_kepler(R0, V0, t + _A[j] * hf, mu), mu)
    return n_sub, table


def position_channels(sp):
    """The three channel policies simplified_run left, as the GPU loop takes them: per channel (knots [s_x, s_v], labels as
    stored (1-based, [n_x, n_v]), acceleration table [n_u, 1] = U_vector; get_optimal_path takes the policy's value as the
    acceleration, :215-222)."""
    if sp.U_idx[0] is None:
        raise RuntimeError("simplified_run() first")
    ut = np.asarray(sp.U_vector, dtype=np.float64).reshape(-1, 1)
    return [([np.ascontiguousarray(g, dtype=np.float64) for g in getattr(sp, "U%d_Opt" % (ch + 1)).GridVectors], np.asarray(sp.U_idx[ch]), ut)
            for ch in range(3)]


def _absmax(m, v):
    """max(m, |v|) that keeps a NaN once met, as numpy's max does"""
    v = abs(v)
    return v if (v > m or v != v) else m


def position_optimal_path_fixed(sp, y0=None, n_steps=None, tol=1e-8, table=None):
    """Solver_position.get_optimal_path with every stage's rkf45 call replaced by its schedule (position_rkf45_table): the scalar
    host loop in the operation order of the GPU kernel (K19), which it equals bit for bit.  Returns what get_optimal_path
    returns plus off_schedule: (T [N], X [6, N], F_Opt_history [3, N], off_schedule), off_schedule the first stage with a
    sub-step where allowed >= 1100 * (te_max + eps) does not hold (rkf45 might not have grown its step fourfold there, or NaN),
    -1 if none; the loop goes on along the schedule either way.  table: (n_sub, table) of position_rkf45_table for at least the
    stages asked for, to spare building it once per start; None builds it."""
    from .orbit import _B, _C4, _C5
    chans = position_channels(sp)
    y = [-1.0, 0.0, 0.0, 0.0, 0.0, 0.0] if y0 is None else [float(v) for v in np.asarray(y0, dtype=np.float64).reshape(6)]
    N = int(math.ceil(sp.T_final / sp.h))
    if n_steps is not None:
        N = min(N, int(n_steps) + 1)
    R0, V0 = sp.get_target_R0V0()
    n_sub, table = position_rkf45_table(N - 1, sp.h, R0, V0) if table is None else table
    if len(n_sub) < N - 1:
        raise ValueError("the table holds %d stages, %d asked for" % (len(n_sub), N - 1))
    table = np.asarray(table)[:N - 1].tolist()
    kn = [[k.tolist() for k in ch[0]] for ch in chans]
    lab = [ch[1] for ch in chans]
    ut = [ch[2][:, 0].tolist() for ch in chans]
    eps = float(np.finfo(np.float64).eps)
    tol = float(tol)
    d = [float(v) for v in (_C4 - _C5)]
    c5 = [float(v) for v in _C5]
    used = (0, 2, 3, 4, 5)                            # d_1 = C5_1 = 0: no term

    def rates(c, a, y):
        c0, c1, c2, c3, c4 = c
        return [y[3], y[4], y[5],
                ((c0 * y[0] - c1 * y[1]) + c2 * y[4]) + a[0],
                ((c1 * y[0] - c3 * y[1]) - c2 * y[3]) + a[1],
                a[2] - c4 * y[2]]

    X = np.zeros((6, N))
    F = np.zeros((3, N))
    X[:, 0] = y
    off = -1
    for k in range(N - 1):
        a = [ut[ch][int(lab[ch][_nearest_index(kn[ch][0], y[ch]), _nearest_index(kn[ch][1], y[3 + ch])]) - 1] for ch in range(3)]
        F[:, k] = a
        on = True
        for s in range(int(n_sub[k])):
            row = table[k][s]
            hf, ha = row[0], row[1]
            f = [rates(row[2:7], a, y)]
            for st in range(1, 6):
                yin = list(y)
                for j in range(st):
                    hb = hf * _B[st][j]
                    yin = [yin[i] + hb * f[j][i] for i in range(6)]
                f.append(rates(row[2 + 5 * st:7 + 5 * st], a, yin))
            te, ym = 0.0, 1.0
            for i in range(6):
                e = f[0][i] * d[0]
                for j in used[1:]:
                    e = e + f[j][i] * d[j]
                te = _absmax(te, hf * e)
                ym = _absmax(ym, y[i])
            if not (tol * ym >= POSITION_GROWTH_MARGIN * (te + eps)):
                on = False
            yn = []
            for i in range(6):
                s5 = f[0][i] * c5[0]
                for j in used[1:]:
                    s5 = s5 + f[j][i] * c5[j]
                yn.append(y[i] + ha * s5)
            y = yn
        if not on and off < 0:
            off = k
        X[:, k + 1] = y
    return np.arange(N) * sp.h, X, F, off
