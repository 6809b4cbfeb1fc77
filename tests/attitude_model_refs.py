"""References for HJB_MODEL_QUAT_EULER321 (include/hjbdp.h; model_quat_next in csrc/kernels_packed2.h and oracle/hjb_oracle.c), numpy
only: a float32 restatement of the model up to the arguments of its three function calls, a classifier of those arguments by the
branches of canon_atan2f / canon_asinf, the same kinematics in float64, and problems whose tables drive every branch.

The model, per state (i0, i1, i2 | i3, i4, i5) = (yaw, pitch, roll | w1, w2, w3): q = tables[.][i0, i1, i2], w = the rate knots,
    x = q + h (0.5 (Omega(w) q)),  x /= |x|,
    yaw' = atan2(2 (x6 x5 + x7 x4), ((x7^2 + x6^2) - x5^2) - x4^2),  pitch' = asin(clamp(-2 (x6 x4 - x7 x5), -1, 1)),
    roll' = atan2(2 (x5 x4 + x7 x6), ((x7^2 - x6^2) - x5^2) + x4^2)
in single precision, every operation rounded (attitude-control/Solver_attitude.m:449-489)."""
import numpy as np

from hjbdp.problem import ProblemSpec, Term

f32 = np.float32
TAN_PI_8 = f32(0.4142135623730950)            # canon_atan2f's reduction threshold, as the compiler rounds the literal
HALF_PI = f32(1.57079632679489662)
PI = f32(3.14159265358979324)
CLASS_FLOOR = 20                              # states every class must hold (tests/test_attitude_model_refs.py)

ATAN2_CLASSES = ("swap", "no_swap", "ay_eq_ax", "r_above", "r_not_above", "x_neg", "x_zero", "y_neg", "y_pos_zero", "y_neg_zero",
                 "den_zero")
# x = -0 cannot come out of the model: x is ((a - b) - c) -+ d of squares, each +0 or positive, a difference of equal numbers
# rounds to +0, and u - v is -0 only for u = -0, v = +0 - so no partial result is -0.  classify_atan2 counts it all the same
# ("x_neg_zero", outside ATAN2_CLASSES) and assert_classes holds it at zero; canon_atan2f itself is driven there directly
# (tests/test_attitude_model_refs.py).  y = 2 (u + v) is -0 whenever both products are.
ASIN_CLASSES = ("a_above_half", "a_not_above_half", "a_eq_one", "s_above_one", "s_below_minus_one")


def model_inputs(spec):
    """(tables [4] float32 over (n0, n1, n2), rate knots [3] float32, h float32) as the library and the twin read them."""
    tabs = [np.asarray(t, dtype=f32) for t in spec.model["tables"]]
    rates = [np.asarray(spec.knots[a]).astype(f32) for a in (3, 4, 5)]
    return tabs, rates, f32(spec.model["h"])


def _on_grid(tabs, rates, dtype):
    q = [np.asarray(t, dtype=f32).astype(dtype)[:, :, :, None, None, None] for t in tabs]
    w1 = np.asarray(rates[0], dtype=f32).astype(dtype)[None, None, None, :, None, None]
    w2 = np.asarray(rates[1], dtype=f32).astype(dtype)[None, None, None, None, :, None]
    w3 = np.asarray(rates[2], dtype=f32).astype(dtype)[None, None, None, None, None, :]
    return q, w1, w2, w3


def _step(q, w1, w2, w3, h, half):
    """The Euler step and the renormalisation, in the dtype of the operands: one rounding per operation, in the model's order."""
    q1, q2, q3, q7 = q
    x4 = q1 + h * (half * ((w3 * q2 - w2 * q3) + w1 * q7))
    x5 = q2 + h * (half * ((-w3 * q1 + w1 * q3) + w2 * q7))
    x6 = q3 + h * (half * ((w2 * q1 - w1 * q2) + w3 * q7))
    x7 = q7 + h * (half * ((-w1 * q1 - w2 * q2) - w3 * q3))
    nrm = np.sqrt(((x4 * x4 + x5 * x5) + x6 * x6) + x7 * x7)
    return x4 / nrm, x5 / nrm, x6 / nrm, x7 / nrm


def _arguments(x4, x5, x6, x7, two):
    return {"yaw": (two * (x6 * x5 + x7 * x4), ((x7 * x7 + x6 * x6) - x5 * x5) - x4 * x4),
            "s": -two * (x6 * x4 - x7 * x5),
            "roll": (two * (x5 * x4 + x7 * x6), ((x7 * x7 - x6 * x6) - x5 * x5) + x4 * x4)}


def arguments_f32(tabs, rates, h):
    """The arguments model_quat_next hands to its three calls, float32 operation for operation, over the whole grid
    [n0, n1, n2, n3, n4, n5]: {"yaw": (y, x), "s": the asin argument BEFORE the clamp, "roll": (y, x)}."""
    q, w1, w2, w3 = _on_grid(tabs, rates, f32)
    with np.errstate(all="ignore"):
        out = _arguments(*_step(q, w1, w2, w3, f32(h), f32(0.5)), f32(2))
    assert all(a.dtype == f32 for v in out.values() for a in (v if isinstance(v, tuple) else (v,)))
    return out


def truth_f64(tabs, rates, h):
    """The same kinematics in float64 from the same float32 inputs -> (yaw', pitch', roll', s) over the whole grid."""
    q, w1, w2, w3 = _on_grid(tabs, rates, np.float64)
    a = _arguments(*_step(q, w1, w2, w3, np.float64(f32(h)), 0.5), 2.0)
    return (np.arctan2(a["yaw"][0], a["yaw"][1]), np.arcsin(np.clip(a["s"], -1.0, 1.0)), np.arctan2(a["roll"][0], a["roll"][1]), a["s"])


def classify_atan2(y, x):
    """States per branch class of canon_atan2f(y, x) (float32 arguments)."""
    y, x = np.asarray(y, dtype=f32), np.asarray(x, dtype=f32)
    ax, ay = np.abs(x), np.abs(y)
    swap = ay > ax
    num, den = np.where(swap, ax, ay), np.where(swap, ay, ax)
    with np.errstate(all="ignore"):
        r = np.where(den == 0, f32(0), num / den).astype(f32)
    c = {"swap": swap, "no_swap": ~swap, "ay_eq_ax": ay == ax, "r_above": r > TAN_PI_8, "r_not_above": ~(r > TAN_PI_8),
         "x_neg": x < 0, "x_zero": x == 0, "x_neg_zero": (x == 0) & np.signbit(x),
         "y_neg": y < 0, "y_pos_zero": (y == 0) & ~np.signbit(y), "y_neg_zero": (y == 0) & np.signbit(y), "den_zero": den == 0}
    return {k: int(np.count_nonzero(c[k])) for k in ATAN2_CLASSES + ("x_neg_zero",)}


def classify_asin(s):
    """States per branch class of the pitch call: a = |s| after the clamp on either side of 0.5 and at 1; |s| > 1 before it."""
    s = np.asarray(s, dtype=f32)
    a = np.minimum(np.abs(s), f32(1))
    c = {"a_above_half": a > f32(0.5), "a_not_above_half": ~(a > f32(0.5)), "a_eq_one": np.abs(s) == 1,
         "s_above_one": s > 1, "s_below_minus_one": s < -1}
    return {k: int(np.count_nonzero(c[k])) for k in ASIN_CLASSES}


def classify(tabs, rates, h):
    """{"yaw": atan2 classes, "roll": atan2 classes, "pitch": asin classes}: how many states of the grid take each branch."""
    a = arguments_f32(tabs, rates, h)
    return {"yaw": classify_atan2(*a["yaw"]), "roll": classify_atan2(*a["roll"]), "pitch": classify_asin(a["s"])}


def assert_classes(spec):
    """The input condition of every test on an edge problem: each branch class of each call holds >= CLASS_FLOOR states."""
    counts = classify(*model_inputs(spec))
    short = [(call, k, n) for call, cls in counts.items() for k, n in cls.items() if k != "x_neg_zero" and n < CLASS_FLOOR]
    assert not short, short
    assert counts["yaw"]["x_neg_zero"] == 0 and counts["roll"]["x_neg_zero"] == 0
    return counts


# ---- the edge problems -------------------------------------------------------------------------------------------------------
INERTIA = (0.02836 + 0.00016, 0.026817 + 0.00150, 0.023 + 0.00150)        # Solver_attitude.m:121-129, the diagonal
# form -> the launch form the library reports for it (option "packed2_mode"), the angle axes (yaw, pitch, roll), the rate knots,
# the torque levels (U1 outermost ... U3 innermost) and the step.  What decides the form (csrc/hjbdp_packed.hip's rules):
#   k15  (mode 8): U3 moves w3 by h dU / J3 = 0.0045 per level (< a cell of 0.15), eleven inner levels, >= 128 angle states;
#   k3w  (mode 6): the same three-plane window, five inner levels (K15 takes eleven or twelve);
#   k3   (mode 3): U3 moves w3 by 0.05 * 0.11 / 0.0245 = 0.22 per level, more than a cell of 0.2: the four-plane window.
FORMS = {
    "k15": dict(mode=8, n_ang=(8, 9, 9), h=0.005, m=(3, 3, 11),
                rates=([-0.3, 0.0, 0.3], [-0.3, -0.1, 0.0, 0.2], [-0.3, -0.15, 0.0, 0.15, 0.3])),
    "k3w": dict(mode=6, n_ang=(9, 9, 8), h=0.02, m=(3, 2, 5),
                rates=([-0.3, -0.1, 0.0, 0.2], [-0.25, 0.0, 0.3], [-0.3, -0.15, 0.0, 0.15, 0.3])),
    "k3": dict(mode=3, n_ang=(8, 9, 8), h=0.05, m=(2, 3, 3),
               rates=([-0.3, 0.0, 0.3], [-0.2, 0.0, 0.1, 0.3], [-0.4, -0.2, 0.0, 0.2, 0.4])),
}
_EDGE_VALUES = (0.0, -0.0, 1.0, -1.0, 0.5, -0.5, np.sqrt(0.5), -np.sqrt(0.5))
_EDGE_SCALES = (1.0, 0.9, 1.1, 1.0, 0.95, 1.05)


def edge_quaternions():
    """Every (q1, q2, q3, q7) with components from {+-0, +-1, +-1/2, +-1/sqrt2} (float32) whose norm lies in [0.9, 1.1]:
    [4, 368] - signed zeros in atan2's arguments, |y| == |x|, both arguments zero, pitch argument +-1 (K17's edge set, which
    tests/test_gpu_rollout_attitude.py builds the same way, without the all-zero quaternion and the far-from-unit ones)."""
    v = np.array(_EDGE_VALUES, dtype=f32)
    E = np.array(np.meshgrid(v, v, v, v, indexing="ij")).reshape(4, -1)
    nrm = np.sqrt((E.astype(np.float64) ** 2).sum(axis=0))
    return E[:, (nrm >= 0.9) & (nrm <= 1.1)]


def edge_tables(n_ang, n_edge=216):
    """(knots of yaw, pitch, roll [float32 values], tables [4] float32 over n_ang).  Yaw and roll span (-3.1, 3.1); pitch runs from
    -float32(pi/2) to +float32(pi/2) through 0; the quaternion of each grid point is formed in float64 with its TRUE scalar
    part (negative where yaw and roll are far apart) and rounded once.  Then `n_edge` consecutive entries (whole roll planes from
    plane 2 on) are overwritten with edge_quaternions(), evenly drawn, each scaled by one of _EDGE_SCALES: norm 0.9 ... 1.1."""
    n0, n1, n2 = n_ang
    assert n1 % 2 == 1
    yaw = np.linspace(-3.1, 3.1, n0).astype(f32)
    pitch = np.linspace(-1.0, 1.0, n1).astype(f32) * HALF_PI          # exact ends, exact 0
    roll = np.linspace(-3.05, 3.1, n2).astype(f32)
    assert pitch[0] == -HALF_PI and pitch[-1] == HALF_PI and pitch[n1 // 2] == 0
    Y, P, R = (a.astype(np.float64) / 2 for a in (yaw[:, None, None], pitch[None, :, None], roll[None, None, :]))
    c4, s4, c5, s5, c6, s6 = np.cos(Y), np.sin(Y), np.cos(P), np.sin(P), np.cos(R), np.sin(R)
    tabs = [s4 * c5 * c6 - c4 * s5 * s6, c4 * s5 * c6 + s4 * c5 * s6, c4 * c5 * s6 - s4 * s5 * c6, c4 * c5 * c6 + s4 * s5 * s6]
    tabs = [np.asfortranarray(t.astype(f32)) for t in tabs]
    E = edge_quaternions()
    pick = E[:, np.round(np.linspace(0, E.shape[1] - 1, n_edge)).astype(int)]
    pick = pick * np.resize(np.array(_EDGE_SCALES, dtype=f32), n_edge)
    first = 2 * n0 * n1
    assert first + n_edge <= n0 * n1 * n2
    for t, e in zip(tabs, pick):
        t.reshape(-1, order="F")[first:first + n_edge] = e            # a view: Fortran-contiguous
    flat = np.stack([t.reshape(-1, order="F") for t in tabs])
    assert np.all(np.isfinite(flat)) and np.all(np.abs(flat).sum(axis=0) > 0)
    assert np.all((flat == 0) | (np.abs(flat) >= np.finfo(f32).tiny))                 # no subnormal component
    assert np.any(flat[3] < 0)                                                        # scalar parts of either sign
    return (yaw, pitch, roll), tabs


def edge_model_problem(form, costs=True, j_storage=None):
    """The edge problem of launch form `form` (FORMS): a ProblemSpec with HJB_MODEL_QUAT_EULER321 whose tables are built directly
    (edge_tables), rate axes and torques with the reference's rate dynamics w_i' = w_i + h (c_i w_j w_k + U_i / J_i)
    (Solver_attitude.m:423-425) sized so that the library chooses that form.  costs=False: the same terms, all zero - the
    backup then returns the interpolated cost-to-go alone (the read-out stages)."""
    F = FORMS[form]
    (yaw, pitch, roll), tabs = edge_tables(F["n_ang"])
    X = [np.array(r, dtype=f32) for r in F["rates"]]
    assert all(3 <= len(x) <= 6 and np.any(x == 0) for x in X)
    h = f32(F["h"])
    J1, J2, J3 = INERTIA
    U = [np.linspace(-0.11, 0.11, k).astype(f32) for k in F["m"]]

    def wnext(c, Xb, Xc, Uc, JJ):
        return (h * (f32(c) * Xb[:, None, None] * Xc[None, :, None] + (Uc / f32(JJ))[None, None, :])).astype(f32)
    t1 = wnext((J2 - J3) / J1, X[1], X[2], U[0], J1)                                              # (w2, w3, U1)
    t2 = np.ascontiguousarray(np.transpose(wnext((J3 - J1) / J2, X[2], X[0], U[1], J2), (1, 0, 2)))   # (w1, w3, U2)
    t3 = wnext((J1 - J2) / J3, X[0], X[1], U[2], J3)                                              # (w1, w2, U3)
    nxt = [[], [], [],
           [Term((3,), X[0]), Term((4, 5, 6), t1)], [Term((4,), X[1]), Term((3, 5, 7), t2)], [Term((5,), X[2]), Term((3, 4, 8), t3)]]
    k = f32(1.0 if costs else 0.0)
    cost = [Term((3 + i,), k * (f32(6) * X[i] ** 2)) for i in range(3)] + \
           [Term((0, 1, 2), k * (f32(6) * tabs[i] ** 2)) for i in range(3)] + \
           [Term((6 + i,), k * (f32(4) * U[i] ** 2)) for i in range(3)]
    knots = [a.astype(np.float64) for a in (yaw, pitch, roll, X[0], X[1], X[2])]
    return ProblemSpec(knots, list(F["m"]), nxt, cost, dtype=np.float32, index_base=1, j_storage=j_storage,
                       model={"kind": "quat_euler321", "h": float(h), "tables": tabs})


def readout_terminal(spec, a):
    """J_next(x) = the knot of angle axis a, over the whole grid (float32, flat in the library's order): with zero costs the backup
    of it is the model's next angle a, up to the rounding of one weight and one lerp."""
    sh = [1] * 6
    sh[a] = -1
    k = np.asarray(spec.knots[a]).astype(f32).reshape(sh)
    return np.ascontiguousarray(np.broadcast_to(k, spec.n).reshape(-1, order="F"))
