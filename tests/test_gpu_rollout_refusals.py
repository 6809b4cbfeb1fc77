"""GPU test of the refusals the run functions of the affine and the attitude model make in their one entry frame (run_call,
csrc/rollout_host.h): hjb_rollout_run, _run_noisy, _run_greedy, _run_lookahead (fly_noise 0 and 1) and _run_attitude, each called
through ctypes with exactly one thing wrong and every output - device_ms included - pre-filled with a sentinel.  Every refusal is
HJB_E_INVALID with its own text, is made before any device work and leaves every output as it was; the good call made before the
refusals is repeated after them, bit for bit.  One affine object on a 3 x 3 grid (D = 2, n_u = 1, two planes) and one attitude
object on the smallest 6-D grid (two knots an axis), 2 trajectories, 2 steps.  The three-channel entry points have their sentinel
tests in test_gpu_rollout_pos_att.py, _pos_att_faults.py, _position.py and _attitude_simplified.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NT, K, SENTINEL = 2, 2, 7.25
I64_MAX = 2 ** 63 - 1


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _planes(*p):
    return np.array(p, dtype=np.int32)


class Entry:
    """One run entry point: how its arguments are laid out (`lead`: method or fly_noise; `streams`: seed and first_stream behind
    X0) and its per-step outputs as (rows, stages - n_steps) behind X_final [W] and cost."""

    def __init__(self, lib, name, W, lead, streams, paths):
        self.fn, self.name, self.W, self.lead, self.streams, self.paths = getattr(lib, name), name, W, lead, streams, paths

    def refused(self, lib, h, X, planes, text, lead=None, n_steps=K, n_traj=NT, first=0, null=(), keep=None):
        """Call with every output a sentinel; -> None after asserting HJB_E_INVALID, `text` and the sentinels.  null: arguments
        handed over as null pointers ("planes", "X0", "X_final"); keep: the paths handed over at all (default: every one)."""
        from hjbdp import _abi
        outs = [np.full(NT * self.W, SENTINEL), np.full(NT, SENTINEL)] + [np.full(NT * r * (K + e), SENTINEL) for r, e in self.paths]
        ptrs = [_dp(o) for o in outs]
        if "X_final" in null:
            ptrs[0] = None
        for i in range(len(self.paths)):
            if keep is not None and i not in keep:
                ptrs[2 + i] = None
        ms = C.c_double(SENTINEL)
        args = [h] + ([self.lead if lead is None else lead] if self.lead is not None else [])
        args += [n_steps, None if "planes" in null else _ip(planes), n_traj, None if "X0" in null else _dp(X)]
        args += [4, first] if self.streams else []
        st = self.fn(*args, *ptrs, C.byref(ms))
        err = lib.hjb_rollout_last_error(h).decode()
        assert st == _abi.HJB_E_INVALID and text in err, (self.name, text, st, err)
        assert all(np.all(o == SENTINEL) for o in outs) and ms.value == SENTINEL, (self.name, text)


def _bits(out):
    """a run's arrays as bytes (the time apart): equal dicts are equal bit for bit, NaNs included"""
    return {k: None if v is None else (v.dtype.str, v.shape, v.tobytes()) for k, v in out.items() if k != "device_ms"}


def test_single_fault_refusals_leave_the_outputs_and_the_object_alone(built):
    import hjbdp
    from hjbdp import _abi
    lib = hjbdp.load_library()
    rng = np.random.default_rng(32)
    knots = [np.array([-1.0, 0.0, 1.0]), np.array([-1.0, 0.25, 1.0])]
    labels = rng.integers(1, 4, size=(9, 2)).astype(np.int32)
    ut = np.array([-0.5, 0.0, 0.5])
    A, B = np.array([[1.0, 0.1], [0.0, 0.9]]), np.array([[0.0], [0.1]])
    J = rng.uniform(0.0, 2.0, size=(9, 2))
    off, w = np.array([[0.0, 0.0], [-0.05, 0.05]]), [0.5, 0.5]
    X0 = np.array([[0.3, -0.6], [0.2, 0.7]])                                    # [D, n_traj]
    k6 = [np.array([-0.5, 0.5])] * 6
    l6 = rng.integers(1, 3, size=(64, 2)).astype(np.uint8)
    u6 = rng.uniform(-0.1, 0.1, size=(2, 3))
    Q0 = np.zeros((7, NT))
    Q0[0:3] = rng.uniform(-0.2, 0.2, size=(3, NT))
    Q0[6] = 1.0

    xu = [(2, 1), (1, 0)]
    one = (1, 0)
    run = Entry(lib, "hjb_rollout_run", 2, _abi.HJB_LOOKUP_LINEAR, False, xu)
    noisy = Entry(lib, "hjb_rollout_run_noisy", 2, _abi.HJB_LOOKUP_LINEAR, True, xu + [one])
    greedy = Entry(lib, "hjb_rollout_run_greedy", 2, None, False, xu + [one, one])
    nominal = Entry(lib, "hjb_rollout_run_lookahead", 2, 0, True, xu + [one, one, one])
    fly = Entry(lib, "hjb_rollout_run_lookahead", 2, 1, True, xu + [one, one, one])
    attitude = Entry(lib, "hjb_rollout_run_attitude", 7, _abi.HJB_LOOKUP_NEAREST, False, [(7, 1), (3, 0), (3, 0)])
    no_w = dict(keep=(0, 1, 2, 3))                                              # a nominal plant takes no W_path
    affine = ((run, {}), (noisy, {}), (greedy, {}), (nominal, no_w), (fly, {}))
    by_labels, by_values = (run, noisy), (greedy, nominal, fly)

    Xc, Qc = np.ascontiguousarray(X0.T), np.ascontiguousarray(Q0.T)             # [n_traj, W] C order: the library's column-major
    Xn, Qn, Qz = Xc.copy(), Qc.copy(), Qc.copy()
    Xn[1, 0], Qn[0, 5] = np.inf, np.nan
    Qz[1, 3:7] = 0.0
    ok, ok6, free = _planes(0, 1), _planes(1, 0), _planes(-1, -1)

    with hjbdp.Rollout(knots, labels, ut) as ro, hjbdp.Rollout(knots, labels, ut) as bare, hjbdp.Rollout(knots, labels, ut) as half, \
            hjbdp.Rollout(k6, l6, u6) as ro6, hjbdp.Rollout(k6, l6, u6) as bare6:
        ro.set_model(A, B, q=[1.0, 0.5], r=[0.1])
        ro.set_noise(off, w)
        ro.set_values(J)
        ro.set_lookahead(off, w)
        ro6.set_attitude_model([1.0, 2.0, 3.0], 0.01, q=np.ones(7), r=np.ones(3))
        half.set_model(A, B)

        def good():
            return [_bits(o) for o in (ro.run(X0, ok, keep_path=True), ro.run_noisy(X0, ok, seed=4, first_stream=3, keep_path=True),
                                       ro.run_greedy(X0, ok, keep_path=True), ro.run_lookahead(X0, ok, keep_path=True),
                                       ro.run_lookahead(X0, ok, noisy=True, seed=4, first_stream=3, keep_path=True),
                                       ro6.run_attitude(Q0, ok6, keep_path=True))]
        before = good()
        h, h6 = ro._ro, ro6._ro

        # the null handle, the sizes, the planes and the starts: every entry point
        for e, kw in affine + ((attitude, {}),):
            X, pl, obj = (Qc, ok6, h6) if e is attitude else (Xc, ok, h)
            e.refused(lib, None, X, pl, "null handle", **kw)
            e.refused(lib, obj, X, pl, "n_steps=-1 < 0", n_steps=-1, **kw)
            e.refused(lib, obj, X, pl, "n_traj=-1 < 0", n_traj=-1, **kw)
            e.refused(lib, obj, X, pl, "null X0 / X_final", null=("X0",), **kw)
            e.refused(lib, obj, X, pl, "null X0 / X_final", null=("X_final",), **kw)
        for e, kw in affine:
            e.refused(lib, h, Xn, ok, "X0 element 2 is not finite", **kw)
        attitude.refused(lib, h6, Qn, ok6, "X0 element 5 is not finite")
        attitude.refused(lib, h6, Qz, ok6, "X0 column 1 has an all-zero quaternion")

        # the method, the model and the planes of the labels' controllers
        for e in by_labels + (attitude,):
            X, pl, obj, none, other = (Qc, ok6, h6, bare6._ro, h) if e is attitude else (Xc, ok, h, bare._ro, h6)
            e.refused(lib, obj, X, pl, "method 7", lead=7)
            e.refused(lib, none, X, pl, "run before hjb_rollout_set_")
            e.refused(lib, other, X, pl, "the object holds the")
            e.refused(lib, obj, X, pl, "null plane_of_step", null=("planes",))
            e.refused(lib, obj, X, _planes(0, 2), "plane_of_step[1] = 2 outside [0, 2)")
            e.refused(lib, obj, X, _planes(-1, 0), "plane_of_step[0] = -1 outside [0, 2)")

        # ... and of the values' controllers, with the sets they need
        for e in by_values:
            kw = no_w if e is nominal else {}
            e.refused(lib, bare._ro, Xc, ok, "before hjb_rollout_set_model", **kw)
            e.refused(lib, h6, Xc, ok, "needs the affine model", **kw)
            e.refused(lib, h, Xc, ok, "null value_plane_of_step", null=("planes",), **kw)
            e.refused(lib, h, Xc, _planes(0, 2), "value_plane_of_step[1] = 2 outside [-1, 2)", **kw)
            e.refused(lib, h, Xc, _planes(-2, 0), "value_plane_of_step[0] = -2 outside [-1, 2)", **kw)
        noisy.refused(lib, half._ro, Xc, ok, "hjb_rollout_run_noisy before hjb_rollout_set_noise")
        greedy.refused(lib, half._ro, Xc, ok, "hjb_rollout_run_greedy before hjb_rollout_set_values")
        nominal.refused(lib, half._ro, Xc, free, "hjb_rollout_run_lookahead before hjb_rollout_set_lookahead", **no_w)
        half.set_lookahead(off, w)
        nominal.refused(lib, half._ro, Xc, ok, "hjb_rollout_run_lookahead before hjb_rollout_set_values", **no_w)
        fly.refused(lib, half._ro, Xc, free, "with fly_noise=1 before hjb_rollout_set_noise")

        # the streams and fly_noise: refused before the object is needed
        for e in (noisy, fly):
            e.refused(lib, h, Xc, ok, "first_stream=-1 < 0", first=-1)
            e.refused(lib, h, Xc, ok, "first_stream + n_traj overflows", first=I64_MAX)
        nominal.refused(lib, h, Xc, ok, "fly_noise=2 is not 0 or 1", lead=2, **no_w)
        nominal.refused(lib, h, Xc, ok, "W_path given with fly_noise=0")

        assert good() == before
