"""CPU tests of how hjbdp.Rollout's nine run methods hand their arguments to the library's nine run entry points: a Rollout built
without __init__ on a recording stand-in for the library, every argument checked by value or by dtype, shape, contiguity and
content, its position against _abi.SYMBOLS, and every returned dict by its keys, dtypes, shapes and content, with keep_path on and
off (run_lookahead also with noisy on and off).  No library, no GPU."""
import ctypes as C

import numpy as np
import pytest

D, NU, NT, K = 2, 1, 3, 4
SEED, FIRST = 2 ** 64 + 7, 11
PLANES, VPLANES = [0, 1, 1, 0], np.array([1, 2, 2, 1], dtype=np.int64)
F64P, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _x0(width):
    return 0.25 * np.arange(width * NT, dtype=np.float64).reshape(width, NT) - 1.0       # [width, n_traj]


def _arr(ptr):
    """the numpy array a pointer made by ndarray.ctypes.data_as keeps alive"""
    return ptr._arr


def _filled(at, size):
    """what the stand-in writes to the output at argument position `at`"""
    return 100.0 * at + np.arange(size)


class FakeLib:
    """Records every call as (name, args).  A run entry point also writes its outputs - the arguments at the positions `outs`
    that are not null, element i of the one at position p as 100 p + i - and 1.5 ms to a trailing double by reference."""

    def __init__(self):
        self.calls, self.outs = [], ()

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            for at in self.outs:
                if args[at] is not None:
                    a = _arr(args[at])
                    a[...] = _filled(at, a.size).reshape(a.shape).astype(a.dtype)
            if hasattr(args[-1], "_obj"):
                args[-1]._obj.value = 1.5
            return 0
        return fn


@pytest.fixture
def ro():
    import hjbdp
    r = object.__new__(hjbdp.Rollout)
    r.lib, r._ro = FakeLib(), C.c_void_p(0x1234)
    r.D, r.n_u, r.n = D, NU, [3, 3]
    r._pa_steps = r._pos_steps = K
    yield r
    r._ro = C.c_void_p()                                                        # nothing to destroy


def _is_array(a, ctype, dtype, want):
    arr = _arr(a)
    want = np.asarray(want, dtype=dtype)
    assert arr.dtype == dtype and arr.shape == want.shape and arr.flags.c_contiguous, (arr.dtype, arr.shape, arr.flags)
    assert np.array_equal(arr, want), (arr, want)
    assert a._type_ is ctype


# A case: the entry point, the state width, the call, and the arguments behind the handle in the order of the prototype -
#   lead:  the scalars in front of n_steps, by value
#   mid:   what sits between X0 and X_final: ints and floats by value, (dtype, content) arrays, None a null pointer
#   vecs:  the per-trajectory outputs behind X_final, (key, dtype) each
#   paths: (key, rows, stages - n_steps, how the dict shows it): "3d" the [n_traj, rows, stages] view, "int" and "row" the one
#          row squeezed to [n_traj, stages], as int32 or as it is; `null`: paths handed over as null pointers whatever keep_path
#   tail:  the per-trajectory outputs behind the paths
#   ms:    whether the call ends in device_ms
def _cases():
    from hjbdp import _abi
    xp, up = ("X_path", D, 1, "3d"), ("U_path", NU, 0, "3d")
    lp, vp, wp = ("L_path", 1, 0, "int"), ("V_path", 1, 0, "row"), ("W_path", 1, 0, "int")
    att = [("X_path", 7, 1, "3d"), ("U_path", 3, 0, "3d"), ("A_path", 3, 0, "3d")]
    pa = [("X_path", 13, 1, "3d"), ("F_path", 12, 0, "3d"), ("FM_path", 6, 0, "3d")]
    cost = [("cost", np.float64)]
    return {
        "run": dict(fn="hjb_rollout_run", width=D, call=lambda r, X, keep: r.run(X, PLANES, method="nearest", keep_path=keep),
                    lead=[_abi.HJB_LOOKUP_NEAREST], planes=PLANES, vecs=cost, paths=[xp, up], ms=True),
        "run_noisy": dict(fn="hjb_rollout_run_noisy", width=D,
                          call=lambda r, X, keep: r.run_noisy(X, PLANES, seed=SEED, first_stream=FIRST, keep_path=keep),
                          lead=[_abi.HJB_LOOKUP_LINEAR], planes=PLANES, mid=[7, FIRST], vecs=cost, paths=[xp, up, wp], ms=True),
        "run_greedy": dict(fn="hjb_rollout_run_greedy", width=D, call=lambda r, X, keep: r.run_greedy(X, VPLANES, keep_path=keep),
                           planes=VPLANES, vecs=cost, paths=[xp, up, lp, vp], ms=True),
        "run_lookahead_nominal": dict(fn="hjb_rollout_run_lookahead", width=D,
                                      call=lambda r, X, keep: r.run_lookahead(X, VPLANES, keep_path=keep), lead=[0], planes=VPLANES,
                                      mid=[0, 0], vecs=cost, paths=[xp, up, lp, vp, wp], null={"W_path"}, ms=True),
        "run_lookahead_noisy": dict(fn="hjb_rollout_run_lookahead", width=D,
                                    call=lambda r, X, keep: r.run_lookahead(X, VPLANES, noisy=True, seed=SEED, first_stream=FIRST,
                                                                            keep_path=keep),
                                    lead=[1], planes=VPLANES, mid=[7, FIRST], vecs=cost, paths=[xp, up, lp, vp, wp], ms=True),
        "run_attitude": dict(fn="hjb_rollout_run_attitude", width=7,
                             call=lambda r, X, keep: r.run_attitude(X, PLANES, method="linear", keep_path=keep),
                             lead=[_abi.HJB_LOOKUP_LINEAR], planes=PLANES, vecs=cost, paths=att, ms=True),
        "run_pos_att": dict(fn="hjb_rollout_run_pos_att", width=13, call=lambda r, X, keep: r.run_pos_att(X, keep_path=keep),
                            planes=[0] * K, paths=pa),
        "run_pos_att_faults": dict(fn="hjb_rollout_run_pos_att_faults", width=13,
                                   call=lambda r, X, keep: r.run_pos_att_faults(X, PLANES, fault_mask=5, fault_stage=[1, 2, 3],
                                                                                pos_tol=0.5, keep_path=keep),
                                   planes=PLANES, mid=[(np.int32, [5, 5, 5]), (np.int32, [1, 2, 3]), None, 0.5, float("inf")],
                                   vecs=[("impulse", np.float64), ("settle_stage", np.int32)], paths=pa, ms=True),
        "run_position": dict(fn="hjb_rollout_run_position", width=6, call=lambda r, X, keep: r.run_position(X, keep_path=keep),
                             planes=[0] * K, paths=[("X_path", 6, 1, "3d"), ("A_path", 3, 0, "3d")], tail=[("off_schedule", np.int32)]),
        "run_attitude_simplified": dict(fn="hjb_rollout_run_attitude_simplified", width=7,
                                        call=lambda r, X, keep: r.run_attitude_simplified(X, PLANES, keep_path=keep), planes=PLANES,
                                        vecs=cost, paths=att),
    }


CASE_NAMES = ["run", "run_noisy", "run_greedy", "run_lookahead_nominal", "run_lookahead_noisy", "run_attitude", "run_pos_att",
              "run_pos_att_faults", "run_position", "run_attitude_simplified"]


def test_the_cases_are_the_nine_run_methods():
    import hjbdp
    cases = _cases()
    assert sorted(cases) == sorted(CASE_NAMES)
    methods = {n for n in dir(hjbdp.Rollout) if n.startswith("run") and "campaign" not in n}
    assert methods == {n.replace("_nominal", "").replace("_noisy", "") if n.startswith("run_lookahead") else n for n in cases}
    assert len(methods) == 9


@pytest.mark.parametrize("keep", [False, True], ids=["no_path", "keep_path"])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_run_method(ro, case, keep):
    from hjbdp import _abi
    c = _cases()[case]
    W, types = c["width"], _abi.SYMBOLS[c["fn"]][1]
    lead, mid, vecs, tail, null = c.get("lead", []), c.get("mid", []), c.get("vecs", []), c.get("tail", []), c.get("null", set())
    first_out = 1 + len(lead) + 4 + len(mid)                                    # X_final's position
    n_out = 1 + len(vecs) + len(c["paths"]) + len(tail)
    ro.lib.outs = range(first_out, first_out + n_out)
    X0 = _x0(W)
    out = c["call"](ro, X0, keep)

    (called, args), = ro.lib.calls
    assert called == c["fn"] and len(args) == len(types), (called, len(args))
    assert args[0] is ro._ro and types[0] is C.c_void_p
    at = 1
    for want in lead:
        assert type(args[at]) is int and args[at] == want and types[at] is C.c_int32, (case, at, args[at])
        at += 1
    assert (type(args[at]), args[at], types[at]) == (int, K, C.c_int32)
    _is_array(args[at + 1], C.c_int32, np.int32, c["planes"])
    assert types[at + 1] == I32P
    assert (type(args[at + 2]), args[at + 2], types[at + 2]) == (int, NT, C.c_int64)
    _is_array(args[at + 3], C.c_double, np.float64, X0.T)                       # [n_traj, W] C order = [W, n_traj] column-major
    assert types[at + 3] == F64P
    at += 4
    for want in mid:
        if want is None:
            assert args[at] is None and types[at] in (I32P, F64P)
        elif isinstance(want, tuple):
            _is_array(args[at], C.c_int32, *want)
            assert types[at] == I32P
        elif isinstance(want, float):
            assert type(args[at]) is float and args[at] == want and types[at] is C.c_double
        else:
            assert type(args[at]) is int and args[at] == want and types[at] in (C.c_uint64, C.c_int64), (case, at, args[at])
        at += 1
    assert at == first_out

    expect = {}                                                                 # the dict, from what the stand-in wrote
    arr = _arr(args[at])
    assert arr.dtype == np.float64 and arr.shape == (NT, W) and arr.flags.c_contiguous and types[at] == F64P
    expect["X_final"] = _filled(at, NT * W).reshape(NT, W).T
    assert out["X_final"].shape == (W, NT) and out["X_final"].flags.f_contiguous
    at += 1
    for key, dtype in list(vecs) + [("the paths", None)] + list(tail):
        if dtype is None:
            for name, rows, extra, show in c["paths"]:
                stages = K + extra
                assert types[at] == F64P
                if not keep or name in null:
                    assert args[at] is None
                    expect[name] = None
                else:
                    arr = _arr(args[at])
                    assert arr.dtype == np.float64 and arr.size == NT * rows * stages and arr.flags.c_contiguous, (name, arr.shape)
                    full = _filled(at, arr.size).reshape((NT, rows, stages), order="F")
                    expect[name] = {"3d": full, "row": full[:, 0, :], "int": full[:, 0, :].astype(np.int32)}[show]
                at += 1
            continue
        arr = _arr(args[at])
        assert arr.dtype == dtype and arr.shape == (NT,) and arr.flags.c_contiguous, (key, arr.dtype, arr.shape)
        assert types[at] == (F64P if dtype == np.float64 else I32P) and args[at]._type_ is (C.c_double if dtype == np.float64 else C.c_int32)
        expect[key] = _filled(at, NT).astype(dtype)
        at += 1
    if c.get("ms"):
        assert isinstance(args[at]._obj, C.c_double) and types[at] == F64P
        expect["device_ms"] = 1.5
        at += 1
    assert at == len(args)

    assert set(out) == set(expect), (sorted(out), sorted(expect))
    for key, want in expect.items():
        got = out[key]
        if want is None:
            assert got is None, key
        elif key == "device_ms":
            assert type(got) is float and got == want
        else:
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (key, got, want)


def test_one_start_and_no_planes(ro):
    """a 1-D X0 is one start; the planes default to the stages the model set last covers"""
    ro._pa_steps = 2
    out = ro.run_pos_att(np.arange(13.0))
    (_, args), = ro.lib.calls
    assert args[1] == 2 and _arr(args[2]).tolist() == [0, 0] and args[3] == 1 and _arr(args[4]).shape == (1, 13)
    assert out["X_final"].shape == (13, 1) and out["X_path"] is None
