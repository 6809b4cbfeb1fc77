"""CPU tests of how the stage and sweep side of hjbdp.core - Backup, MultiBackup, RankSlab and the lifetime they share with Rollout -
hands its arguments to the library: objects built without __init__ on a recording stand-in that returns 0, fills the hjb_result
and the hjb_info it is handed with known values and writes 100 * position + i into the output arrays that are not null.  Every
field of the hjb_solve_opts a sweep receives is read INSIDE the call (what it points to need not outlive it), every other call is
checked by position against _abi.SYMBOLS, every returned dict by its keys, dtypes, shapes, memory and content.  The pure decisions
of solve_batch and the channel store of the two three-channel solvers are pinned on hand-worked figures, its group runner on the
same stand-in (the members' hjb_solve_opts, the fallback to plain sweeps).  No library, no GPU."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

H = 0x1234                                                                      # every object's handle
N_ST = 3
N_STATES, J_ELEMS = 12, 20                                                      # hjb_get_info: a haloed J layout
RES = dict(stages_done=2, stopped_early=1, sweep_ms=1.5, last_e=0.25, last_e2=0.125)
TYPES = [(np.float32, np.uint8), (np.float64, np.int32)]
TYPE_IDS = ["f32_u8", "f64_i32"]
# class -> (handle attribute, destroy, last error, create)
CLASSES = {"Rollout": ("_ro", "hjb_rollout_destroy", "hjb_rollout_last_error", "hjb_rollout_create"),
           "Backup": ("_h", "hjb_destroy", "hjb_last_error", "hjb_create"),
           "MultiBackup": ("_m", "hjb_destroy_multi", "hjb_multi_last_error", "hjb_create_multi"),
           "RankSlab": ("_r", "hjb_rank_destroy", "hjb_rank_last_error", "hjb_rank_create")}


def _filled(at, size, dtype):
    """what the stand-in writes to the output at position `at` (narrow labels wrap)"""
    return (100 * at + np.arange(size)).astype(dtype)


def _mem(addr, dtype, count):
    """the `count` elements of `dtype` at an address, as a writable array"""
    return np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(addr), dtype=dtype)


def _spec(dtype=np.float64, idx_dtype=np.int32):
    from hjbdp.problem import ProblemSpec, Term
    k0, k1, u = np.linspace(0.0, 1.0, 3), np.linspace(-1.0, 1.0, 4), np.array([-1.0, 0.0, 1.0])
    return ProblemSpec([k0, k1], [3], [[Term((0,), k0), Term((2,), 0.1 * u)], [Term((1,), k1)]],
                       [Term((0,), k0 ** 2), Term((2,), u ** 2)], dtype=dtype, idx_dtype=idx_dtype)


class FakeLib:
    """Records every call as (name, args) and returns status[name] (0 unless set).  *_last_error tells a null object from a
    live one; hjb_get_info, hjb_get_option, hjb_rank_info and hjb_evaluate's trailing double are filled; a sweep call is read
    and answered by _sweep; on[name](args) runs inside any other call (to read what the arguments point to)."""

    def __init__(self, spec=None):
        self.calls, self.status, self.on, self.spec, self.seen = [], {}, {}, spec, None

    def hjb_status_string(self, st):
        return b"status %d" % st

    def _sweep(self, o, res):
        from hjbdp import _abi
        s, nS = self.spec, self.spec.nS
        pos = {name: i for i, (name, _) in enumerate(_abi.hjb_solve_opts._fields_)}
        seen = {f: getattr(o, f) for f in ("n_stages", "monitor_period", "monitor_tol", "progress_user", "progress_every_stage",
                                          "monitor_single")}
        seen["terminal"] = _mem(o.terminal, s.j_dtype, nS).copy() if o.terminal else None
        for f, dt, count in (("J_final", s.j_dtype, nS), ("idx_final", s.idx_np_dtype, nS),
                             ("J_stages", s.j_dtype, nS * o.n_stages), ("idx_stages", s.idx_np_dtype, nS * o.n_stages)):
            seen[f] = getattr(o, f)
            if seen[f]:
                a = _mem(seen[f], dt, count)
                seen[f + "_before"] = a.copy()
                a[:] = _filled(pos[f], count, dt)
        seen["progress"] = bool(o.progress)
        if o.progress:
            o.progress(None, 3, 0.5, 0.25, 2.0)
        seen["probe"] = None
        if o.probe:
            pb = o.probe.contents
            seen["probe"] = dict(lo=list(pb.lo), hi=list(pb.hi), control=list(pb.control),
                                 set={f for f in ("g", "x_next", "j_interp") if getattr(pb, f)})
        for k, v in RES.items():
            setattr(res, k, v)
        self.seen = seen

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name.endswith("last_error"):
                return b"error of the null object" if args[0] is None else b"error of the object"
            st = self.status.get(name, 0)
            if name in ("hjb_solve", "hjb_solve_multi"):
                self._sweep(args[1]._obj, args[2]._obj)
            elif name == "hjb_get_info":
                args[1]._obj.n_states, args[1]._obj.j_elems, args[1]._obj.kernel_variant = N_STATES, J_ELEMS, 1
            elif name in ("hjb_get_option", "hjb_rank_get_option"):
                args[2]._obj.value = 0 if args[1].startswith(b"dist_") else 7
            elif name == "hjb_rank_info":
                args[1][:] = list(range(10))
            elif name == "hjb_evaluate":
                args[-1]._obj.value = 1.5
            if name in self.on:
                self.on[name](args)
            return st
        return fn

    def named(self, name):
        (args,) = [a for n, a in self.calls if n == name]
        return args


def _make(cls_name, spec=None):
    import hjbdp.core as core
    obj = object.__new__(getattr(core, cls_name))
    obj.lib, obj.spec = FakeLib(spec), spec
    setattr(obj, CLASSES[cls_name][0], C.c_void_p(H))
    return obj


def _is_handle(a):
    return isinstance(a, C.c_void_p) and a.value == H


# ---- Backup.solve and MultiBackup.solve: the hjb_solve_opts the library receives and the dict that comes back -------------------
KEYWORDS = ["none", "terminal", "keep_J", "keep_idx", "progress", "progress_every_stage", "monitor_single", "probe"]
TAKES = {"Backup": KEYWORDS, "MultiBackup": KEYWORDS[:6]}
TERMINAL = np.arange(12.0).reshape(3, 4) - 2.0                                  # C-ordered [3, 4]
PROBE = {"lo": [0, 1], "hi": [2, 3], "control": [1], "want": ("g", "j_interp")}
BASE_KEYS = {"J", "idx", "J_stages", "idx_stages", "stages_done", "stopped_early", "sweep_ms", "last_e", "last_e2"}


@pytest.mark.parametrize("types", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("cls,on", [(c, k) for c in ("Backup", "MultiBackup") for k in TAKES[c]])
def test_solve(cls, on, types):
    from hjbdp import _abi
    spec = _spec(*types)
    jdt, idt, nS = np.dtype(types[0]), np.dtype(types[1]), 12
    assert (spec.nS, spec.n, spec.j_dtype, spec.idx_np_dtype) == (nS, (3, 4), jdt, idt)
    obj = _make(cls, spec)
    got = []
    kw = {"none": {}, "terminal": {"terminal": TERMINAL}, "keep_J": {"keep_J": True}, "keep_idx": {"keep_idx": True},
          "progress": {"progress": lambda *a: got.append(a)}, "progress_every_stage": {"progress_every_stage": True},
          "monitor_single": {"monitor_single": True}, "probe": {"probe": PROBE}}[on]
    out = obj.solve(N_ST, monitor_period=4, monitor_tol=0.5, **kw)

    fn = {"Backup": "hjb_solve", "MultiBackup": "hjb_solve_multi"}[cls]
    (called, args), = obj.lib.calls
    assert called == fn and len(args) == len(_abi.SYMBOLS[fn][1]) == 3 and _is_handle(args[0])
    assert isinstance(args[1]._obj, _abi.hjb_solve_opts) and isinstance(args[2]._obj, _abi.hjb_result)
    seen = obj.lib.seen
    assert (seen["n_stages"], seen["monitor_period"], seen["monitor_tol"], seen["progress_user"]) == (N_ST, 4, 0.5, None)
    assert seen["progress_every_stage"] == (1 if on == "progress_every_stage" else 0)
    assert seen["monitor_single"] == (1 if on == "monitor_single" else 0)
    if on == "terminal":
        assert seen["terminal"].dtype == jdt and np.array_equal(seen["terminal"], TERMINAL.reshape(-1, order="F").astype(jdt))
    else:
        assert seen["terminal"] is None
    at = {name: i for i, (name, _) in enumerate(_abi.hjb_solve_opts._fields_)}
    for key, field, dt in (("J", "J_final", jdt), ("idx", "idx_final", idt)):
        a = out[key]
        assert seen[field] and a.ctypes.data == seen[field] and a.dtype == dt and a.shape == (nS,)
        assert np.array_equal(a, _filled(at[field], nS, dt))
    for key, dt, kept in (("J_stages", jdt, on == "keep_J"), ("idx_stages", idt, on == "keep_idx")):
        a = out[key]
        if not kept:
            assert a is None and seen[key] is None
            continue
        assert a.ctypes.data == seen[key] and a.dtype == dt and a.shape == (nS, N_ST) and a.flags.f_contiguous
        assert not seen[key + "_before"].any()                                  # handed over zeroed
        assert np.array_equal(a, _filled(at[key], nS * N_ST, dt).reshape((nS, N_ST), order="F"))
    assert seen["progress"] == (on == "progress") and got == ([(3, 0.5, 0.25, 2.0)] if on == "progress" else [])
    if on == "probe":
        assert seen["probe"] == dict(lo=[0, 1, 0, 0, 0, 0], hi=[2, 3, 0, 0, 0, 0], control=[1, 0, 0], set={"g", "j_interp"})
        assert set(out["probe"]) == {"g", "j_interp"}
        for a in out["probe"].values():
            assert a.shape == (2, 2, N_ST) and a.dtype == spec.dtype and a.flags.f_contiguous and not a.any()
    else:
        assert seen["probe"] is None

    assert set(out) == (BASE_KEYS | {"probe"} if cls == "Backup" else BASE_KEYS)
    assert (out["stages_done"], out["stopped_early"], out["sweep_ms"], out["last_e"], out["last_e2"]) == (2, True, 1.5, 0.25, 0.125)
    assert type(out["stopped_early"]) is bool
    if cls == "Backup" and on != "probe":
        assert out["probe"] is None


@pytest.mark.parametrize("cls", ["Backup", "MultiBackup"])
def test_solve_refuses_a_terminal_of_the_wrong_size(cls):
    obj = _make(cls, _spec())
    with pytest.raises(ValueError, match="^terminal cost must have nS elements$"):
        obj.solve(N_ST, terminal=np.zeros(11))
    assert obj.lib.calls == []


# ---- the stages on host buffers, the evaluation sweep, the probe: by position against _abi.SYMBOLS -------------------------
@pytest.mark.parametrize("types", TYPES, ids=TYPE_IDS)
def test_backup_stage(types):
    from hjbdp import _abi
    spec = _spec(*types)
    bk = _make("Backup", spec)
    J_next = np.arange(20.0).reshape(4, 5)
    seen = {}
    bk.lib.on["hjb_backup_stage"] = lambda a: seen.update(J_next=_mem(a[1], spec.j_dtype, J_ELEMS).copy())
    Jo, idx = bk.backup_stage(J_next)
    args = bk.lib.named("hjb_backup_stage")
    assert len(args) == len(_abi.SYMBOLS["hjb_backup_stage"][1]) == 4 and _is_handle(args[0])
    assert np.array_equal(seen["J_next"], J_next.reshape(-1, order="F").astype(spec.j_dtype))
    assert (Jo.ctypes.data, Jo.dtype, Jo.shape) == (args[2], spec.j_dtype, (J_ELEMS,))
    assert (idx.ctypes.data, idx.dtype, idx.shape) == (args[3], spec.idx_np_dtype, (N_STATES,))
    with pytest.raises(ValueError, match="^J_next has 12 elements, the handle's J layout has 20$"):
        bk.backup_stage(np.zeros(12))


@pytest.mark.parametrize("types", TYPES, ids=TYPE_IDS)
def test_evaluate_stage(types):
    from hjbdp import _abi
    spec = _spec(*types)
    bk = _make("Backup", spec)
    J_next, labels = np.arange(20.0).reshape(4, 5), (np.arange(12) % 3).astype(spec.idx_np_dtype)
    seen = {}
    bk.lib.on["hjb_evaluate_stage"] = lambda a: seen.update(J_next=_mem(a[1], spec.j_dtype, J_ELEMS).copy(),
                                                            labels=_mem(a[2], spec.idx_np_dtype, N_STATES).copy())
    Jo = bk.evaluate_stage(J_next, labels)
    args = bk.lib.named("hjb_evaluate_stage")
    assert len(args) == len(_abi.SYMBOLS["hjb_evaluate_stage"][1]) == 4 and _is_handle(args[0])
    assert np.array_equal(seen["J_next"], J_next.reshape(-1, order="F").astype(spec.j_dtype)) and np.array_equal(seen["labels"], labels)
    assert (Jo.ctypes.data, Jo.dtype, Jo.shape) == (args[3], spec.j_dtype, (J_ELEMS,))
    with pytest.raises(ValueError, match="^J_next has 19 elements, the handle's J layout has 20$"):
        bk.evaluate_stage(np.zeros(19), labels)
    with pytest.raises(ValueError, match=r"^labels must be %s \(spec.idx_np_dtype\), got int64$" % spec.idx_np_dtype):
        bk.evaluate_stage(J_next, labels.astype(np.int64))
    with pytest.raises(ValueError, match=r"^labels of shape \(11,\): expected \(12,\)$"):
        bk.evaluate_stage(J_next, labels[:11])


@pytest.mark.parametrize("types", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("per_stage", [0, 1], ids=["labels_1d", "labels_2d"])
@pytest.mark.parametrize("opts", [False, True], ids=["bare", "terminal_keep_J"])
def test_evaluate(types, per_stage, opts):
    from hjbdp import _abi
    spec = _spec(*types)
    jdt, idt, nS = spec.j_dtype, spec.idx_np_dtype, 12
    bk = _make("Backup", spec)
    labels = (np.arange(nS * N_ST).reshape(N_ST, nS).T % 3).astype(idt) if per_stage else (np.arange(nS) % 3).astype(idt)
    seen = {}

    def inside(a):
        seen["labels"] = _mem(a[3], idt, labels.size).copy()
        seen["terminal"] = None if a[2] is None else _mem(a[2], jdt, nS).copy()
        seen["J_stages"] = None if a[6] is None else _mem(a[6], jdt, nS * N_ST).copy()
        _mem(a[5], jdt, nS)[:] = _filled(5, nS, jdt)
    bk.lib.on["hjb_evaluate"] = inside
    out = bk.evaluate(N_ST, labels, **({"terminal": TERMINAL, "keep_J": True} if opts else {}))
    (called, args), = bk.lib.calls
    assert called == "hjb_evaluate" and len(args) == len(_abi.SYMBOLS["hjb_evaluate"][1]) == 8 and _is_handle(args[0])
    assert (type(args[1]), args[1], type(args[4]), args[4]) == (int, N_ST, int, per_stage)
    assert np.array_equal(seen["labels"], labels.reshape(-1, order="F"))
    assert isinstance(args[7]._obj, C.c_double)
    assert set(out) == {"J", "J_stages", "sweep_ms"} and out["sweep_ms"] == 1.5
    assert (out["J"].ctypes.data, out["J"].dtype, out["J"].shape) == (args[5], jdt, (nS,)) and np.array_equal(out["J"], _filled(5, nS, jdt))
    if opts:
        assert np.array_equal(seen["terminal"], TERMINAL.reshape(-1, order="F").astype(jdt)) and not seen["J_stages"].any()
        Js = out["J_stages"]
        assert (Js.ctypes.data, Js.dtype, Js.shape) == (args[6], jdt, (nS, N_ST)) and Js.flags.f_contiguous
    else:
        assert args[2] is None and args[6] is None and out["J_stages"] is None


def test_evaluate_refusals():
    bk = _make("Backup", _spec())
    labels = np.zeros(12, np.int32)
    with pytest.raises(ValueError, match="^terminal cost must have nS elements$"):
        bk.evaluate(N_ST, labels, terminal=np.zeros(13))
    with pytest.raises(ValueError, match=r"^labels must be int32 \(spec.idx_np_dtype\), got uint8$"):
        bk.evaluate(N_ST, labels.astype(np.uint8))
    with pytest.raises(ValueError, match=r"^labels of shape \(12, 2\): expected \(12,\) or \(12, 3\)$"):
        bk.evaluate(N_ST, np.zeros((12, 2), np.int32))
    assert bk.lib.calls == []


@pytest.mark.parametrize("types", TYPES, ids=TYPE_IDS)
def test_probe_stage(types):
    from hjbdp import _abi
    spec = _spec(*types)
    bk = _make("Backup", spec)
    J_next = np.arange(12.0).reshape(3, 4)
    seen = {}

    def inside(a):
        pb = a[2]._obj
        seen.update(J_next=None if a[1] is None else _mem(a[1], spec.j_dtype, 12).copy(), lo=list(pb.lo), hi=list(pb.hi),
                    control=list(pb.control), ptrs=(pb.g, pb.x_next, pb.j_interp))
    bk.lib.on["hjb_probe_stage"] = inside
    out = bk.probe_stage({"lo": [0, 1], "hi": [2, 3], "control": [2]}, J_next)
    (called, args), = bk.lib.calls
    assert called == "hjb_probe_stage" and len(args) == len(_abi.SYMBOLS["hjb_probe_stage"][1]) == 3 and _is_handle(args[0])
    assert isinstance(args[2]._obj, _abi.hjb_probe)
    assert np.array_equal(seen["J_next"], J_next.reshape(-1, order="F").astype(spec.j_dtype))
    assert (seen["lo"], seen["hi"], seen["control"]) == ([0, 1, 0, 0, 0, 0], [2, 3, 0, 0, 0, 0], [2, 0, 0])
    assert seen["ptrs"] == (out["g"].ctypes.data, out["x_next"].ctypes.data, out["j_interp"].ctypes.data)
    assert out["g"].shape == out["j_interp"].shape == (2, 2) and out["x_next"].shape == (2, 2, 2)
    assert all(a.dtype == spec.dtype and a.flags.f_contiguous for a in out.values())
    bk.lib.calls.clear()
    out = bk.probe_stage({"lo": [0, 0], "hi": [1, 1], "control": [0], "want": ("g",)})
    assert bk.lib.calls[0][1][1] is None and seen["ptrs"] == (out["g"].ctypes.data, None, None) and set(out) == {"g"}
    with pytest.raises(ValueError, match="^j_interp needs J_next$"):
        bk.probe_stage({"lo": [0, 0], "hi": [1, 1], "control": [0]})


# ---- device pointers and streams: a tensor-like object, a DeviceBuffer, a bare integer and None ------------------------------
class _Tensor:
    def data_ptr(self):
        return 0x1000


@pytest.fixture
def buf():
    import hjbdp.core as core
    b = object.__new__(core.DeviceBuffer)
    b.ptr = 0x2000
    yield b
    b.ptr = None                                                                # nothing to free


def _ints(args, want):
    assert [type(a) for a in args] == [int if w is not None else type(None) for w in want] and list(args) == list(want), args


def test_stage_device_calls(buf):
    from hjbdp import _abi
    t = _Tensor()
    bk = _make("Backup", _spec())
    bk.backup_stage_device(t, buf, None)
    bk.backup_stage_device(0x3000, t, buf, stream=77)
    bk.evaluate_stage_device(buf, 0x3000, t)
    bk.evaluate_stage_device(t, buf, 0x3000, stream=5)
    bk.check_device_status()
    bk.check_device_status(stream=9)
    want = [("hjb_backup_stage_device", (0x1000, 0x2000, None, None)), ("hjb_backup_stage_device", (0x3000, 0x1000, 0x2000, 77)),
            ("hjb_evaluate_stage_device", (0x2000, 0x3000, 0x1000, None)), ("hjb_evaluate_stage_device", (0x1000, 0x2000, 0x3000, 5)),
            ("hjb_check_device_status", (None,)), ("hjb_check_device_status", (9,))]
    assert len(bk.lib.calls) == len(want)
    for (called, args), (fn, rest) in zip(bk.lib.calls, want):
        assert called == fn and len(args) == len(_abi.SYMBOLS[fn][1]) and _is_handle(args[0])
        _ints(args[1:], rest)


@pytest.mark.parametrize("method,fn", [("stage", "hjb_rank_stage"), ("stage_post", "hjb_rank_stage_post")])
def test_rank_stage_calls(buf, method, fn):
    from hjbdp import _abi
    t = _Tensor()
    rk = _make("RankSlab", _spec())
    getattr(rk, method)(t, buf, 0x3000)
    getattr(rk, method)(buf, 0x3000, None, compute_stream=0, halo_stream=9)
    getattr(rk, method)(0x3000, t, buf, compute_stream=8, halo_stream=0)
    want = [(0x1000, 0x2000, 0x3000, None, None), (0x2000, 0x3000, None, None, 9), (0x3000, 0x1000, 0x2000, 8, None)]
    assert len(rk.lib.calls) == 3
    for (called, args), rest in zip(rk.lib.calls, want):
        assert called == fn and len(args) == len(_abi.SYMBOLS[fn][1]) == 6 and _is_handle(args[0])
        _ints(args[1:], rest)


def test_rank_wait_strips_and_status():
    rk = _make("RankSlab", _spec())
    rk.lib.on["hjb_rank_wait_strips"] = lambda a: setattr(a[2]._obj, "value", 1)
    assert rk.wait_strips(0) is True and rk.wait_strips(6) is True
    rk.check_device_status()
    rk.check_device_status(stream=4)
    assert [(n, a[1]) for n, a in rk.lib.calls] == [("hjb_rank_wait_strips", None), ("hjb_rank_wait_strips", 6),
                                                    ("hjb_rank_check_status", None), ("hjb_rank_check_status", 4)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("cls,fn", [("Backup", "hjb_device_fill_separable"), ("RankSlab", "hjb_rank_fill_separable")])
def test_fill_separable(buf, cls, fn, dtype):
    from hjbdp import _abi
    obj = _make(cls, _spec(dtype, np.int32))
    vecs = [[1, 2, 3], np.arange(4.0)[::-1]]
    seen = []
    obj.lib.on[fn] = lambda a: seen.append([_mem(a[1][k], dtype, len(v)).copy() for k, v in enumerate(vecs)])
    obj.fill_separable(vecs, _Tensor())
    obj.fill_separable(vecs, buf, stream=3)
    obj.fill_separable(vecs, 0x3000, stream=0)
    assert len(obj.lib.calls) == 3
    for (called, args), got, rest in zip(obj.lib.calls, seen, [(0x1000, None), (0x2000, 3), (0x3000, None)]):
        assert called == fn and len(args) == len(_abi.SYMBOLS[fn][1]) == 4 and _is_handle(args[0])
        assert isinstance(args[1], C.c_void_p * 2)
        assert all(g.dtype == dtype and np.array_equal(g, np.asarray(v, dtype=dtype)) for g, v in zip(got, vecs))
        _ints(args[2:], rest)


# ---- lifetime and errors: one rule for the four handle classes --------------------------------------------------------------
@pytest.mark.parametrize("cls", list(CLASSES))
def test_close_destroys_once(cls):
    attr, destroy, _, _ = CLASSES[cls]
    obj = _make(cls)
    lib = obj.lib
    obj.close()
    (called, args), = lib.calls
    assert called == destroy and len(args) == 1 and _is_handle(args[0])
    assert getattr(obj, attr).value is None
    obj.close()
    obj.__del__()
    assert len(lib.calls) == 1


@pytest.mark.parametrize("cls", list(CLASSES))
def test_with_closes(cls):
    """(RankSlab is a context manager like the other three)"""
    attr, destroy, _, _ = CLASSES[cls]
    obj = _make(cls)
    with obj as same:
        assert same is obj and obj.lib.calls == []
    assert [n for n, _ in obj.lib.calls] == [destroy] and getattr(obj, attr).value is None


@pytest.mark.parametrize("cls", list(CLASSES))
def test_del_survives_a_half_made_object(cls):
    import hjbdp.core as core
    object.__new__(getattr(core, cls)).__del__()                                 # no handle attribute, no lib


@pytest.mark.parametrize("cls,call", [("Rollout", lambda o: o.set_option("chunk", 4)), ("Backup", lambda o: o.set_option("variant", 4)),
                                      ("Backup", lambda o: o.get_option("cs_split")), ("Backup", lambda o: o.check_device_status()),
                                      ("MultiBackup", lambda o: o.set_option("variant", 4)), ("MultiBackup", lambda o: o.slab_info(0)),
                                      ("RankSlab", lambda o: o.get_option("variant")), ("RankSlab", lambda o: o.refresh())])
def test_a_status_raises_the_objects_last_error(cls, call):
    import hjbdp
    last_error = CLASSES[cls][2]
    obj = _make(cls, _spec())
    obj.lib.status = {n: 3 for n in ("hjb_rollout_set_option", "hjb_set_option", "hjb_get_option", "hjb_check_device_status",
                                     "hjb_multi_set_option", "hjb_multi_slab_info", "hjb_rank_get_option", "hjb_rank_info")}
    with pytest.raises(hjbdp.HjbError, match=r"^libhjbdp: error of the object \(status 3\)$") as e:
        call(obj)
    assert e.value.status == 3
    called, args = obj.lib.calls[-1]
    assert called == last_error and len(args) == 1 and _is_handle(args[0])


@pytest.mark.parametrize("cls", list(CLASSES))
def test_a_failed_create_raises_and_leaves_a_null_handle(cls, monkeypatch):
    import hjbdp
    import hjbdp.core as core
    attr, destroy, last_error, create = CLASSES[cls]
    lib = FakeLib()
    lib.status[create] = 4
    monkeypatch.setattr(core, "load_library", lambda path=None: lib)
    spec = _spec()
    obj = object.__new__(getattr(core, cls))
    init = {"Rollout": lambda: obj.__init__(spec.knots, np.ones(12, np.uint8), [0.0, 1.0]), "Backup": lambda: obj.__init__(spec, device=0),
            "MultiBackup": lambda: obj.__init__(spec, [0, 0]), "RankSlab": lambda: obj.__init__(spec, 0, 0, 2)}[cls]
    with pytest.raises(hjbdp.HjbError, match=r"^libhjbdp: error of the null object \(status 4\)$") as e:
        init()
    assert e.value.status == 4
    assert [n for n, _ in lib.calls] == [create, last_error] and lib.calls[1][1] == (None,)
    assert getattr(obj, attr).value is None
    obj.close()
    assert destroy not in [n for n, _ in lib.calls]


def test_an_error_without_text_falls_back_to_the_status_string():
    import hjbdp
    bk = _make("Backup", _spec())
    bk.lib.status["hjb_set_option"] = 2
    bk.lib.hjb_last_error = lambda h: None
    with pytest.raises(hjbdp.HjbError, match=r"^libhjbdp: status 2 \(status 2\)$"):
        bk.set_option("variant", 1)


# ---- solve_batch's two pure decisions ---------------------------------------------------------------------------------------
def _member(n=(8, 8), j_dtype=np.float32, cost64=False):
    return SimpleNamespace(n=tuple(n), D=len(n), nS=int(np.prod(n)), j_dtype=np.dtype(j_dtype),
                           cost_dtype=np.dtype(np.float64) if cost64 else None)


def test_batch_groups_keys():
    from hjbdp.core import _batch_groups
    variants, axes = [7, 7, 5, 7, 0], [2, 2, None, 3, None]
    specs = [_member((60, 5, 8, 8)), _member((60, 5, 8, 8)), _member(), _member((60, 5, 8, 8)), _member()]
    # 0 and 1 sweep columns along one group axis; 3 along another; 2 is the only table-kernel member; 4 runs neither kernel
    assert _batch_groups(variants, axes, specs) == [[0, 1], [2], [3], [4]]
    # a float64 cost is another form of the column sweep: 1 leaves 0
    specs[1] = _member((60, 5, 8, 8), cost64=True)
    assert _batch_groups(variants, axes, specs) == [[0], [1], [2], [3], [4]]
    # the table kernel: one (j_dtype, D) per launch, and only up to D = 4
    specs = [_member(), _member(j_dtype=np.float64), _member(), _member((4, 4, 4)), _member((2,) * 5), _member((2,) * 5)]
    assert _batch_groups([5] * 6, [None] * 6, specs) == [[0, 2], [1], [3], [4], [5]]


def test_batch_groups_dissolves_a_table_group_beyond_one_round_of_wave_slots():
    from hjbdp.core import _batch_groups
    assert 256 * 32 * 64 == 524288
    big, fits = _member((300000,)), _member((200000,))                         # 600,000 > 524,288 >= 400,000
    assert _batch_groups([5, 5], [None, None], [fits, fits]) == [[0, 1]]
    assert _batch_groups([5, 5], [None, None], [big, big]) == [[0], [1]]
    # the dissolved members go behind every group that stayed
    assert _batch_groups([5, 0, 5, 7], [None, None, None, 2], [big, _member(), big, _member((60, 5, 8, 8))]) == [[1], [3], [0], [2]]
    # one member alone is never "dissolved": it keeps its place
    assert _batch_groups([5, 0], [None, None], [_member((600000,)), _member()]) == [[0], [1]]


def test_batch_cs_split():
    from hjbdp.core import _batch_cs_split
    two = [_member((60, 5, 8, 8))] * 2                                          # cols = 2 * (1 * 8 * 8) = 128; slots = 6 * 4 * 256 = 6144
    assert _batch_cs_split(two, [7, 7], [49, 100], False) == 48                  # 6144 // 128
    assert _batch_cs_split(two, [7, 7], [100, 48], False) == 0                   # not below every member's own split
    assert _batch_cs_split(two, [7, 7], [49, 100], True) == 40                   # slots = 5 * 4 * 256 = 5120
    assert _batch_cs_split(two, [7, 7], [40, 100], True) == 0
    # n0 = 61: two column pieces per column -> cols = 256
    assert _batch_cs_split([_member((61, 5, 8, 8))] * 2, [7, 7], [100, 100], False) == 24
    # members of other kernels do not count
    assert _batch_cs_split([two[0], _member(), two[0]], [7, 5, 7], [49, 49], False) == 48
    # three 120^4: cols = 3 * (2 * 120 * 120) = 86,400 > slots -> quotient 0 -> 1, kept while every own split is above 1
    three = [_member((120,) * 4)] * 3
    assert _batch_cs_split(three, [7, 7, 7], [2, 3, 2], False) == 1
    assert _batch_cs_split(three, [7, 7, 7], [2, 1, 2], False) == 0


def test_solve_group_makes_one_batched_call_or_falls_back_to_plain_sweeps():
    import hjbdp
    from hjbdp import _abi
    from hjbdp.core import _solve_group
    spec = _spec(np.float32, np.uint8)
    lib = FakeLib(spec)
    bks = [_make("Backup", spec) for _ in range(3)]
    for k, bk in enumerate(bks):
        bk.lib, bk._h = lib, C.c_void_p(H + k)
    seen, got = [], []

    def batch(a):
        for k in range(a[0]):
            lib._sweep(a[2][k].contents, a[3][k].contents)
            seen.append((a[1][k], lib.seen))
    lib.on["hjb_solve_batch"] = batch
    kw = dict(monitor_period=4, monitor_tol=0.5, progress=lambda *a: got.append(a), monitor_single=True)
    outs, sizes = _solve_group(lib, bks, [2, 0], N_ST, kw)
    (called, args), = lib.calls
    assert called == "hjb_solve_batch" and len(args) == len(_abi.SYMBOLS["hjb_solve_batch"][1]) == 4 and args[0] == 2 and sizes == [2]
    assert [h for h, _ in seen] == [H + 2, H] and got == [(3, 0.5, 0.25, 2.0)] * 2
    for (_, s), out in zip(seen, outs):
        assert (s["n_stages"], s["monitor_period"], s["monitor_tol"], s["monitor_single"], s["progress_every_stage"]) == (N_ST, 4, 0.5, 1, 0)
        assert s["terminal"] is None and s["J_stages"] is None and s["idx_stages"] is None and s["probe"] is None and s["progress"]
        assert set(out) == BASE_KEYS | {"probe"} and out["probe"] is None and out["J_stages"] is None and out["idx_stages"] is None
        assert out["J"].ctypes.data == s["J_final"] and out["idx"].ctypes.data == s["idx_final"]
        assert (out["J"].dtype, out["idx"].dtype, out["J"].shape, out["idx"].shape) == (np.float32, np.uint8, (12,), (12,))
        assert (out["stages_done"], out["stopped_early"], out["sweep_ms"], out["last_e"], out["last_e2"]) == (2, True, 1.5, 0.25, 0.125)
    assert outs[0]["J"].ctypes.data != outs[1]["J"].ctypes.data

    del lib.on["hjb_solve_batch"]                                               # a group the library does not take: plain sweeps
    lib.calls.clear()
    lib.status["hjb_solve_batch"] = _abi.HJB_E_UNSUPPORTED
    outs, sizes = _solve_group(lib, bks, [2, 0], N_ST, kw)
    assert sizes == [1, 1] and len(outs) == 2 and all(set(o) == BASE_KEYS | {"probe"} for o in outs)
    assert lib.calls[0][0] == "hjb_solve_batch" and sorted((n, a[0].value) for n, a in lib.calls[1:]) == [("hjb_solve", H), ("hjb_solve", H + 2)]

    lib.calls.clear()                                                           # any other status is the call's error
    lib.status["hjb_solve_batch"] = _abi.HJB_E_DEVICE
    with pytest.raises(hjbdp.HjbError, match=r"^libhjbdp: error of the null object \(status 3\)$"):
        _solve_group(lib, bks, [2, 0], N_ST, kw)
    assert [n for n, _ in lib.calls] == ["hjb_solve_batch", "hjb_last_error"]

    lib.calls.clear()                                                           # a member alone: its plain sweep, no batched call
    outs, sizes = _solve_group(lib, bks, [1], N_ST, kw)
    assert sizes == [1] and len(outs) == 1 and [(n, a[0].value) for n, a in lib.calls] == [("hjb_solve", H + 1)]


# ---- the channel store of the two three-channel solvers -----------------------------------------------------------------------
@pytest.mark.parametrize("keep_policy", [False, True], ids=["last_stage", "keep_policy"])
def test_store_channel_results(keep_policy):
    from hjbdp.core import store_channel_results
    from hjbdp.solver_position import NearestPolicy
    n_st = 2
    grids = [(np.linspace(-1, 1, 3), np.linspace(0, 1, 4)), (np.linspace(-2, 2, 5), np.linspace(0, 1, 2)),
             (np.linspace(-3, 3, 2), np.linspace(0, 1, 3))]
    built = [(None, a, b) for a, b in grids]
    U = np.array([-0.5, 0.0, 0.5])
    outs = []
    for ch, (a, b) in enumerate(grids):
        nS = len(a) * len(b)
        outs.append({"J": 10.0 * ch + np.arange(nS), "idx": (1 + (np.arange(nS) + ch) % 3).astype(np.int32), "sweep_ms": 1.0 + ch,
                     "idx_stages": np.asfortranarray(1 + (np.arange(nS * n_st).reshape(n_st, nS).T + ch) % 3).astype(np.int32)
                     if keep_policy else None})
    solver = SimpleNamespace(U_vector=U, F_values=[None] * 3, U_idx=[None] * 3, sweep_ms=[None] * 3)
    store_channel_results(solver, built, outs, n_st, keep_policy, U.astype(np.float64))
    for ch, (a, b) in enumerate(grids):
        shape = (len(a), len(b))
        assert solver.F_values[ch].shape == shape and np.array_equal(solver.F_values[ch], outs[ch]["J"].reshape(shape, order="F"))
        assert solver.U_idx[ch].shape == shape and np.array_equal(solver.U_idx[ch], outs[ch]["idx"].reshape(shape, order="F"))
        assert np.shares_memory(solver.F_values[ch], outs[ch]["J"]) and np.shares_memory(solver.U_idx[ch], outs[ch]["idx"])
        assert solver.sweep_ms[ch] == 1.0 + ch
        pol = getattr(solver, "U%d_Opt" % (ch + 1))
        assert isinstance(pol, NearestPolicy) and pol.GridVectors[0] is a and pol.GridVectors[1] is b
        assert pol.Values.shape == shape and np.array_equal(pol.Values, U[solver.U_idx[ch] - 1])
    if keep_policy:
        for ch, (a, b) in enumerate(grids):
            ix = solver.U_idx_stages[ch]
            assert ix.shape == (len(a), len(b), n_st) and np.array_equal(ix, outs[ch]["idx_stages"].reshape(ix.shape, order="F"))
            assert solver.U_Opt_stages[ch].shape == ix.shape and np.array_equal(solver.U_Opt_stages[ch], U[ix - 1])
    else:
        assert solver.U_idx_stages is None and solver.U_Opt_stages is None
