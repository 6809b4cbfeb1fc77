"""GPU tests (-m gpu): ONE handle with stages in flight on TWO streams (include/hjbdp.h, hjb_backup_stage_device).  Every
serving stage kernel is forced on a small problem; rounds of `stage(J_a -> O_a, stream A); stage(J_b -> O_b, stream B)` are
enqueued without a host synchronisation in between, over outputs prefilled with NaN, and each output must then equal a plain
hjb_backup_stage of its own input on the same handle, bit for bit, labels included.  K15 keeps per-handle claim counters for
its chunk walk (kernels_uniwin.h): two launches that shared (and re-zeroed) one set would skip each other's chunks.
No torch in this process: the streams come from the HIP runtime libhjbdp.so has mapped, the buffers from hjb_device_malloc."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROUNDS = 3


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi, c_oracle


class _Hip:
    """hipStreamCreateWithFlags / hipStreamSynchronize / hipStreamDestroy and timing events from the libamdhip64 that
    libhjbdp.so already has mapped (found in /proc/self/maps: the same runtime instance, never a second copy)."""

    def __init__(self):
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64.so" in line:
                    path = line.split()[-1]
                    break
        assert path, "libamdhip64 is not mapped (libhjbdp.so not loaded?)"
        self.lib = lib = C.CDLL(path)
        for name, args in (("hipStreamCreateWithFlags", [C.POINTER(C.c_void_p), C.c_uint]),
                           ("hipStreamSynchronize", [C.c_void_p]), ("hipStreamDestroy", [C.c_void_p]),
                           ("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                           ("hipEventSynchronize", [C.c_void_p]), ("hipEventDestroy", [C.c_void_p]),
                           ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p])):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, C.c_int

    def _ok(self, e, what):
        assert e == 0, "%s returned hipError %d" % (what, e)

    def stream(self):
        s = C.c_void_p()
        self._ok(self.lib.hipStreamCreateWithFlags(C.byref(s), 1), "hipStreamCreateWithFlags")      # hipStreamNonBlocking
        return s.value

    def sync(self, s):
        self._ok(self.lib.hipStreamSynchronize(s), "hipStreamSynchronize")

    def destroy(self, s):
        self._ok(self.lib.hipStreamDestroy(s), "hipStreamDestroy")

    def event(self):
        e = C.c_void_p()
        self._ok(self.lib.hipEventCreate(C.byref(e)), "hipEventCreate")
        return e.value

    def record(self, e, s):
        self._ok(self.lib.hipEventRecord(e, s), "hipEventRecord")

    def ms(self, a, b):
        t = C.c_float()
        self._ok(self.lib.hipEventElapsedTime(C.byref(t), a, b), "hipEventElapsedTime")
        return t.value


def _problem(kind):
    """-> (spec, variant to force or None, options to set, the packed2_mode expected or None)."""
    from problems import colsweep_problem, nested_problem, random_problem, rate_shared_problem
    from test_gpu_parity import _chain_spec, _row_problem
    import hjbdp
    if kind in ("v0", "v3", "v5"):
        return random_problem(4101, (5, 4, 3, 4, 3), (3, 3), dtype=np.float32, index_base=1), int(kind[1]), {}, None
    if kind in ("v1", "v2", "v4"):
        return nested_problem(4102, (13, 11, 9), (4, 5), dtype=np.float32, nonuniform=True, monotone="dec", spread=0.45), \
            int(kind[1]), {}, None
    if kind == "v6":
        return _row_problem((130, 5, 4), (5,), np.float32, True, 0.4), 6, {}, None
    if kind == "v7":
        return colsweep_problem(4107, (70, 9, 8, 11), nU=9), 7, {}, None
    if kind == "k3_mode4":
        return _chain_spec((9, 8, 7), (3, 4, 6), (0.05, 0.05, 0.10), -1.0, 1.0, lambda k: list(range(k))), 4, {}, 4
    if kind == "k3_mode5":
        return _chain_spec((20, 3, 4, 5, 4, 6), (3, 5, 5), (0.05, 0.10, 0.12), -1.0, 1.0, lambda k: list(range(k))), 4, \
            {"uniwin": 0}, 5
    if kind == "k15_mode7":      # 4.1M states x 1331 controls: a chunk walk long enough for the two launches to overlap
        return rate_shared_problem(4115, (40, 36, 36), (4, 4, 5)), None, {"uniwin": 1}, 7
    if kind in ("k15_mode8", "k15_attitude"):      # the attitude model evaluated on the fly (HJB_MODEL_QUAT_EULER321)
        sa = hjbdp.Solver_attitude(n_mesh_w=6, n_mesh_q=8) if kind == "k15_mode8" else hjbdp.Solver_attitude(n_mesh_w=10, n_mesh_q=14)
        sa.U_vector = np.linspace(-0.11, 0.11, 11)
        return sa.build_spec_model(), None, {"uniwin": 1}, 8
    raise ValueError(kind)


def _open(hjbdp, kind):
    spec, variant, opts, mode = _problem(kind)
    bk = hjbdp.Backup(spec, variant=variant)
    for k, v in opts.items():
        bk.set_option(k, v)
    if variant is not None:
        assert bk.info()["kernel_variant"] == variant
    if mode is not None:
        assert bk.info()["kernel_variant"] == 4 and bk.get_option("packed2_mode") == mode
    return spec, bk


def _buffers(hjbdp, bk, spec, inputs):
    """Device input / NaN-prefilled output / 0xff-prefilled label buffers, one triple per input."""
    inf = bk.info()
    jd, idt = np.dtype(spec.j_dtype), np.dtype(spec.idx_np_dtype)
    out = []
    for J in inputs:
        dIn = hjbdp.DeviceBuffer(J.nbytes)
        dIn.upload(J)
        dOut = hjbdp.DeviceBuffer(inf["j_elems"] * jd.itemsize)
        dOut.upload(np.full(inf["j_elems"], np.nan, dtype=jd))
        dI = hjbdp.DeviceBuffer(inf["n_states"] * idt.itemsize)
        dI.upload(np.full(inf["n_states"] * idt.itemsize, 0xff, dtype=np.uint8))
        out.append((dIn, dOut, dI))
    return out


def _check_outputs(bk, spec, inputs, bufs, what):
    for r, (J, (dIn, dOut, dI)) in enumerate(zip(inputs, bufs)):
        Jr, ir = bk.backup_stage(J)                        # the same handle, alone on the null stream
        Jg, ig = dOut.download(spec.j_dtype), dI.download(spec.idx_np_dtype)
        bad = np.flatnonzero(~(Jg == Jr))
        assert bad.size == 0, (what, r, "J", bad.size, bad[:8], Jg[bad[:4]], Jr[bad[:4]])
        bad = np.flatnonzero(ig != ir)
        assert bad.size == 0, (what, r, "labels", bad.size, bad[:8])


def _inputs(spec, seed, count):
    rng = np.random.default_rng(seed)
    return [(rng.random(spec.nS) * (1.0 + k)).astype(spec.j_dtype) for k in range(count)]


KINDS = ["v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "k3_mode4", "k3_mode5", "k15_mode7", "k15_mode8"]


@pytest.mark.order(8)
@pytest.mark.parametrize("kind", KINDS)
def test_one_handle_two_streams(env, kind):
    """ROUNDS x (stage on stream A; stage on stream B) with distinct inputs and no host synchronisation in between: every
    output equals the handle's own single-stage result for its input, bit for bit, labels included."""
    hjbdp, _abi, c_oracle = env
    hip = _Hip()
    spec, bk = _open(hjbdp, kind)
    sA, sB = hip.stream(), hip.stream()
    try:
        ins = _inputs(spec, 77 + len(kind), 2 * ROUNDS)
        bufs = _buffers(hjbdp, bk, spec, ins)
        ev = [hip.event() for _ in range(4 * ROUNDS)]
        for r in range(ROUNDS):
            for k, s in enumerate((sA, sB)):
                dIn, dOut, dI = bufs[2 * r + k]
                hip.record(ev[4 * r + 2 * k], s)
                bk.backup_stage_device(dIn, dOut, dI, stream=s)
                hip.record(ev[4 * r + 2 * k + 1], s)
        hip.sync(sA)
        hip.sync(sB)
        bk.check_device_status(stream=sA)
        bk.check_device_status(stream=sB)
        # did the two streams' stages overlap at all?  (reported, not asserted: the device decides)
        t = [hip.ms(ev[0], e) for e in ev]
        over = sum(1 for r in range(ROUNDS) for q in range(ROUNDS)
                   if min(t[4 * r + 1], t[4 * q + 3]) > max(t[4 * r], t[4 * q + 2]))
        print("\n[streams] %s: variant %d, %d of %d A/B stage pairs overlap in time; A/B stage %.3f / %.3f ms"
              % (kind, bk.info()["kernel_variant"], over, ROUNDS * ROUNDS, t[1] - t[0], t[3] - t[2]))
        for e in ev:
            hip.lib.hipEventDestroy(e)
        _check_outputs(bk, spec, ins, bufs, kind)
        if kind == "v0":           # the plain kernel against the oracle as well: the single-stage reference is itself checked
            Jo, io = c_oracle.backup_stage(_abi, spec, ins[0])
            assert np.array_equal(bufs[0][1].download(spec.j_dtype), Jo)
            assert np.array_equal(bufs[0][2].download(spec.idx_np_dtype), io)
        for b in bufs:
            for d in b:
                d.free()
    finally:
        hip.destroy(sA)
        hip.destroy(sB)
        bk.close()


@pytest.mark.order(8)
@pytest.mark.parametrize("kind", ["k15_mode7", "k15_attitude", "v7"])
def test_graph_solve_beside_a_second_stream(env, kind):
    """A graph-replayed hjb_solve on the handle's own stream while device-entry stages of the SAME handle are in flight on a
    second stream (enqueued first, not waited for): the solve equals a solve alone, every stage on the second stream equals
    the handle's own single-stage result."""
    hjbdp, _abi, c_oracle = env
    hip = _Hip()
    spec, bk = _open(hjbdp, kind)
    sB = hip.stream()
    try:
        term = _inputs(spec, 5, 1)[0]
        n = 64                                               # 2 x kGraphStages: the stage loop is captured and replayed
        alone = bk.solve(n, terminal=term)
        ins = _inputs(spec, 911, 2 * ROUNDS)
        bufs = _buffers(hjbdp, bk, spec, ins)
        for dIn, dOut, dI in bufs:
            bk.backup_stage_device(dIn, dOut, dI, stream=sB)
        both = bk.solve(n, terminal=term)
        hip.sync(sB)
        bk.check_device_status(stream=sB)
        assert np.array_equal(both["J"], alone["J"]) and np.array_equal(both["idx"], alone["idx"])
        # (the random rate-shared problem's sweep leaves float32's range within 64 stages on most states; the attitude model's
        # and the column sweep's stay finite everywhere)
        assert np.isfinite(alone["J"]).all() if kind != "k15_mode7" else np.isfinite(alone["J"]).any()
        print("\n[streams] %s: graph solve beside stream B, %.1f %% of J finite after %d stages"
              % (kind, 100.0 * np.isfinite(alone["J"]).mean(), n))
        _check_outputs(bk, spec, ins, bufs, kind)
        for b in bufs:
            for d in b:
                d.free()
    finally:
        hip.destroy(sB)
        bk.close()


@pytest.mark.order(8)
def test_k15_more_streams_than_counter_sets(env):
    """K15 on ten streams of one handle at once: the first eight (the null stream of the reference backups included) get claim
    counter sets of their own, the rest take the chunk walk's static form - every output equals the single-stage result."""
    hjbdp, _abi, c_oracle = env
    hip = _Hip()
    spec, bk = _open(hjbdp, "k15_mode7")
    streams = [hip.stream() for _ in range(10)]
    try:
        ins = _inputs(spec, 1010, len(streams))
        bufs = _buffers(hjbdp, bk, spec, ins)
        for (dIn, dOut, dI), s in zip(bufs, streams):
            bk.backup_stage_device(dIn, dOut, dI, stream=s)
        for s in streams:
            hip.sync(s)
            bk.check_device_status(stream=s)
        _check_outputs(bk, spec, ins, bufs, "ten streams")
        for b in bufs:
            for d in b:
                d.free()
    finally:
        for s in streams:
            hip.destroy(s)
        bk.close()
