"""CPU tests of how hjbdp.Rollout's four campaign methods hand their arguments to the library's five campaign entry points: a
Rollout built without __init__ on a recording stand-in for the library, every argument checked by value or by dtype, shape,
contiguity and content, every returned dict by its keys.  Beside them the planes Dynamic_Solver's campaign methods choose
(_stage_planes, and through the methods that use it).  No library, no GPU."""
import ctypes as C

import numpy as np
import pytest

D, NU, NS, K, M = 2, 1, 3, 4, 5
SEED, FIRST = 2 ** 64 + 7, 11
X0 = np.array([[0.5, -1.0, 2.0], [0.25, 0.0, -0.75]])                          # [D, n_starts]
THR, TOL = 1.5, [0.1, 0.2]                                                      # a scalar threshold, a per-axis tol
HIST = (-1.0, [2.0, 3.0, 4.0], 6)                                               # lo a scalar, hi per start, n_bins
PLANES, VPLANES = [0, 1, 1, 0], np.array([1, 2, 2, 1], dtype=np.int64)
CAMPAIGN_KEYS = {"stats", "mean", "var", "std", "min", "max", "n_exceed", "n_left", "n_settled", "mean_settled"}
HIST_KEYS = {"hist", "hist_lo", "hist_hi"}
PAIR_KEYS = {"a", "b", "stats_d", "mean_diff", "var_diff", "std_diff", "se_diff", "t", "min_diff", "max_diff", "n_b_lower", "n_a_lower",
             "n_tie", "n_both_in", "mean_diff_both_in"}


def _arr(ptr):
    """the numpy array a pointer made by ndarray.ctypes.data_as keeps alive"""
    return ptr._arr


class FakeLib:
    """Records every call as (name, args); a campaign entry point also writes its outputs: record r of a call as r + 1 + 0.125 *
    (the element's flat index), the counts as their flat index, the time as 1.5 ms."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            from hjbdp import _abi
            self.calls.append((name, args))
            if "campaign" in name:
                types = _abi.SYMBOLS[name][1]
                outs = [a for a, t in zip(args[:-1], types) if t == C.POINTER(C.c_double) and a is not None and _arr(a).shape == (NS, 8)]
                for r, a in enumerate(outs):
                    _arr(a)[...] = r + 1 + 0.125 * np.arange(NS * 8).reshape(NS, 8)
                for a, t in zip(args, types):
                    if t == C.POINTER(C.c_int64):
                        _arr(a)[...] = np.arange(_arr(a).size).reshape(_arr(a).shape)
                args[-1]._obj.value = 1.5
            return 0
        return fn


@pytest.fixture
def ro():
    import hjbdp
    r = object.__new__(hjbdp.Rollout)
    r.lib, r._ro = FakeLib(), C.c_void_p(0x1234)
    r.D, r.n_u, r.n = D, NU, [3, 3]
    yield r
    r._ro = C.c_void_p()                                                        # nothing to destroy


def _is_array(a, dtype, want):
    arr = _arr(a)
    want = np.asarray(want, dtype=dtype)
    assert arr.dtype == dtype and arr.shape == want.shape and arr.flags.c_contiguous, (arr.dtype, arr.shape, arr.flags)
    assert np.array_equal(arr, want), (arr, want)
    assert a._type_ is {np.float64: C.c_double, np.int32: C.c_int32, np.int64: C.c_int64}[dtype]


def _check_call(ro, name, lead, n_lead_arrays, hist, n_records):
    """The one call the method made: its name, its arity, then - behind the handle and the `lead` the method owns (scalars by value,
    arrays as (dtype, content)) - what every campaign call carries."""
    from hjbdp import _abi
    (called, args), = ro.lib.calls
    assert called == name
    assert len(args) == len(_abi.SYMBOLS[name][1]), (name, len(args))
    assert args[0] is ro._ro
    at = 1
    for want in lead:
        if isinstance(want, tuple):
            _is_array(args[at], *want)
        else:
            assert type(args[at]) is int and args[at] == want, (name, at, args[at], want)
        at += 1
    assert n_lead_arrays == sum(isinstance(w, tuple) for w in lead)
    ns, m, x, seed, first, thr, tol = args[at:at + 7]
    assert (type(ns), ns, type(m), m) == (int, NS, int, M)
    _is_array(x, np.float64, X0.T)                                              # [n_starts, D] C order = [D, n_starts] column-major
    assert (type(seed), seed, type(first), first) == (int, 7, int, FIRST)       # the seed masked to 64 bits
    _is_array(thr, np.float64, [THR] * NS)                                      # the scalar broadcast to the starts
    _is_array(tol, np.float64, TOL)
    at += 7
    if hist:
        lo, hi, nb = args[at:at + 3]
        _is_array(lo, np.float64, [-1.0] * NS)
        _is_array(hi, np.float64, HIST[1])
        assert type(nb) is int and nb == 6
        at += 3
    for r in range(n_records):
        _is_array(args[at], np.float64, r + 1 + 0.125 * np.arange(NS * 8).reshape(NS, 8))      # as the stand-in wrote it
        at += 1
    if hist:
        _is_array(args[at], np.int64, np.arange(NS * 8).reshape(NS, 8))                          # [n_starts, n_bins + 2]
        at += 1
    assert at == len(args) - 1 and isinstance(args[at]._obj, C.c_double)
    return args


def _check_record(out, r):
    assert np.array_equal(out["stats"], r + 1 + 0.125 * np.arange(NS * 8).reshape(NS, 8))
    assert np.array_equal(out["mean"], out["stats"][:, 0] / M) and out["n_exceed"].dtype == np.int64


def test_run_campaign(ro):
    from hjbdp import _abi
    out = ro.run_campaign(X0, PLANES, M, seed=SEED, first_stream=FIRST, method="nearest", cost_threshold=THR, settle_tol=TOL)
    _check_call(ro, "hjb_rollout_run_campaign", [_abi.HJB_LOOKUP_NEAREST, K, (np.int32, PLANES)], 1, False, 1)
    assert set(out) == CAMPAIGN_KEYS | {"device_ms"} and out["device_ms"] == 1.5
    _check_record(out, 0)


def test_run_campaign_with_a_histogram(ro):
    from hjbdp import _abi
    out = ro.run_campaign(X0, PLANES, M, seed=SEED, first_stream=FIRST, cost_threshold=THR, settle_tol=TOL, hist=HIST)
    _check_call(ro, "hjb_rollout_run_campaign_hist", [_abi.HJB_LOOKUP_LINEAR, K, (np.int32, PLANES)], 1, True, 1)
    assert set(out) == CAMPAIGN_KEYS | HIST_KEYS | {"device_ms"} and out["device_ms"] == 1.5
    _check_record(out, 0)
    assert out["hist"].dtype == np.int64 and np.array_equal(out["hist"], np.arange(NS * 8).reshape(NS, 8))
    assert out["hist_lo"].tolist() == [-1.0] * NS and out["hist_hi"].tolist() == HIST[1]


def test_run_lookahead_campaign(ro):
    out = ro.run_lookahead_campaign(X0, VPLANES, M, seed=SEED, first_stream=FIRST, cost_threshold=THR, settle_tol=TOL)
    _check_call(ro, "hjb_rollout_run_lookahead_campaign", [K, (np.int32, VPLANES)], 1, False, 1)
    assert set(out) == CAMPAIGN_KEYS | {"device_ms"} and out["device_ms"] == 1.5
    _check_record(out, 0)


def test_run_lookahead_campaign_hist(ro):
    out = ro.run_lookahead_campaign_hist(X0, VPLANES, M, HIST, seed=SEED, first_stream=FIRST, cost_threshold=THR, settle_tol=TOL)
    _check_call(ro, "hjb_rollout_run_lookahead_campaign_hist", [K, (np.int32, VPLANES)], 1, True, 1)
    assert set(out) == CAMPAIGN_KEYS | HIST_KEYS | {"device_ms"} and out["device_ms"] == 1.5
    _check_record(out, 0)
    assert out["hist"].dtype == np.int64 and np.array_equal(out["hist"], np.arange(NS * 8).reshape(NS, 8))


def test_run_campaign_pair(ro):
    from hjbdp import _abi
    out = ro.run_campaign_pair(X0, ("labels", PLANES, "nearest"), ("greedy", VPLANES), M, seed=SEED, first_stream=FIRST, cost_threshold=THR,
                               settle_tol=TOL)
    _check_call(ro, "hjb_rollout_run_campaign_pair", [_abi.HJB_PAIR_LABELS, _abi.HJB_LOOKUP_NEAREST, (np.int32, PLANES), _abi.HJB_PAIR_GREEDY, 0,
                                                      (np.int32, VPLANES), K], 2, False, 3)
    assert set(out) == PAIR_KEYS | {"device_ms"} and out["device_ms"] == 1.5
    assert set(out["a"]) == set(out["b"]) == CAMPAIGN_KEYS
    _check_record(out["a"], 0)
    _check_record(out["b"], 1)
    assert np.array_equal(out["stats_d"], 3 + 0.125 * np.arange(NS * 8).reshape(NS, 8))
    assert np.array_equal(out["mean_diff"], out["stats_d"][:, 0] / M)
    with pytest.raises(ValueError, match="a and b: 4 and 3 steps"):
        ro.run_campaign_pair(X0, ("labels", PLANES), ("lookahead", [1, 2, 3]), M)


def test_no_bounds_are_null_pointers(ro):
    ro.run_lookahead_campaign(X0, VPLANES, M)
    (_, args), = ro.lib.calls
    assert args[6] == 0 and args[7] == 0 and args[8] is None and args[9] is None        # seed, first_stream, threshold, tol


# ---- the planes Dynamic_Solver's campaign methods hand over ---------------------------------------------------------------------
BAD_PLANES = ((dict(mode="ssu", ssu_num=0), r"ssu_num must lie in 1\.\.N-1 = 3"), (dict(mode="ssu", ssu_num=4), r"ssu_num must lie in 1\.\.N-1 = 3"),
              (dict(mode="both"), "mode must be 'Nssu' or 'ssu'"))


def test_stage_planes():
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N = 4
    for values, free, frozen in ((False, [0, 1, 2], [1, 1, 1]), (True, [1, 2, 3], [2, 2, 2])):
        for got, want in ((ds._stage_planes("Nssu", 2, values), free), (ds._stage_planes("ssu", 2, values), frozen)):
            assert got.dtype == np.int32 and got.tolist() == want, (values, got)
        for kw, text in BAD_PLANES:
            with pytest.raises(ValueError, match=text):
                ds._stage_planes(kw["mode"], kw.get("ssu_num", 1), values)


def test_the_planes_the_campaign_methods_fly(monkeypatch):
    """the same planes and the same three refusals, through the public methods (N = 3: two steps)"""
    import solver_recorder as rec
    planes = lambda calls, name: [args[1] for n, args, _ in calls if n == name][0]
    for kw, labels, values in ((dict(), [0, 1], [1, 2]), (dict(mode="ssu", ssu_num=2), [1, 1], [2, 2])):
        _, calls = rec.record(monkeypatch, "get_noisy_cost_statistics", np.zeros((2, 1)), 4, **kw)
        assert planes(calls, "run_campaign").dtype == np.int32 and planes(calls, "run_campaign").tolist() == labels
        _, calls = rec.record(monkeypatch, "get_lookahead_cost_statistics", np.zeros((2, 1)), 4, **kw)
        assert planes(calls, "run_lookahead_campaign").dtype == np.int32 and planes(calls, "run_lookahead_campaign").tolist() == values
        _, calls = rec.record(monkeypatch, "get_paired_cost_statistics", np.zeros((2, 1)), 4, a="labels", b="disturbed", **kw)
        (_, a, b, _), = [args for n, args, _ in calls if n == "run_campaign_pair"]
        assert a[1].tolist() == labels and b[1].tolist() == values
    for method in ("get_noisy_cost_statistics", "get_lookahead_cost_statistics", "get_paired_cost_statistics", "get_noisy_cost_quantiles",
                   "get_lookahead_cost_quantiles"):
        for kw, text in BAD_PLANES:
            text = text.replace("= 3", "= 2")
            with pytest.raises(ValueError, match=text):
                rec.record(monkeypatch, method, np.zeros((2, 1)), 4, **kw)
            assert rec.RecordingRollout.calls == []                             # refused before an object is opened
