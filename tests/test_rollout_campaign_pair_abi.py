"""CPU tests of the paired campaign's ABI (include/hjbdp.h "paired campaigns"): the two prototypes in both headers and in the
ctypes table, the constants, the contract's wording, the refusals that need no object, the Python faces and the MATLAB shim's call
sequence and arities.  No GPU."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
RUN, REDUCE = "hjb_rollout_run_campaign_pair", "hjb_rollout_campaign_pair_reduce"
PAIR_FNS = {RUN: 19, REDUCE: 7}
PKG = ROOT / "optimal-control-dynamic-programming_amd"
SHIM = PKG / "matlab" / "Dynamic_Solver_hjbdp_paired_cost_map.m"


@pytest.fixture(scope="module")
def lib(built):
    import hjbdp
    return hjbdp.load_library()


def test_prototypes_are_identical_in_both_headers_and_the_ctypes_table(lib):
    from hjbdp import _abi
    from test_abi import _prototypes
    full = _prototypes((ROOT / "include" / "hjbdp.h").read_text())
    flat = _prototypes((ROOT / "include" / "hjbdp_matlab.h").read_text())
    for name, arity in PAIR_FNS.items():
        assert name in full and name in flat, name
        assert full[name] == flat[name], (name, full[name], flat[name])
        assert len(full[name]) == arity, (name, full[name])
        assert hasattr(lib, name), name
        res, args = _abi.SYMBOLS[name]
        assert res is C.c_int32 and len(args) == arity, name
    side = ["int32_t", "int32_t", "int32_t*"]                                   # kind, method, planes
    plain = full["hjb_rollout_run_campaign"]                                    # ... n_starts, n_samples, X0, seed, first, thr, tol, stats, ms
    assert full[RUN] == ["void*"] + side + side + ["int32_t"] + plain[4:11] + ["double*"] * 3 + plain[12:]
    assert full[REDUCE] == ["int64_t", "int64_t", "double*", "double*", "uint8_t*", "uint8_t*", "double*"]
    mine, theirs = _abi.SYMBOLS[RUN][1], _abi.SYMBOLS["hjb_rollout_run_campaign"][1]
    assert mine[0] is C.c_void_p and mine[1:4] == mine[4:7] == [C.c_int32, C.c_int32, C.POINTER(C.c_int32)] and mine[7] is C.c_int32
    assert mine[8:15] == theirs[4:11] and mine[15:] == [C.POINTER(C.c_double)] * 4
    assert _abi.SYMBOLS[REDUCE][1][4:6] == [C.POINTER(C.c_uint8)] * 2


def test_the_constants_and_the_contract_are_stated(lib):
    from hjbdp import _abi
    text = (ROOT / "include" / "hjbdp.h").read_text()
    for name, value in (("HJB_PAIR_LABELS", 0), ("HJB_PAIR_LOOKAHEAD", 1), ("HJB_PAIR_GREEDY", 2), ("HJB_CAMPAIGN_PAIR_NSTAT", 8)):
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, text, flags=re.M)
        assert m and int(m.group(1)) == getattr(_abi, name) == value, name
    assert text.index("---- campaign cost histograms") < text.index("---- paired campaigns")       # below K30
    sect = " ".join(text[text.index("---- paired campaigns"):text.index("#define HJB_PAIR_LABELS")].replace("\n *", " ").split())
    for word in ("first_stream + s*M + m", "d = c_B - c_A", "one rounded subtraction per sample", "A negative d means B paid less",
                 "e = d < 0", "l = d > 0", "t = neither flight left the grid", "A NaN d sets neither e nor l", "campaign_slot(d, t)",
                 "word for word", "CampVals, campaign_op, campaign_tree", "there is no second reduction", "0 sum d", "1 sum d*d, each product rounded",
                 "4 n(B lower)", "5 n(A lower)", "6 n(both stayed in the grid)", "7 sum d over those samples",
                 "Counts are exact integers stored as doubles", "There are no atomics anywhere in this call",
                 'Options "chunk" and "lds" change no bit of any of the three records', "[D + 1 + 24, n_starts] doubles",
                 "24 doubles per block of a launch", "one double and one byte per lane of a launch", "No array of the call has a dimension of n_starts * M",
                 "ONE zero node of weight 1", "neither read nor changed", "a pair of a controller with itself is legal",
                 'a NULL left_* means "none left"', "a kind outside 0..2", '("A:" / "B:")', "n_starts = 0 is HJB_OK",
                 "Out of scope: a histogram of d, pairs across two objects, pairs on the integrated plants"):
        assert word in sect, word
    assert "Out of scope: a paired-difference statistic" not in text
    k29 = text[text.index("---- lookahead campaigns"):text.index("int32_t hjb_rollout_run_lookahead_campaign(")]
    assert RUN in k29
    design = (ROOT / "DESIGN.md").read_text()
    assert "K31" in design and "a histogram of `d`" in design
    shared = (PKG / "csrc" / "hjbdp_campaign.h").read_text()
    assert "campaign_pair_start" in shared and "campaign_pair_diff" in shared and "hip_runtime" not in shared
    host = (PKG / "csrc" / "rollout_host.h").read_text()
    assert "own_set" in host
    for unit in ("rollout_campaign_pair.hip", "rollout_lookahead_campaign_pair.hip", "rollout_campaign_pair_host.hip",
                 "kernels_rollout_campaign_pair.h", "kernels_rollout_lookahead_campaign_pair.h"):
        assert (PKG / "csrc" / unit).exists(), unit
    for unit in ("kernels_rollout_campaign_pair.h", "kernels_rollout_lookahead_campaign_pair.h", "rollout_campaign_pair_host.hip"):
        assert "atomic" not in (PKG / "csrc" / unit).read_text().replace("No atomics", ""), unit


def test_refusals_that_need_no_object(lib):
    """sizes, streams, kinds and the null handle are refused before an object is needed; the outputs stay untouched"""
    from hjbdp import _abi
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = [np.full(32, 7.25) for _ in range(3)]
    X = np.zeros(8)
    ms = C.c_double(7.25)
    for ka, kb, n_samples, first, word in ((0, 1, 1, 0, "null handle"), (0, 1, 0, 0, "n_samples=0"), (0, 1, 1, -1, "first_stream=-1"),
                                           (0, 1, 2 ** 62, 0, "overflows"), (3, 1, 1, 0, "A: kind 3"), (-1, 1, 1, 0, "A: kind -1"),
                                           (0, 3, 1, 0, "B: kind 3"), (2, -7, 1, 0, "B: kind -7")):
        st = lib.hjb_rollout_run_campaign_pair(None, ka, 1, None, kb, 0, None, 0, 4, n_samples, dp(X), 0, first, None, None, dp(out[0]), dp(out[1]),
                                               dp(out[2]), C.byref(ms))
        assert st == _abi.HJB_E_INVALID, (ka, kb, n_samples, first)
        assert word in lib.hjb_rollout_last_error(None).decode(), (word, lib.hjb_rollout_last_error(None).decode())
    assert all(np.all(o == 7.25) for o in out) and ms.value == 7.25
    assert lib.hjb_rollout_campaign_pair_reduce(1, 0, dp(X), dp(X), None, None, dp(out[0])) == _abi.HJB_E_INVALID
    assert lib.hjb_rollout_campaign_pair_reduce(-1, 1, dp(X), dp(X), None, None, dp(out[0])) == _abi.HJB_E_INVALID
    assert lib.hjb_rollout_campaign_pair_reduce(1, 1, None, dp(X), None, None, dp(out[0])) == _abi.HJB_E_INVALID
    assert np.all(out[0] == 7.25)


def test_python_faces_exist():
    import hjbdp
    assert callable(hjbdp.campaign_pair_reduce) and "campaign_pair_reduce" in hjbdp.__all__
    assert list(inspect.signature(hjbdp.campaign_pair_reduce).parameters) == ["cost_a", "cost_b", "n_samples", "left_a", "left_b"]
    sig = inspect.signature(hjbdp.Rollout.run_campaign_pair)
    assert list(sig.parameters) == ["self", "X0", "a", "b", "n_samples", "seed", "first_stream", "cost_threshold", "settle_tol"]
    ds = hjbdp.Dynamic_Solver
    sig = inspect.signature(ds.get_paired_cost_statistics)
    assert list(sig.parameters)[:9] == ["self", "X0s", "n_samples", "a", "b", "seed", "mode", "ssu_num", "method"]
    assert sig.parameters["a"].default == "labels" and sig.parameters["b"].default == "disturbed"
    assert list(inspect.signature(ds.paired_cost_map).parameters)[:4] == ["self", "n_samples", "a", "b"]
    out = hjbdp.campaign_pair_reduce([1.0, 3.0], [2.0, 1.0], 2)
    for key in ("a", "b", "stats_d", "mean_diff", "var_diff", "std_diff", "se_diff", "t", "min_diff", "max_diff", "n_b_lower", "n_a_lower",
                "n_tie", "n_both_in", "mean_diff_both_in", "device_ms"):
        assert key in out, key
    assert out["stats_d"].tolist() == [[-1.0, 5.0, -2.0, 1.0, 1.0, 1.0, 2.0, -1.0]]
    d = hjbdp.Dynamic_Solver(precision="double")
    with pytest.raises(RuntimeError):
        d.paired_cost_map(4)                                                    # run() first


def test_matlab_shim_call_sequence(monkeypatch):
    """the shim drives the entry points Dynamic_Solver.paired_cost_map drives, in its order, each with the flat header's arity"""
    import solver_recorder as rec
    from test_abi import _matlab_calllibs, _prototypes
    flat = _prototypes((ROOT / "include" / "hjbdp_matlab.h").read_text())
    text = SHIM.read_text()
    calls = _matlab_calllibs(text)
    names = [n for n, _ in calls]
    body = [n for n in names if n not in ("hjb_rollout_last_error", "hjb_status_string")]
    assert body == ["hjb_rollout_create", "hjb_rollout_destroy", "hjb_rollout_set_model", "hjb_rollout_set_values", "hjb_rollout_set_lookahead",
                    "hjb_rollout_set_noise", RUN], body
    for name, nargs in calls:
        assert nargs == len(flat[name]), (name, nargs, flat[name])
    assert "hjb_rollout_run_noisy" not in names and "hjb_rollout_run_lookahead'" not in text     # no per-trajectory array on the MATLAB side
    assert text.count("zeros(8, ns)") == 3 and "tested twin: hjbdp/dynamic_solver.py paired_cost_map" in text
    assert "matlab/Dynamic_Solver_hjbdp_paired_cost_map.m" in (ROOT / "include" / "hjbdp_matlab.h").read_text()
    assert "Dynamic_Solver_hjbdp_paired_cost_map.m" in (ROOT / "INTEGRATION.md").read_text()
    # the twin, by the calls it makes on the object it opens: the shim's, in the shim's order, and never a per-trajectory run
    out, calls = rec.record(monkeypatch, "paired_cost_map", 4, a="labels", b="nominal")
    assert rec.as_entry_points(calls) == rec.shim_order(body), calls
    assert not {"run_noisy", "run_lookahead"} & {name for name, _, _ in calls}
    assert out["stats_d"].shape == (3, 3, 8) and out["a"]["stats"].shape == (3, 3, 8) and out["b"]["mean"].shape == (3, 3)
    (X0, a, b, n_samples), = [args for name, args, _ in calls if name == "run_campaign_pair"]
    assert a[0] == "labels" and a[1].tolist() == [0, 1] and b[0] == "greedy" and b[1].tolist() == [1, 2] and n_samples == 4
