"""CPU tests of the lookahead campaign's ABI (include/hjbdp.h "lookahead campaigns"): the prototypes in both headers and in the
ctypes table, the contract's wording, the Python faces, and the MATLAB shim's call sequence and arities.  No GPU."""
import ctypes as C
import inspect
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
RUN, TWIN = "hjb_rollout_run_lookahead_campaign", "hjb_rollout_lookahead_campaign_host"
SHIM = ROOT / "optimal-control-dynamic-programming_amd" / "matlab" / "Dynamic_Solver_hjbdp_lookahead_cost_map.m"


@pytest.fixture(scope="module")
def lib(built):
    import hjbdp
    return hjbdp.load_library()


def test_prototypes_are_identical_in_both_headers_and_the_ctypes_table(lib):
    from hjbdp import _abi
    from test_abi import _prototypes
    full = _prototypes((ROOT / "include" / "hjbdp.h").read_text())
    flat = _prototypes((ROOT / "include" / "hjbdp_matlab.h").read_text())
    assert RUN in full and RUN in flat and full[RUN] == flat[RUN]
    assert TWIN in full and TWIN not in flat                                    # the twin is not part of the MATLAB face, as its kin
    for name, arity in ((RUN, 12), (TWIN, 31)):
        assert len(full[name]) == arity, (name, full[name])
        assert hasattr(lib, name), name
        res, args = _abi.SYMBOLS[name]
        assert res is C.c_int32 and len(args) == arity, name
    # hjb_rollout_run_campaign's arguments without the method
    camp = full["hjb_rollout_run_campaign"]
    assert full[RUN] == camp[:1] + camp[2:]
    assert full[RUN] == ["void*", "int32_t", "int32_t*", "int64_t", "int64_t", "double*", "uint64_t", "int64_t", "double*", "double*",
                         "double*", "double*"]
    run = _abi.SYMBOLS[RUN][1]
    assert run[0] is C.c_void_p and run[3] is C.c_int64 and run[4] is C.c_int64 and run[6] is C.c_uint64 and run[7] is C.c_int64
    # the twin: hjb_rollout_lookahead_host's problem (16) and lookahead set (4), the flight set (3), the campaign (8)
    host = full["hjb_rollout_lookahead_host"]
    assert full[TWIN][:16] == host[:16] and full[TWIN][16:20] == host[24:28]
    assert full[TWIN][20:23] == ["int32_t", "double*", "double*"]
    assert full[TWIN][23:] == full[RUN][3:11]
    twin = _abi.SYMBOLS[TWIN][1]
    assert twin[:16] == _abi.SYMBOLS["hjb_rollout_lookahead_host"][1][:16]
    assert twin[23:] == run[3:11]


def test_the_contract_is_stated_in_the_header():
    text = (ROOT / "include" / "hjbdp.h").read_text()
    sect = text[text.index("---- lookahead campaigns"):text.index("int32_t " + RUN)]
    for word in ("first_stream + s*M + m", "fly_noise = 1", "Common random numbers", "hjb_rollout_run_campaign's (above), word for word",
                 "after the noise", 'Options "chunk" and "lds" change no bit', "[D + 1 + 8, n_starts]", "a start's blocks may straddle launches",
                 "one\n * zero lookahead node of weight 1", "no nominal-plant form", "It never holds more than one start's samples",
                 "n_starts = 0 is HJB_OK", "paired-difference", "float16 value planes"):
        assert word in sect, word
    k28 = text[text.index("---- noisy campaigns"):text.index("#define HJB_CAMPAIGN_NSTAT")]
    assert "campaigns of the greedy / lookahead controllers" not in k28 and RUN in k28
    assert "quantiles" in k28 and "campaigns of the integrated plants" in k28
    flat = (ROOT / "include" / "hjbdp_matlab.h").read_text()
    assert "matlab/Dynamic_Solver_hjbdp_lookahead_cost_map.m" in flat and SHIM.exists()


def test_python_faces_exist():
    import hjbdp
    assert callable(hjbdp.lookahead_campaign_host) and "lookahead_campaign_host" in hjbdp.__all__
    assert callable(hjbdp.Rollout.run_lookahead_campaign)
    sig = inspect.signature(hjbdp.Rollout.run_lookahead_campaign)
    assert list(sig.parameters) == ["self", "X0", "value_plane_of_step", "n_samples", "seed", "first_stream", "cost_threshold", "settle_tol"]
    ds = hjbdp.Dynamic_Solver
    sig = inspect.signature(ds.get_lookahead_cost_statistics)
    assert list(sig.parameters) == ["self", "X0s", "n_samples", "seed", "mode", "ssu_num", "lookahead", "cost_threshold", "settle_tol"]
    assert sig.parameters["lookahead"].default == "disturbed" and callable(ds.lookahead_cost_map)
    for fn in (ds.get_lookahead_cost_statistics, ds.lookahead_cost_map):          # the docstrings say what the streams pair with
        doc = " ".join(fn.__doc__.split())
        assert "streams pair with" in doc and "noisy_cost_map" in doc and "common random numbers" in doc
    assert "common random numbers" in " ".join(hjbdp.Rollout.run_lookahead_campaign.__doc__.split())
    d = hjbdp.Dynamic_Solver(precision="double")
    with pytest.raises(RuntimeError):
        d.lookahead_cost_map(4)                                                 # run() first


def test_matlab_shim_call_sequence(monkeypatch):
    """the shim drives the entry points Dynamic_Solver.lookahead_cost_map drives, in its order, each with the flat header's arity"""
    import numpy as np
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
    assert "hjb_rollout_run_lookahead'" not in text                             # no per-trajectory array on the MATLAB side either
    assert "zeros(8, ns)" in text and "ndgrid(s_r, s_r)" in text and "tested twin: hjbdp/dynamic_solver.py lookahead_cost_map" in text
    # the twin, by the calls it makes on the object it opens: the shim's, in the shim's order, under either lookahead, and never a
    # per-trajectory run
    for lookahead in ("disturbed", "nominal"):
        out, calls = rec.record(monkeypatch, "lookahead_cost_map", 4, lookahead=lookahead)
        assert rec.as_entry_points(calls) == rec.shim_order(body), (lookahead, calls)
        assert not {"run_noisy", "run_lookahead"} & {name for name, _, _ in calls}
        assert out["stats"].shape == (3, 3, 8)
        (off, w, mode), = [args for name, args, _ in calls if name == "set_lookahead"]
        ds = rec.hand_set_solver()
        if lookahead == "disturbed":                                            # the solver's own set, in its own mode
            assert np.array_equal(off, ds.disturbance[0]) and w == ds.disturbance[1] and mode == "expect"
        else:                                                                   # one zero node of weight 1
            assert np.array_equal(off, np.zeros((2, 1))) and list(w) == [1.0] and mode == "expect"
        # ... and the two-pass quantile map: the same object, the plain campaign, then the histogram one
        out, calls = rec.record(monkeypatch, "lookahead_cost_quantile_map", 4, n_bins=5, lookahead=lookahead)
        assert rec.as_entry_points(calls) == rec.shim_order(body)[:-1] + [RUN + "_hist", "hjb_rollout_destroy"], (lookahead, calls)
        assert out["hist"].shape == (3, 3, 7) and out["quantiles"].shape == (3, 3, 3)
