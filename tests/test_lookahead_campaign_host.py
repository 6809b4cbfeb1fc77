"""CPU tests of the lookahead campaign's host twin (hjb_rollout_lookahead_campaign_host, hjbdp.lookahead_campaign_host): its
statistics equal, as bits, the chain of the entry points it is built from - noise_thresholds -> noise_draw -> lookahead_host under
the drawn nodes -> campaign_refs.left_flags -> campaign_reduce - at every D, both value types and block shapes M = 1, 5 and 65;
the seeds of the GPU test's instantiation cases exercise every statistic; the stream numbering; the refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import lookahead_campaign_refs as lc
from lookahead_campaign_refs import bits

KEYS = ("mean", "var", "std", "min", "max", "n_exceed", "n_left", "n_settled", "mean_settled")


def _twin(pb, X0, M, thr=None, tol=None, planes=lc.PLANES, seed=None, first=None):
    import hjbdp
    return hjbdp.lookahead_campaign_host(pb["knots"], pb["ut"], pb["A"], pb["B"], pb["V"], X0, planes, M, pb["E"], pb["F"], weights=pb["P"],
                                         mode=pb["mode"], flight_weights=pb["Pf"], seed=pb["seed"] if seed is None else seed,
                                         first_stream=pb["first"] if first is None else first, cost_threshold=thr, settle_tol=tol,
                                         **pb["model"])


@pytest.mark.parametrize("M", [1, 5, 65])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_host_twin_is_the_chain_of_its_parts(built, D, dtype, M):
    pb = lc.problem(D, dtype)
    X0 = pb["X0"][:, :11] if M == 65 else pb["X0"]              # 65: two blocks a start, the second almost all padding
    flown = lc.fly_chain(pb, X0, M)
    for thr, tol in ((None, None), lc.bounds_of(flown)):
        want = lc.reduce_flown(flown, M, thr, tol)
        got = _twin(pb, X0, M, thr, tol)
        assert got["stats"].shape == (X0.shape[1], 8)
        assert np.array_equal(bits(got["stats"]), bits(want["stats"])), (thr, got["stats"], want["stats"])
        for key in KEYS:
            assert np.array_equal(got[key], want[key], equal_nan=True), key


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_the_instantiation_seeds_exercise_every_statistic(built, D, dtype):
    """what tests/test_gpu_rollout_lookahead_campaign.py's first test relies on, checked here without a device: at M = 5 and 37
    starts some flight left the grid, and under the bounds taken from the flight n_exceed and n_settled are neither empty nor full"""
    pb = lc.problem(D, dtype)
    M, ns = 5, lc.N_STARTS
    flown = lc.fly_chain(pb, pb["X0"], M)
    got = _twin(pb, pb["X0"], M, *lc.bounds_of(flown))
    assert got["n_left"].sum() > 0 and got["n_left"].max() <= M
    assert 0 < got["n_exceed"].sum() < ns * M
    assert 0 < got["n_settled"].sum() < ns * M
    assert np.array_equal(got["n_settled"] == 0, np.isnan(got["mean_settled"]))


def test_streams_count_through_the_starts_and_the_seed_matters(built):
    pb = lc.problem(2, np.float64)
    M = 200                                                     # four blocks a start, the last of 8 samples
    X0 = pb["X0"][:, :14]
    whole = _twin(pb, X0, M, 0.5, 0.3)
    halves = [_twin(pb, X0[:, 7 * i:7 * i + 7], M, 0.5, 0.3, first=pb["first"] + 7 * M * i) for i in (0, 1)]
    assert np.array_equal(bits(whole["stats"]), bits(np.concatenate([h["stats"] for h in halves])))
    assert np.array_equal(bits(whole["stats"]), bits(lc.reduce_flown(lc.fly_chain(pb, X0, M), M, 0.5, 0.3)["stats"]))
    other = _twin(pb, X0, M, 0.5, 0.3, seed=pb["seed"] + 1)
    assert not np.array_equal(other["stats"][:, 0], whole["stats"][:, 0])


def test_one_zero_node_in_both_sets_is_m_copies_of_the_greedy_cost(built):
    import hjbdp
    pb = lc.problem(3, np.float32)
    zero = np.zeros((3, 1))
    zero[2, 0] = -0.0
    greedy = hjbdp.greedy_host(pb["knots"], pb["ut"], pb["A"], pb["B"], pb["V"], pb["X0"], lc.PLANES, **pb["model"])
    for M in (1, 16, 65):
        got = hjbdp.lookahead_campaign_host(pb["knots"], pb["ut"], pb["A"], pb["B"], pb["V"], pb["X0"], lc.PLANES, M, zero, zero, weights=[1.0],
                                            seed=3, **pb["model"])
        assert np.array_equal(bits(got["min"]), bits(greedy["cost"])) and np.array_equal(bits(got["max"]), bits(greedy["cost"]))
        want = hjbdp.campaign_reduce(np.repeat(greedy["cost"], M), M)
        assert np.array_equal(bits(got["stats"][:, [0, 1, 2, 3]]), bits(want["stats"][:, [0, 1, 2, 3]]))


def test_refusals_leave_the_output_untouched(built):
    import hjbdp
    from hjbdp import _abi
    lib = hjbdp.load_library()
    pb = lc.problem(2, np.float64)
    D, ns, M = 2, 5, 3
    knots = np.ascontiguousarray(np.concatenate(pb["knots"]))
    n = (C.c_int32 * 2)(*[len(k) for k in pb["knots"]])
    nl, nu = pb["ut"].shape
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    f = lambda a, order="C": np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, order=order))
    base = dict(D=D, n=n, knots=knots, nl=nl, nu=nu, ut=f(pb["ut"], "F"), A=f(pb["A"], "F"), B=f(pb["B"], "F"), dtype=_abi.HJB_F64, nv=3,
                V=np.ascontiguousarray(pb["V"].reshape(-1, order="F")), K=len(lc.PLANES), planes=np.array(lc.PLANES, dtype=np.int32), mode=0,
                W=3, E=f(pb["E"], "F"), P=f(pb["P"]) if pb["P"] is not None else None, Wf=4, F=f(pb["F"], "F"), Pf=f(pb["Pf"]), ns=ns, M=M,
                X0=f(pb["X0"][:, :ns].T), first=0, thr=None, tol=None)
    if pb["mode"] == "worst":
        base["mode"], base["P"] = 1, None
    nan_thr, neg_tol, bad_w = np.full(ns, np.nan), np.array([0.1, -1.0]), np.array([0.5, -0.5, 0.5, 0.5])
    inf_x = base["X0"].copy()
    inf_x[3] = np.inf
    far = np.array([0, 3, 0, 0, 0, 0], dtype=np.int32)

    def call(**kw):
        a = {**base, **kw}
        stats = np.full(8 * ns, 7.25)
        pl = a["planes"]
        st = lib.hjb_rollout_lookahead_campaign_host(
            a["D"], a["n"], dp(a["knots"]), a["nl"], a["nu"], dp(a["ut"]), dp(a["A"]), dp(a["B"]), None, None, None, a["dtype"], a["nv"],
            a["V"].ctypes.data, a["K"], None if pl is None else pl.ctypes.data_as(C.POINTER(C.c_int32)), a["mode"], a["W"], dp(a["E"]),
            dp(a["P"]), a["Wf"], dp(a["F"]), dp(a["Pf"]), a["ns"], a["M"], dp(a["X0"]), 4, a["first"], dp(a["thr"]), dp(a["tol"]),
            None if kw.get("no_stats") else dp(stats))
        return st, stats

    st, stats = call()
    assert st == _abi.HJB_OK and not (stats == 7.25).any()
    for kw, code in ((dict(M=0), _abi.HJB_E_INVALID), (dict(M=2 ** 62), _abi.HJB_E_INVALID), (dict(first=-1), _abi.HJB_E_INVALID),
                     (dict(first=2 ** 63 - 10), _abi.HJB_E_INVALID), (dict(ns=-1), _abi.HJB_E_INVALID), (dict(D=7), _abi.HJB_E_UNSUPPORTED),
                     (dict(W=0), _abi.HJB_E_INVALID), (dict(Wf=0), _abi.HJB_E_INVALID), (dict(F=None), _abi.HJB_E_INVALID),
                     (dict(Pf=bad_w), _abi.HJB_E_INVALID), (dict(planes=far), _abi.HJB_E_INVALID), (dict(planes=None), _abi.HJB_E_INVALID),
                     (dict(X0=inf_x), _abi.HJB_E_INVALID), (dict(X0=None), _abi.HJB_E_INVALID), (dict(thr=nan_thr), _abi.HJB_E_INVALID),
                     (dict(tol=neg_tol), _abi.HJB_E_INVALID), (dict(no_stats=True), _abi.HJB_E_INVALID), (dict(dtype=2), _abi.HJB_E_INVALID)):
        st, stats = call(**kw)
        assert st == code and np.all(stats == 7.25), (kw, st)
    st, stats = call(ns=0)
    assert st == _abi.HJB_OK and np.all(stats == 7.25)
