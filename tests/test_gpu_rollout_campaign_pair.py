"""GPU tests of the paired campaign (hjb_rollout_run_campaign_pair, csrc/kernels_rollout_campaign_pair.h and
csrc/kernels_rollout_lookahead_campaign_pair.h: K31; hjbdp.Rollout.run_campaign_pair, Dynamic_Solver.paired_cost_map).  The anchors
are code older than the pair: run_campaign (K28) and run_lookahead_campaign (K29) for the two plain records, and for the record of
the difference hjbdp.campaign_pair_reduce - itself held to the numpy restatement without a device, test_campaign_pair_refs.py - of
the per-trajectory costs and campaign_refs.left_flags of run_noisy (K25) and run_lookahead(noisy=True) (K27) on
np.repeat(X0, M, axis=1).  Everything is compared as bits unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

import campaign_pair_refs as prefs
import campaign_refs as crefs
import lookahead_campaign_refs as lc
import noisy_rollout_refs as nrefs
from lookahead_campaign_refs import PLANES, bits
from test_gpu_rollout_lookahead_campaign import DS_NODES, DS_WEIGHTS, kirk  # noqa: F401  (kirk: the fixture of that file)

pytestmark = pytest.mark.gpu

LPLANES = [1, 0, 2, 2, 1, 0]                # the label planes of the 6 steps (PLANES: the value planes)
SENT = 7.25
EPS = np.finfo(np.float64).eps


def _labels(pb, dtype, seed, n_labels=5, n_planes=3, base=1):
    nS = int(np.prod([len(k) for k in pb["knots"]]))
    return np.random.default_rng(seed).integers(base, base + n_labels, size=(nS, n_planes)).astype(dtype)


def _open(pb, labels, base=1):
    """an object holding the problem's labels, model, value planes, lookahead set and flight set"""
    import hjbdp
    ro = hjbdp.Rollout(pb["knots"], labels, pb["ut"], index_base=base)
    try:
        ro.set_model(pb["A"], pb["B"], **pb["model"])
        ro.set_values(pb["V"])
        ro.set_lookahead(pb["E"], pb["P"], pb["mode"])
        ro.set_noise(pb["F"], pb["Pf"])
    except Exception:
        ro.close()
        raise
    return ro


class _ZeroNode:
    """the object's lookahead set replaced by one zero node of weight 1 for the block, then put back"""

    def __init__(self, ro, pb, on=True):
        self.ro, self.pb, self.on = ro, pb, on

    def __enter__(self):
        if self.on:
            self.ro.set_lookahead(np.zeros((len(self.pb["knots"]), 1)), [1.0], "expect")

    def __exit__(self, *exc):
        if self.on:
            self.ro.set_lookahead(self.pb["E"], self.pb["P"], self.pb["mode"])


def _fly(ro, pb, X0, M, side, seed, first):
    """the per-trajectory flights of one controller by the code older than the pair, with the left-the-grid flags of its path"""
    Xr = np.repeat(X0, M, axis=1)
    if side[0] == "labels":
        out = ro.run_noisy(Xr, side[1], seed=seed, first_stream=first, method=side[2], keep_path=True)
    else:
        with _ZeroNode(ro, pb, side[0] == "greedy"):
            out = ro.run_lookahead(Xr, side[1], noisy=True, seed=seed, first_stream=first, keep_path=True)
    return {"cost": out["cost"], "left": crefs.left_flags(out["X_path"], pb["knots"])}


def _plain(ro, pb, X0, M, side, seed, first, thr, tol):
    """the plain campaign of one controller"""
    if side[0] == "labels":
        return ro.run_campaign(X0, side[1], M, seed=seed, first_stream=first, method=side[2], cost_threshold=thr, settle_tol=tol)
    with _ZeroNode(ro, pb, side[0] == "greedy"):
        return ro.run_lookahead_campaign(X0, side[1], M, seed=seed, first_stream=first, cost_threshold=thr, settle_tol=tol)


def _check_pair(ro, pb, X0, M, a, b, seed, first, thr=None, tol=None, flown=None, what=None):
    """one pair call against the three anchors -> (the pair's dict, the flights of a and of b)"""
    import hjbdp
    fa, fb = flown if flown is not None else (_fly(ro, pb, X0, M, a, seed, first), _fly(ro, pb, X0, M, b, seed, first))
    got = ro.run_campaign_pair(X0, a, b, M, seed=seed, first_stream=first, cost_threshold=thr, settle_tol=tol)
    ns = X0.shape[1]
    for key, side in (("a", a), ("b", b)):
        want = _plain(ro, pb, X0, M, side, seed, first, thr, tol)
        assert got[key]["stats"].shape == (ns, 8)
        assert np.array_equal(bits(got[key]["stats"]), bits(want["stats"])), (what, key, got[key]["stats"], want["stats"])
    want = hjbdp.campaign_pair_reduce(fa["cost"], fb["cost"], M, left_a=fa["left"], left_b=fb["left"])
    assert got["stats_d"].shape == (ns, 8)
    rows = [i for i in range(ns) if not prefs.same_bits(got["stats_d"][i], want["stats_d"][i])]               # a NaN equals a NaN
    assert not rows, (what, rows, got["stats_d"][rows].tolist(), want["stats_d"][rows].tolist())
    for key in ("mean_diff", "var_diff", "std_diff", "se_diff", "t", "min_diff", "max_diff", "n_b_lower", "n_a_lower", "n_tie", "n_both_in",
                "mean_diff_both_in"):
        assert np.array_equal(got[key], want[key], equal_nan=True), (what, key)
    return got, (fa, fb)


def _check_sum_bound(got, M):
    """|sum d - (sum c_B - sum c_A)| <= 4 M eps (sum c_A + sum c_B) per start with finite costs: the costs are non-negative
    (q, r >= 0), each of the three sums over M terms is within (M - 1) eps of its exact value relative to the sum of the
    magnitudes whatever the order of summation, |d| <= c_A + c_B, and each d carries one rounding of its own"""
    sa, sb, sd = got["a"]["stats"][:, 0], got["b"]["stats"][:, 0], got["stats_d"][:, 0]
    ok = np.isfinite(got["a"]["stats"][:, 3]) & np.isfinite(got["b"]["stats"][:, 3])
    assert ok.any() and np.all(got["a"]["stats"][ok, 2] >= 0) and np.all(got["b"]["stats"][ok, 2] >= 0)
    err, bound = np.abs(sd[ok] - (sb[ok] - sa[ok])), 4 * M * EPS * (sa[ok] + sb[ok])
    print("sum bound: max error %.3e, min bound %.3e" % (err.max(), bound.min()))
    assert np.all(err <= bound), (err, bound)


# ---- 1. every instantiation, in both roles ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_every_label_instantiation_in_both_roles(built, D, dtype):
    """k_rollout_campaign_pair<D, label type, method, LDS> as A (it fills the scratch) and as B (it reads it and reduces d), the
    other side the lookahead kernel; the value type alternates"""
    pb = lc.problem(D, np.float32 if (D + np.dtype(dtype).itemsize) % 2 else np.float64)
    M, ns = 5, lc.N_STARTS                          # G = 8 with three padding slots; 37 blocks: the last wave part-filled
    X0, seed, first = pb["X0"], pb["seed"], pb["first"]
    look = ("lookahead", PLANES)
    one_sided = 0
    with _open(pb, _labels(pb, dtype, 3100 + D)) as ro:
        fb = _fly(ro, pb, X0, M, look, seed, first)
        for method in ("nearest", "linear"):
            lab = ("labels", LPLANES, method)
            fa = _fly(ro, pb, X0, M, lab, seed, first)
            both = np.concatenate([fa["cost"], fb["cost"]])
            bounds = (float(np.median(both[np.isfinite(both)])), np.full(D, 0.4))         # a label flight may overflow outside the grid
            for lds in (1, 0):
                ro.set_option("lds", lds)
                ta, tb = (bounds, (None, None)) if lds else ((None, None), bounds)          # given and not given, in both roles
                got, _ = _check_pair(ro, pb, X0, M, lab, look, seed, first, *ta, flown=(fa, fb), what=(method, lds, "A"))
                _check_sum_bound(got, M)
                rev, _ = _check_pair(ro, pb, X0, M, look, lab, seed, first, *tb, flown=(fb, fa), what=(method, lds, "B"))
                _check_sum_bound(rev, M)
                assert got["device_ms"] > 0
            one_sided += int((fa["left"] != fb["left"]).sum())
            n_in = got["n_both_in"]
            assert (n_in > 0).any() and (n_in < M).any()                        # index 6 is neither 0 nor M everywhere
    assert one_sided > 0                                                        # flights that left the grid on one side only


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_lookahead_instantiation_in_both_roles(built, D, dtype):
    """k_rollout_lookahead_campaign_pair<D, value type, LDS> on both sides: the object's lookahead set against one zero node"""
    pb = lc.problem(D, dtype)
    M = 5
    X0, seed, first = pb["X0"], pb["seed"], pb["first"]
    look, greedy = ("lookahead", PLANES), ("greedy", PLANES)
    with _open(pb, _labels(pb, np.uint8, 3200 + D)) as ro:
        fa, fb = _fly(ro, pb, X0, M, look, seed, first), _fly(ro, pb, X0, M, greedy, seed, first)
        bounds = (float(np.median(fa["cost"][np.isfinite(fa["cost"])])), np.full(D, 0.4))
        for lds in (1, 0):
            ro.set_option("lds", lds)
            ta, tb = (bounds, (None, None)) if lds else ((None, None), bounds)
            got, _ = _check_pair(ro, pb, X0, M, look, greedy, seed, first, *ta, flown=(fa, fb), what=(lds, "look-greedy"))
            _check_sum_bound(got, M)
            rev, _ = _check_pair(ro, pb, X0, M, greedy, look, seed, first, *tb, flown=(fb, fa), what=(lds, "greedy-look"))
            _check_sum_bound(rev, M)
    n_in = got["n_both_in"]
    assert (n_in > 0).any() and (n_in < M).any()


# ---- 2. block shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3, 63, 64, 65, 200])
def test_block_shapes(built, M):
    """one block per start (M <= 64), two blocks with the second almost all padding (65), four blocks (200); 1, 3 and 70 starts"""
    pb = lc.problem(2, np.float64, n_starts=70)
    with _open(pb, _labels(pb, np.uint16, 3300)) as ro:
        for ns in (1, 3, 70):
            X0 = pb["X0"][:, 70 - ns:] if ns < 70 else pb["X0"]     # the few starts from the end: outside the grid
            got, _ = _check_pair(ro, pb, X0, M, ("labels", LPLANES, "linear"), ("lookahead", PLANES), 11 + ns, 1000 * ns, 0.5, 0.3,
                                 what=(M, ns))
            assert np.array_equal(got["n_tie"] + got["n_b_lower"] + got["n_a_lower"], np.full(ns, M))


# ---- 3. chunks, streams, LDS -----------------------------------------------------------------------------------------------------------
def test_chunks_streams_and_lds_change_no_bit(built):
    pb = lc.problem(2, np.float32, n_starts=14)
    M, first = 200, 300
    X0 = pb["X0"]
    a, b = ("labels", LPLANES, "linear"), ("lookahead", PLANES)
    kw = dict(seed=12, cost_threshold=0.5, settle_tol=0.3)
    recs = lambda out: np.concatenate([bits(out["a"]["stats"]), bits(out["b"]["stats"]), bits(out["stats_d"])], axis=1)
    with _open(pb, _labels(pb, np.int32, 3400)) as ro:
        whole, _ = _check_pair(ro, pb, X0[:, :7], M, a, b, 12, first, 0.5, 0.3, what="whole")
        for chunk in (64, 192, 1 << 20, 1):         # one block a launch; three: a start's four blocks across launches, the scratch
            ro.set_option("chunk", chunk)           # re-used launch after launch; one launch; below one block: still a whole block
            for lds in (1, 0):
                ro.set_option("lds", lds)
                got = ro.run_campaign_pair(X0[:, :7], a, b, M, first_stream=first, **kw)
                assert np.array_equal(recs(got), recs(whole)), (chunk, lds)
        ro.set_option("chunk", 1 << 20)
        ro.set_option("lds", 1)
        both = ro.run_campaign_pair(X0, a, b, M, first_stream=first, **kw)
        second = ro.run_campaign_pair(X0[:, 7:], a, b, M, first_stream=first + 7 * M, **kw)
        assert np.array_equal(recs(both)[:7], recs(whole)) and np.array_equal(recs(both)[7:], recs(second))
        other = ro.run_campaign_pair(X0[:, :7], a, b, M, seed=13, first_stream=first)
        assert not np.array_equal(other["stats_d"][:, 0], whole["stats_d"][:, 0])


# ---- 4. identities -------------------------------------------------------------------------------------------------------------------
def test_a_controller_against_itself_and_the_swapped_pair(built):
    pb = lc.problem(3, np.float64)
    M = 5
    X0, seed, first = pb["X0"], pb["seed"], pb["first"]
    lab, look, greedy = ("labels", LPLANES, "linear"), ("lookahead", PLANES), ("greedy", PLANES)
    with _open(pb, _labels(pb, np.uint8, 3500)) as ro:
        for side in (lab, look, greedy):
            got = ro.run_campaign_pair(X0, side, side, M, seed=seed, first_stream=first, cost_threshold=0.5, settle_tol=0.4)
            assert np.array_equal(bits(got["a"]["stats"]), bits(got["b"]["stats"])), side[0]
            sd = got["stats_d"]
            fin = np.isfinite(got["a"]["stats"][:, 3])                          # a flight that overflowed has d = inf - inf
            assert fin.sum() > len(fin) // 2
            assert not sd[fin][:, (0, 1, 2, 3, 7)].any(), (side[0], sd)         # d is 0 in every sample: sums, min and max
            assert not sd[:, (4, 5)].any() and np.all(got["n_tie"] == M)        # ... and nobody is lower, a NaN d included
            assert np.array_equal(sd[:, 6], M - got["a"]["stats"][:, 5])
        # HJB_PAIR_GREEDY is the kind LOOKAHEAD after set_lookahead(zeros, [1.0], "expect"); it leaves the object's set alone
        g = ro.run_campaign_pair(X0, lab, greedy, M, seed=seed, first_stream=first)
        again = ro.run_lookahead_campaign(X0, PLANES, M, seed=seed, first_stream=first)      # still under the object's own set
        with _ZeroNode(ro, pb):
            l = ro.run_campaign_pair(X0, lab, look, M, seed=seed, first_stream=first)
        for key in ("a", "b"):
            assert np.array_equal(bits(g[key]["stats"]), bits(l[key]["stats"])), key
        assert np.array_equal(bits(g["stats_d"]), bits(l["stats_d"]))
        own = ro.run_campaign_pair(X0, lab, look, M, seed=seed, first_stream=first)
        assert np.array_equal(bits(own["b"]["stats"]), bits(again["stats"])) and not np.array_equal(own["b"]["stats"], g["b"]["stats"])
        # the swapped pair gives the antisymmetric record, as values
        rev = ro.run_campaign_pair(X0, look, lab, M, seed=seed, first_stream=first)
        assert prefs.same_values(rev["stats_d"], prefs.swap_of(own["stats_d"]))
        assert np.array_equal(bits(rev["a"]["stats"]), bits(own["b"]["stats"])) and np.array_equal(bits(rev["b"]["stats"]), bits(own["a"]["stats"]))
        assert own["n_b_lower"].sum() > 0 and own["n_a_lower"].sum() > 0


@pytest.mark.parametrize("mode", ["expect", "worst"])
def test_lattice_labels_against_lookahead_differ_nowhere(built, mode):
    """on the exactly posed lattice the flights of the stored labels and of the lookahead coincide (K27's and K29's lattice tests):
    d is zero in every one of the 9 x 2^12 samples"""
    import hjbdp
    K = nrefs.LATTICE_STAGES
    with hjbdp.Backup(nrefs.lattice_spec(mode)) as bk:
        sol = bk.solve(K, keep_J=True, keep_idx=True)
    J = sol["J_stages"].reshape(33, K, order="F")
    idx = sol["idx_stages"].reshape(33, K, order="F")
    weights = nrefs.LATTICE_P if mode == "expect" else None
    X0 = nrefs.LATTICE_STARTS.reshape(1, -1)
    M = 1 << 12
    with hjbdp.Rollout([nrefs.LATTICE_KNOTS], idx, nrefs.LATTICE_U, index_base=0) as ro:
        ro.set_model([[1.0]], [[1.0]], q=[1.0], r=[0.5])
        ro.set_noise(nrefs.LATTICE_NODES, weights)
        ro.set_values(J)
        ro.set_lookahead(nrefs.LATTICE_NODES, weights, mode)
        got = ro.run_campaign_pair(X0, ("labels", np.arange(K), "nearest"), ("lookahead", list(range(1, K)) + [-1]), M, seed=2029)
    sd = got["stats_d"]
    assert not sd[:, (0, 1, 2, 3, 4, 5, 7)].any(), sd
    assert np.all(sd[:, 6] == M) and np.all(got["n_tie"] == M)
    assert np.array_equal(bits(got["a"]["stats"]), bits(got["b"]["stats"])) and np.all(got["a"]["std"] > 0)


# ---- 6. isolation and refusals with a device ---------------------------------------------------------------------------------------
def _others(ro, X0, label_planes):
    """every other run function of the object, paths kept"""
    return (ro.run(X0, label_planes, keep_path=True), ro.run_noisy(X0, label_planes, seed=5, keep_path=True),
            ro.run_greedy(X0, [1, 0, -1], keep_path=True), ro.run_lookahead(X0, [1, 0, -1], keep_path=True),
            ro.run_lookahead(X0, [1, 0, -1], noisy=True, seed=5, first_stream=9, keep_path=True),
            ro.run_campaign(X0[:, :11], label_planes[:4], 6, seed=4, cost_threshold=0.5, settle_tol=0.4),
            ro.run_lookahead_campaign(X0[:, :11], [1, 0, -1, 1], 6, seed=4, cost_threshold=0.5, settle_tol=0.4))


def test_isolation_and_refusals_with_a_device(built):
    import hjbdp
    from hjbdp import _abi
    from test_gpu_rollout import _random_problem
    import lookahead_rollout_refs as lrefs
    rng = np.random.default_rng(314)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 3, 2, np.uint16, 9, 4)
    lo = np.array([k[0] for k in knots]) - 0.1
    hi = np.array([k[-1] for k in knots]) + 0.1
    X0 = rng.uniform(lo[:, None], hi[:, None], size=(3, 300))
    label_planes = rng.integers(0, 4, size=6)
    nS = int(np.prod([len(k) for k in knots]))
    V = rng.uniform(0, 1, size=(nS, 2))
    off, p = rng.uniform(-0.2, 0.2, size=(3, 5)), rng.uniform(0.1, 1.0, size=5)
    E, P = lrefs.node_sets(rng, 3, 3, [0, 2])
    ns, M = 11, 6
    lplanes = np.ascontiguousarray(label_planes[:4], dtype=np.int32)
    vplanes = np.array([1, 0, -1, 1], dtype=np.int32)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    Xc = np.ascontiguousarray(X0[:, :ns].T)
    LAB, LOOK, GREEDY = _abi.HJB_PAIR_LABELS, _abi.HJB_PAIR_LOOKAHEAD, _abi.HJB_PAIR_GREEDY

    def raw(ro, **call):
        """hjb_rollout_run_campaign_pair through ctypes on sentinel-filled outputs -> (status, outputs untouched, the text)"""
        out = [np.full(ns * 8, SENT) for _ in range(3)]
        ms = C.c_double(SENT)
        ptr = [dp(o) for o in out]
        for i, key in enumerate(("sa", "sb", "sd")):
            if key in call:
                ptr[i] = call[key]
        st = ro.lib.hjb_rollout_run_campaign_pair(ro._ro, call.get("ka", LAB), call.get("ma", 1), call.get("pa", ip(lplanes)),
                                                  call.get("kb", LOOK), call.get("mb", 0), call.get("pb", ip(vplanes)), call.get("K", 4),
                                                  call.get("ns", ns), call.get("M", M), call.get("X", dp(Xc)), 4, call.get("first", 0),
                                                  call.get("thr", None), call.get("tol", None), *ptr, C.byref(ms))
        return st, bool(all(np.all(o == SENT) for o in out) and ms.value == SENT), ro.lib.hjb_rollout_last_error(ro._ro).decode()

    def refused(ro, text, **call):
        st, untouched, err = raw(ro, **call)
        assert st == _abi.HJB_E_INVALID and untouched, (call, st, untouched, err)
        for t in ([text] if isinstance(text, str) else text):
            assert t in err, (call, t, err)

    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        refused(ro, ("A:", "run before hjb_rollout_set_model"))
        refused(ro, ("A:", "before hjb_rollout_set_model"), ka=GREEDY, pa=ip(vplanes))
        ro.set_model(A, B, c=c, q=np.ones(3), r=[0.5, 0.25])
        refused(ro, ("A:", "before hjb_rollout_set_noise"))
        refused(ro, ("A:", "before hjb_rollout_set_lookahead"), ka=LOOK, pa=ip(vplanes))
        ro.set_noise(off, p)
        zero_fn = np.full(4, -1, dtype=np.int32)
        refused(ro, ("B:", "before hjb_rollout_set_lookahead"))
        refused(ro, ("B:", "before hjb_rollout_set_lookahead"), ka=GREEDY, pa=ip(zero_fn))       # A's greedy needs no set; B's kind does
        refused(ro, ("B:", "before hjb_rollout_set_values"), kb=GREEDY)
        st, untouched, _ = raw(ro, kb=GREEDY, pb=ip(zero_fn))                   # only -1: no values, and no lookahead set
        assert st == _abi.HJB_OK and not untouched
        ro.set_lookahead(E, P)
        refused(ro, ("B:", "before hjb_rollout_set_values"))
        ro.set_values(V)
        # the object holds everything: every other run function gives the bits it gave before the pair calls
        before = _others(ro, X0, label_planes)
        a, b, g = ("labels", lplanes, "linear"), ("lookahead", vplanes), ("greedy", vplanes)
        good = ro.run_campaign_pair(X0[:, :ns], a, b, M, seed=4, cost_threshold=0.5, settle_tol=0.4)
        ro.run_campaign_pair(X0[:, :ns], g, a, M, seed=4)
        after = _others(ro, X0, label_planes)
        for x, y in zip(after, before):
            for key in x:
                if key != "device_ms" and x[key] is not None:
                    assert np.array_equal(x[key], y[key], equal_nan=True), key
        assert np.array_equal(bits(good["a"]["stats"]), bits(after[5]["stats"])) and np.array_equal(bits(good["b"]["stats"]), bits(after[6]["stats"]))
        # the refusals, each on sentinel-filled outputs that stay untouched
        Xn = Xc.copy()
        Xn[7, 2] = np.inf
        thr, tol = np.full(ns, 0.5), np.full(3, 0.4)
        bad_thr, bad_tol, neg_tol = thr.copy(), tol.copy(), tol.copy()
        bad_thr[4], bad_tol[1], neg_tol[2] = np.nan, np.nan, -0.1
        for call, text in ((dict(ka=3), ("A:", "kind 3")), (dict(kb=-1), ("B:", "kind -1")), (dict(ma=2), ("A:", "method 2")),
                           (dict(ka=LAB, kb=LAB, pb=ip(lplanes), mb=7), ("B:", "method 7")),
                           (dict(first=-1), "first_stream=-1 < 0"), (dict(first=2 ** 63 - 10), "overflows"), (dict(M=0), "n_samples=0 < 1"),
                           (dict(M=2 ** 62), "n_starts * n_samples overflows"), (dict(K=-1), "n_steps=-1"), (dict(ns=-2), "n_traj=-2"),
                           (dict(pa=ip(np.array([0, 4, 0, 0], dtype=np.int32))), ("A:", "plane_of_step[1] = 4 outside [0, 4)")),
                           (dict(pb=ip(np.array([0, 2, 0, 0], dtype=np.int32))), ("B:", "value_plane_of_step[1] = 2 outside [-1, 2)")),
                           (dict(ka=GREEDY, pa=ip(np.array([0, 0, -2, 0], dtype=np.int32))), ("A:", "value_plane_of_step[2] = -2")),
                           (dict(pa=None), ("A:", "null plane_of_step")), (dict(pb=None), ("B:", "null value_plane_of_step")),
                           (dict(X=dp(Xn)), "not finite"), (dict(X=None), "null X0"), (dict(thr=dp(bad_thr)), "threshold[4] is NaN"),
                           (dict(tol=dp(bad_tol)), "tol[1]"), (dict(tol=dp(neg_tol)), "tol[2]"), (dict(sa=None), "null stats_a"),
                           (dict(sb=None), "null stats_a / stats_b"), (dict(sd=None), "stats_d")):
            refused(ro, text, **call)
        st, untouched, _ = raw(ro, ns=0)                                        # no starts: no work
        assert st == _abi.HJB_OK
        none = ro.run_campaign_pair(np.zeros((3, 0)), a, b, M)
        assert none["stats_d"].shape == (0, 8) and none["device_ms"] == 0.0
        again = ro.run_campaign_pair(X0[:, :ns], a, b, M, seed=4, cost_threshold=0.5, settle_tol=0.4)
        assert np.array_equal(bits(again["stats_d"]), bits(good["stats_d"])) and again["device_ms"] > 0
        with pytest.raises(ValueError):
            ro.run_campaign_pair(X0[:, :ns], ("other", vplanes), b, M)
        with pytest.raises(ValueError):
            ro.run_campaign_pair(X0[:, :ns], a, ("lookahead", vplanes[:3]), M)
    lib = hjbdp.load_library()
    assert lib.hjb_rollout_run_campaign_pair(None, 0, 1, None, 1, 0, None, 0, 0, 1, None, 0, 0, None, None, None, None, None, None) \
        == _abi.HJB_E_INVALID
    knots6 = [np.linspace(-1, 1, 3)] * 6                                        # a model other than the affine one
    with hjbdp.Rollout(knots6, rng.integers(1, 4, size=(3 ** 6, 1)).astype(np.uint8), rng.uniform(-1, 1, size=(3, 3)), index_base=1) as ro:
        ro.set_attitude_model([1.0, 2.0, 3.0], 0.01)
        ro.set_values(np.zeros((3 ** 6, 1)))
        ro.set_lookahead(np.zeros((6, 1)))
        ro.set_noise(np.full((6, 2), 0.01))
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_campaign_pair(np.zeros((6, 4)), ("lookahead", [0, -1]), ("labels", [0, 0], "linear"), 3)
        assert ei.value.status == _abi.HJB_E_INVALID and "A:" in str(ei.value) and "needs the affine model" in str(ei.value)
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_campaign_pair(np.zeros((6, 4)), ("labels", [0, 0], "linear"), ("greedy", [0, -1]), 3)
        assert ei.value.status == _abi.HJB_E_INVALID and "A:" in str(ei.value) and "attitude" in str(ei.value)


# ---- 7. the mirror -------------------------------------------------------------------------------------------------------------------
def test_dynamic_solver_paired_cost_map(kirk):  # noqa: F811
    import hjbdp
    ds, s_r, nodes = kirk
    M = 8
    pmap = ds.paired_cost_map(M, a="labels", b="disturbed", seed=6, cost_threshold=1.0)
    labels = ds.noisy_cost_map(M, seed=6, cost_threshold=1.0)
    disturbed = ds.lookahead_cost_map(M, seed=6, cost_threshold=1.0)
    assert pmap["a"]["stats"].shape == (13, 13, 8) and pmap["stats_d"].shape == (13, 13, 8) and pmap["mean_diff"].shape == (13, 13)
    assert np.array_equal(bits(pmap["a"]["stats"]), bits(labels["stats"])) and np.array_equal(bits(pmap["b"]["stats"]), bits(disturbed["stats"]))
    assert np.array_equal(pmap["a"]["mean"], labels["mean"]) and np.array_equal(pmap["b"]["n_exceed"], disturbed["n_exceed"])
    ca = ds.get_noisy_paths(nodes, M, seed=6)                                   # [169, 8] each, the same streams
    cb = ds.get_lookahead_paths(nodes, n_samples=M, seed=6)
    want = hjbdp.campaign_pair_reduce(ca.reshape(-1), cb.reshape(-1), M)        # no flags: every index but 6 and 7
    sd = pmap["stats_d"].reshape(169, 8, order="F")
    assert prefs.same_bits(sd[:, :6], want["stats_d"][:, :6])
    for key in ("mean_diff", "var_diff", "se_diff", "n_b_lower", "n_a_lower", "n_tie"):
        assert np.array_equal(pmap[key].reshape(-1, order="F"), want[key], equal_nan=True), key
    assert pmap["n_b_lower"].sum() > 0 and pmap["n_a_lower"].sum() > 0 and pmap["device_ms"] > 0
    # ("nominal", "disturbed") against a run flown by hand, left flags included
    pair = ds.paired_cost_map(M, a="nominal", b="disturbed", seed=6, settle_tol=0.5)
    ut = np.asarray(ds._U_mesh, dtype=np.float64)
    flown = []
    with hjbdp.Rollout([s_r, s_r], ds.u_star_idxs, ut, index_base=1) as ro:
        ro.set_model(ds.A, ds.B, q=np.diag(ds.Q), r=[ds.R])
        ro.set_values(ds.J_star)
        ro.set_noise(DS_NODES, DS_WEIGHTS)
        for E, P in ((np.zeros((2, 1)), [1.0]), (DS_NODES, DS_WEIGHTS)):
            ro.set_lookahead(E, P, "expect")
            out = ro.run_lookahead(np.repeat(nodes, M, axis=1), np.arange(1, 6), noisy=True, seed=6, first_stream=0, keep_path=True)
            flown.append((out["cost"], crefs.left_flags(out["X_path"], [s_r, s_r])))
    want = hjbdp.campaign_pair_reduce(flown[0][0], flown[1][0], M, left_a=flown[0][1], left_b=flown[1][1])
    assert prefs.same_bits(pair["stats_d"].reshape(169, 8, order="F"), want["stats_d"])
    nominal = ds.lookahead_cost_map(M, seed=6, lookahead="nominal", settle_tol=0.5)
    assert np.array_equal(bits(pair["a"]["stats"]), bits(nominal["stats"]))
    stat = ds.get_paired_cost_statistics(nodes[:, 10:13], M, a="disturbed", b="labels", seed=6)       # three starts on streams 0 .. 3 M
    assert stat["stats_d"].shape == (3, 8)
    for kw in (dict(a="other"), dict(b="greedy"), dict(a=None)):
        with pytest.raises(ValueError):
            ds.get_paired_cost_statistics(nodes[:, :2], M, **kw)
    saved, ds.disturbance = ds.disturbance, None
    try:
        with pytest.raises(RuntimeError):
            ds.paired_cost_map(4)
    finally:
        ds.disturbance = saved
