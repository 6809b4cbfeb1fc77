"""GPU tests of the campaign histogram (hjb_rollout_run_campaign_hist, csrc/kernels_rollout_campaign_hist.h: K30;
hjbdp.Rollout.run_campaign(hist=...), Dynamic_Solver.get_noisy_cost_quantiles): the counts equal to the host reduce of
hjb_rollout_run_noisy's own costs and the statistics bit-equal to the plain campaign's at every instantiation, block and
workgroup shape and chunking; samples exactly on lo and on hi; the two-pass quantiles against the order statistics; validation."""
import ctypes as C

import numpy as np
import pytest

import campaign_hist_refs as hrefs
from test_gpu_rollout_campaign import _bits, _problem, _starts

pytestmark = pytest.mark.gpu


def _check(ro, X0, planes, M, seed, first, method, lo, hi, n_bins, flown=None):
    """run_campaign(hist=...) against campaign_hist_reduce of run_noisy's own costs, and its stats against the plain call's bits"""
    import hjbdp
    ns = X0.shape[1]
    if flown is None:
        flown = ro.run_noisy(np.repeat(X0, M, axis=1), planes, seed=seed, first_stream=first, method=method)
    plain = ro.run_campaign(X0, planes, M, seed=seed, first_stream=first, method=method, cost_threshold=0.4, settle_tol=0.3)
    got = ro.run_campaign(X0, planes, M, seed=seed, first_stream=first, method=method, cost_threshold=0.4, settle_tol=0.3,
                          hist=(lo, hi, n_bins))
    want = hjbdp.campaign_hist_reduce(flown["cost"], M, lo, hi, n_bins)
    assert got["hist"].shape == (ns, n_bins + 2) and got["hist"].dtype == np.int64
    assert np.array_equal(got["hist"], want), (M, ns, n_bins, got["hist"], want)
    assert np.all(got["hist"].sum(axis=1) == M)
    assert np.array_equal(_bits(got["stats"]), _bits(plain["stats"])), (M, ns, n_bins)
    assert np.array_equal(got["hist_lo"], np.broadcast_to(lo, (ns,))) and np.array_equal(got["hist_hi"], np.broadcast_to(hi, (ns,)))
    return got, flown


# ---- 1. every instantiation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_every_instantiation_counts_what_the_host_reduce_counts(built, D, dtype):
    import hjbdp
    rng = np.random.default_rng(3000 + 100 * D + np.dtype(dtype).itemsize)
    nu = 1 + D % 3
    knots, labels, ut, base, A, B, c = _problem(rng, D, nu, dtype)
    M, ns, n_bins = 5, 3, 4
    X0 = _starts(rng, knots, ns)
    planes = rng.integers(0, 3, size=9)
    off, p = rng.uniform(-0.3, 0.3, size=(D, 5)), rng.uniform(0.1, 1.0, size=5)
    seed, first = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=rng.uniform(0, 1, size=D), r=rng.uniform(0, 1, size=nu))
        ro.set_noise(off, p)
        for method in ("nearest", "linear"):
            flown = ro.run_noisy(np.repeat(X0, M, axis=1), planes, seed=seed, first_stream=first, method=method)
            lo, hi = hrefs.exact_range(flown["cost"], M)
            for lds in (1, 0):
                ro.set_option("lds", lds)
                got, _ = _check(ro, X0, planes, M, seed, first, method, lo, hi, n_bins, flown)
                assert not got["hist"][:, 0].any() and not got["hist"][:, -1].any()       # the exact range: nothing under or over
                assert np.all(got["hist"][:, 1] >= 1) and np.all(got["hist"][:, n_bins] >= 1)   # the min in bin 1, the max in the last


# ---- 2. block and workgroup shapes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3, 63, 64, 65, 200, 300])
def test_block_and_workgroup_shapes(built, M):
    """G < 64 counts with global atomics (M = 1 with 300 starts: 256 starts in one workgroup); G = 64 with a histogram per wave in
    LDS: a workgroup of four blocks of one start (200, 300), of several starts (65: two blocks a start), part-filled at the end"""
    import hjbdp
    rng = np.random.default_rng(3300 + M)
    knots, labels, ut, base, A, B, c = _problem(rng, 2, 2, np.uint16)
    planes = rng.integers(0, 3, size=6)
    off, p = rng.uniform(-0.3, 0.3, size=(2, 4)), rng.uniform(0.1, 1.0, size=4)
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=[1.0, 0.5], r=[0.1, 0.2])
        ro.set_noise(off, p)
        for ns, n_bins in ((1, 7), (5, 256), (300, 1), (5, 1), (300, 7)):
            X0 = _starts(rng, knots, ns)
            flown = ro.run_noisy(np.repeat(X0, M, axis=1), planes, seed=11 + ns, first_stream=1000 * ns)
            cost = flown["cost"].reshape(ns, M)
            lo, hi = hrefs.exact_range(cost, M)
            hi = np.where(lo < hi, hi, lo + 1.0)
            _check(ro, X0, planes, M, 11 + ns, 1000 * ns, "linear", lo, hi, n_bins, flown)
            if ns == 5:
                # every sample of a start in ONE bin - the hot counter - and ranges that put samples under and over
                wide_lo, wide_hi = cost.min(axis=1) - 1.0, cost.max(axis=1) + 1e6
                got, _ = _check(ro, X0, planes, M, 11 + ns, 1000 * ns, "linear", wide_lo, wide_hi, n_bins, flown)
                assert np.all(got["hist"][:, 1] == M)
                med = np.median(cost, axis=1)
                got, _ = _check(ro, X0, planes, M, 11 + ns, 1000 * ns, "linear", med - 1e-3, med + 1e-3, n_bins, flown)
                if M >= 63:
                    assert got["hist"][:, 0].sum() > 0 and got["hist"][:, -1].sum() > 0
                got, _ = _check(ro, X0, planes, M, 11 + ns, 1000 * ns, "linear", 1e9, 2e9, n_bins, flown)      # one scalar range: all under
                assert np.all(got["hist"][:, 0] == M)


# ---- 3. chunking -------------------------------------------------------------------------------------------------------------------
def test_chunks_change_no_count(built):
    """3 starts x 200 samples are 12 blocks: a launch of one block, of three (a start's four blocks across launches: the
    histogram persists on the device between them), of all; and a chunk below one block"""
    import hjbdp
    rng = np.random.default_rng(3400)
    knots, labels, ut, base, A, B, c = _problem(rng, 2, 2, np.uint8)
    planes = rng.integers(0, 3, size=6)
    off, p = rng.uniform(-0.3, 0.3, size=(2, 9)), rng.uniform(0.1, 1.0, size=9)
    M, ns, n_bins = 200, 3, 16
    X0 = _starts(rng, knots, ns)
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=[1.0, 0.5], r=[0.1, 0.2])
        ro.set_noise(off, p)
        flown = ro.run_noisy(np.repeat(X0, M, axis=1), planes, seed=12)
        lo, hi = hrefs.exact_range(flown["cost"], M)
        whole, _ = _check(ro, X0, planes, M, 12, 0, "linear", lo, hi, n_bins, flown)
        for chunk in (1, 64, 192, 1 << 20):
            ro.set_option("chunk", chunk)
            got, _ = _check(ro, X0, planes, M, 12, 0, "linear", lo, hi, n_bins, flown)
            assert np.array_equal(got["hist"], whole["hist"]) and np.array_equal(_bits(got["stats"]), _bits(whole["stats"])), chunk


# ---- 4. edges on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [16, 256])
def test_samples_exactly_on_lo_and_on_hi(built, M):
    """one zero-offset node: every sample's cost is K16's exactly (test_gpu_rollout_campaign.py establishes it).  lo = that cost:
    all M samples in bin 1; hi = that cost: all M in the overflow"""
    import hjbdp
    rng = np.random.default_rng(3500 + M)
    knots, labels, ut, base, A, B, c = _problem(rng, 3, 2, np.int32)
    ns, n_bins = 21, 7
    X0 = _starts(rng, knots, ns)
    planes = rng.integers(0, 3, size=6)
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=[1.0, 0.5, 0.25], r=[0.1, 0.2])
        ro.set_noise(np.zeros((3, 1)))
        k16 = ro.run(X0, planes)["cost"]
        at_lo = ro.run_campaign(X0, planes, M, seed=5, hist=(k16, k16 + 1.0, n_bins))
        assert np.array_equal(_bits(at_lo["min"]), _bits(k16)) and np.array_equal(_bits(at_lo["max"]), _bits(k16))
        assert np.all(at_lo["hist"][:, 1] == M) and at_lo["hist"].sum() == ns * M
        at_hi = ro.run_campaign(X0, planes, M, seed=5, hist=(k16 - 1.0, k16, n_bins))
        assert np.all(at_hi["hist"][:, n_bins + 1] == M) and at_hi["hist"].sum() == ns * M
        below_hi = ro.run_campaign(X0, planes, M, seed=5, hist=(k16 - 1.0, np.nextafter(k16, np.inf), n_bins))
        assert np.all(below_hi["hist"][:, n_bins] == M)
        above = ro.run_campaign(X0, planes, M, seed=5, hist=(np.nextafter(k16, np.inf), k16 + 1.0, n_bins))
        assert np.all(above["hist"][:, 0] == M)


# ---- 5. two-pass quantiles -----------------------------------------------------------------------------------------------------------
def test_two_pass_quantiles_bracket_the_order_statistics(built):
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N, ds.dx, ds.du = 6, 9, 20
    off, w = hjbdp.gaussian_nodes([0.02, 0.05], order=3)
    ds.disturbance = (off, w, "expect")
    ds.run()
    M, n_bins = 256, 64
    qs = (0.0, 0.5, 0.95, 0.99, 1.0)
    X0s = np.array([[0.3, -0.5, 0.1, 0.0], [0.2, 0.4, -0.6, 0.0]])
    out = ds.get_noisy_cost_quantiles(X0s, M, q=qs, n_bins=n_bins, seed=6)
    cost = ds.get_noisy_paths(X0s, M, seed=6)                                   # [4, 256], the same streams
    srt = np.sort(cost, axis=1)
    assert out["quantiles"].shape == (4, len(qs)) and out["hist"].shape == (4, n_bins + 2)
    assert np.array_equal(out["min"], srt[:, 0]) and np.array_equal(out["max"], srt[:, -1])
    assert np.array_equal(out["hist"], hjbdp.campaign_hist_reduce(cost, M, out["hist_lo"], out["hist_hi"], n_bins))
    assert not out["hist"][:, 0].any() and not out["hist"][:, -1].any() and np.all(out["hist"].sum(axis=1) == M)
    plain = ds.get_noisy_cost_statistics(X0s, M, seed=6)
    assert np.array_equal(_bits(out["stats"]), _bits(plain["stats"]))
    for s in range(4):
        lo, hi = out["hist_lo"][s], out["hist_hi"][s]
        assert lo == srt[s, 0] and (hi == np.nextafter(srt[s, -1], np.inf) or (srt[s, 0] == srt[s, -1] and hi == lo + 1.0))
        for i, q in enumerate(qs):
            j = hrefs.quantile_column(out["hist"][s], q)
            x = srt[s, hrefs.rank_of(q, M) - 1]
            q_hat, below = min(hrefs.edge(j, lo, hi, n_bins), srt[s, -1]), hrefs.edge(j - 1, lo, hi, n_bins)
            print("start %d q=%.2f: %.17g <= x_(k)=%.17g <= q_hat=%.17g" % (s, q, below, x, q_hat))
            assert out["quantiles"][s, i] == q_hat and below <= x <= q_hat
    assert np.array_equal(out["quantiles"][:, -1], srt[:, -1])                  # q = 1 is the max itself
    qmap = ds.noisy_cost_quantile_map(8, q=(0.5, 1.0), n_bins=4, seed=6)
    assert qmap["quantiles"].shape == (9, 9, 2) and qmap["hist"].shape == (9, 9, 6) and qmap["mean"].shape == (9, 9)
    assert np.array_equal(qmap["quantiles"][:, :, 1], qmap["max"]) and np.all(qmap["hist"].sum(axis=2) == 8)


# ---- 6. validation with a device -----------------------------------------------------------------------------------------------------
def test_validation_with_a_device(built):
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(3600)
    knots, labels, ut, base, A, B, c = _problem(rng, 3, 2, np.int32, 9, 5)
    ns, M, n_bins = 11, 6, 5
    X0 = _starts(rng, knots, ns)
    planes = rng.integers(0, 5, size=6)
    off, p = rng.uniform(-0.2, 0.2, size=(3, 5)), rng.uniform(0.1, 1.0, size=5)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        lib, h = ro.lib, ro._ro
        err = lambda: lib.hjb_rollout_last_error(h).decode()
        with pytest.raises(hjbdp.HjbError) as ei:                               # no model yet
            ro.run_campaign(X0, planes, M, hist=(0.0, 1.0, n_bins))
        assert ei.value.status == _abi.HJB_E_INVALID and "hjb_rollout_set_model" in str(ei.value)
        ro.set_model(A, B, c=c, q=[1, 1, 1])
        with pytest.raises(hjbdp.HjbError) as ei:                               # a model, no noise
            ro.run_campaign(X0, planes, M, hist=(0.0, 1.0, n_bins))
        assert ei.value.status == _abi.HJB_E_INVALID and "before hjb_rollout_set_noise" in str(ei.value)
        ro.set_noise(off, p)
        good = ro.run_campaign(X0, planes, M, seed=4, hist=(0.0, 1.0, n_bins))
        Xc = np.ascontiguousarray(X0.T)
        ps = np.ascontiguousarray(planes, dtype=np.int32)
        pp = ps.ctypes.data_as(C.POINTER(C.c_int32))
        K = len(ps)
        Xn = Xc.copy()
        Xn[7, 2] = np.inf
        lo, hi = np.zeros(ns), np.ones(ns)
        edit = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]])
        bad_tol = np.array([0.4, np.nan, 0.4])
        for call, text in ((dict(first=-1), "first_stream=-1 < 0"), (dict(M=0), "n_samples=0 < 1"), (dict(method=7), "method 7"),
                           (dict(K=-1), "n_steps=-1"), (dict(ns=-2), "n_traj=-2"), (dict(pl=None), "null plane_of_step"),
                           (dict(X=dp(Xn)), "not finite"), (dict(X=None), "null X0"), (dict(tol=dp(bad_tol)), "tol[1]"),
                           (dict(stats=None), "null stats"),
                           (dict(nb=0), "n_bins=0 not in 1..256"), (dict(nb=257), "n_bins=257 not in 1..256"), (dict(nb=-3), "n_bins=-3"),
                           (dict(lo=None), "null lo / hi / hist"), (dict(hi=None), "null lo / hi / hist"), (dict(hist=None), "null lo / hi / hist"),
                           (dict(lo=dp(edit(lo, 3, np.nan))), "lo[3]"), (dict(hi=dp(edit(hi, 9, np.inf))), "hi[9]"),
                           (dict(lo=dp(edit(lo, 0, -np.inf))), "lo[0]"), (dict(lo=dp(edit(lo, 5, 1.0))), "lo[5] = 1 is not below hi[5] = 1"),
                           (dict(lo=dp(edit(lo, 6, 2.0))), "is not below"), (dict(hi=dp(edit(hi, 2, 5e-324)), nb=256), "is not finite")):
            stats = np.full(ns * 8, 7.25)
            hist = np.full(ns * 258, -7, dtype=np.int64)
            ms = C.c_double(7.25)
            hist_p = hist.ctypes.data_as(C.POINTER(C.c_int64)) if "hist" not in call else None
            st = lib.hjb_rollout_run_campaign_hist(h, call.get("method", 1), call.get("K", K), call.get("pl", pp), call.get("ns", ns),
                                                   call.get("M", M), call.get("X", dp(Xc)), 4, call.get("first", 0), None,
                                                   call.get("tol", None), call.get("lo", dp(lo)), call.get("hi", dp(hi)), call.get("nb", n_bins),
                                                   call.get("stats", dp(stats)), hist_p, C.byref(ms))
            assert st == _abi.HJB_E_INVALID and text in err(), (call, err())
            assert np.all(stats == 7.25) and np.all(hist == -7) and ms.value == 7.25, call
        again = ro.run_campaign(X0, planes, M, seed=4, hist=(0.0, 1.0, n_bins))
        assert np.array_equal(again["hist"], good["hist"]) and np.array_equal(_bits(again["stats"]), _bits(good["stats"]))
        assert again["device_ms"] > 0
        none = ro.run_campaign(np.zeros((3, 0)), planes, M, hist=(0.0, 1.0, n_bins))      # no starts: no work
        assert none["stats"].shape == (0, 8) and none["hist"].shape == (0, n_bins + 2) and none["device_ms"] == 0.0
        # the plain call is untouched by the histogram call before it
        plain = ro.run_campaign(X0, planes, M, seed=4)
        assert np.array_equal(_bits(plain["stats"]), _bits(good["stats"])) and "hist" not in plain
