"""CPU tests of the campaign histogram's host side (include/hjbdp.h "campaign cost histograms"; no GPU): the host reduce
hjbdp.campaign_hist_reduce against the numpy restatement of the bin rule (campaign_hist_refs.py) with costs placed on and beside
every edge, its refusals, and the bracketing of hjbdp.campaign_quantiles and the bin-width bound of hjbdp.campaign_tail_mean.

The quantile bracket.  For the rank k = ceil(q M) the estimator returns the upper edge q_hat of the first bin whose cumulative
count reaches k, so the k-th order statistic x_(k) lies in that bin: q_hat - width <= x_(k) <= q_hat.  That follows from the
estimator's definition and takes no tolerance.  The lower end is evaluated as the bin's lower edge by the edge formula itself,
lo + (j - 1) * (hi - lo) / n_bins - the same number as q_hat - width in exact arithmetic, without the cancellation of a computed
q_hat against a computed width (which at j = 1, where x_(1) = lo exactly, would be off lo by a rounding half the time)."""
import numpy as np
import pytest

import campaign_hist_refs as refs

BINS = (1, 2, 3, 64, 256)
RANGES = ((0.0, 1.0), (60.0, 60.0 + 1e-9), (-3.0, 1e12))


@pytest.fixture(scope="module")
def hjbdp(built):
    import hjbdp
    return hjbdp


def _edge_costs(lo, hi, n_bins):
    c = [lo, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), hi, np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf),
         np.inf, -np.inf, np.nan, 0.5 * (lo + hi)]
    for j in range(1, n_bins):                                                  # every interior edge and both of its neighbours
        e = refs.edge(j, lo, hi, n_bins)
        c += [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)]
    return np.array(c, dtype=np.float64)


@pytest.mark.parametrize("n_bins", BINS)
@pytest.mark.parametrize("rng", RANGES)
def test_the_host_reduce_is_the_bin_rule_on_and_beside_every_edge(hjbdp, n_bins, rng):
    lo, hi = rng
    c = _edge_costs(lo, hi, n_bins)
    M = c.size
    got = hjbdp.campaign_hist_reduce(np.concatenate([c, c[::-1]]), M, lo, hi, n_bins)
    want = refs.hist_of(c, M, lo, hi, n_bins)
    assert got.dtype == np.int64 and got.shape == (2, n_bins + 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[0])  # the order of the samples changes no count
    assert got.sum(axis=1).tolist() == [M, M]
    # lo itself is in bin 1, the double below it under; hi itself, +inf and the NaN are over, the double below hi in the last bin
    one = lambda v: int(np.argmax(hjbdp.campaign_hist_reduce([v], 1, lo, hi, n_bins)[0]))
    assert one(lo) == 1 and one(np.nextafter(lo, -np.inf)) == 0 and one(-np.inf) == 0
    assert one(hi) == n_bins + 1 and one(np.inf) == n_bins + 1 and one(np.nan) == n_bins + 1
    assert one(np.nextafter(hi, -np.inf)) == n_bins


@pytest.mark.parametrize("n_bins", BINS)
def test_minus_zero_at_lo_zero_is_in_the_first_bin(hjbdp, n_bins):
    got = hjbdp.campaign_hist_reduce([-0.0, 0.0], 2, 0.0, 1.0, n_bins)
    assert got[0, 1] == 2 and got.sum() == 2


def test_a_product_that_rounds_up_to_n_bins_stays_in_the_last_bin(hjbdp):
    """c < hi but (c - lo) * scale rounds to n_bins (or above): the min() of the rule keeps it in bin n_bins, not the overflow"""
    found = 0
    cases = [(0.0, 1.0, 3), (-3.0, 1e12, 3), (60.0, 60.0 + 1e-9, 64), (0.3, 1.7, 131), (0.3, 1.7, 181), (0.0, 1e12, 124), (0.3, 1.0, 181),
             (1.0, 1e12 + 1.0, 147)]
    for lo, hi, n_bins in cases:
        c = np.nextafter(hi, -np.inf)
        b = (np.float64(c) - np.float64(lo)) * (np.float64(n_bins) / (np.float64(hi) - np.float64(lo)))
        found += int(b >= n_bins)
        assert refs.bin_of(c, lo, hi, n_bins) == n_bins
        got = hjbdp.campaign_hist_reduce([c], 1, lo, hi, n_bins)
        assert got[0, n_bins] == 1 and got[0, n_bins + 1] == 0, (lo, hi, n_bins, b)
    assert found >= 4, "no case of the list rounds up to n_bins: the test would show nothing"


def test_refusals(hjbdp):
    ok = ([1.0, 2.0], 2, 0.0, 3.0, 4)
    assert hjbdp.campaign_hist_reduce(*ok).sum() == 2
    lib = hjbdp.load_library()
    import ctypes as C
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    cost, lo, hi = np.array([1.0, 2.0]), np.array([0.0]), np.array([3.0])

    def call(n_starts=1, n_samples=2, cost=cost, lo=lo, hi=hi, n_bins=4, hist="own"):
        h = np.full(n_bins + 2 if 0 < n_bins <= 256 else 8, -7, dtype=np.int64)
        st = lib.hjb_rollout_campaign_hist_reduce(n_starts, n_samples, None if cost is None else f64(cost), None if lo is None else f64(lo),
                                                  None if hi is None else f64(hi), n_bins, None if hist is None else i64(h))
        return st, h

    st, h = call()
    assert st == 0 and h.tolist() == [0, 0, 1, 1, 0, 0]
    bad = [dict(n_bins=0), dict(n_bins=-1), dict(n_bins=257), dict(lo=None), dict(hi=None), dict(hist=None), dict(cost=None),
           dict(lo=np.array([np.nan])), dict(hi=np.array([np.inf])), dict(lo=np.array([-np.inf])), dict(hi=np.array([np.nan])),
           dict(lo=np.array([3.0])), dict(lo=np.array([4.0])),                  # !(lo < hi)
           dict(lo=np.array([0.0]), hi=np.array([5e-324]), n_bins=256),         # a scale that is not finite
           dict(n_samples=0), dict(n_starts=-1)]
    for kw in bad:
        st, h = call(**kw)
        assert st != 0, kw
        assert np.all(h == -7), kw                                              # the output untouched
    st, h = call(n_starts=0)
    assert st == 0 and np.all(h == -7)                                          # n_starts = 0 is HJB_OK and writes nothing
    for kw in (dict(lo=np.nan), dict(hi=np.inf), dict(lo=3.0), dict(n_bins=0), dict(n_bins=257)):
        args = dict(cost=[1.0, 2.0], n_samples=2, lo=0.0, hi=3.0, n_bins=4)
        args.update(kw)
        with pytest.raises((hjbdp.HjbError, ValueError)):
            hjbdp.campaign_hist_reduce(**args)


@pytest.mark.parametrize("M", (1, 2, 100))
@pytest.mark.parametrize("n_bins", (1, 64))
def test_quantiles_bracket_the_order_statistic(hjbdp, M, n_bins):
    rng = np.random.default_rng(1000 * M + n_bins)
    ns = 7
    cost = np.exp(rng.normal(size=(ns, M)) * 2.0) * np.array([1e-3, 1.0, 60.0, 1e4, 1e9, 3.0, 0.5])[:, None]
    lo, hi = refs.exact_range(cost, M)
    hist = hjbdp.campaign_hist_reduce(cost, M, lo, hi, n_bins)
    assert np.array_equal(hist, refs.hist_of(cost, M, lo, hi, n_bins))
    assert np.all(hist[:, 0] == 0) and np.all(hist[:, -1] == 0) and np.all(hist.sum(axis=1) == M)      # the range fits exactly
    qs = (0.0, 0.5, 0.95, 0.99, 1.0)
    est = hjbdp.campaign_quantiles(hist, lo, hi, qs)
    assert est.shape == (ns, len(qs))
    srt = np.sort(cost, axis=1)
    for s in range(ns):
        for i, q in enumerate(qs):
            j = refs.quantile_column(hist[s], q)
            x = srt[s, refs.rank_of(q, M) - 1]
            q_hat, below = refs.edge(j, lo[s], hi[s], n_bins), refs.edge(j - 1, lo[s], hi[s], n_bins)
            print("M=%d bins=%d start=%d q=%.2f: %.17g <= x_(k)=%.17g <= q_hat=%.17g" % (M, n_bins, s, q, below, x, q_hat))
            assert est[s, i] == q_hat
            assert below <= x <= q_hat
    # clipped to the campaign's min and max: q = 1 is the max itself
    clipped = hjbdp.campaign_quantiles(hist, lo, hi, qs, cmin=srt[:, 0], cmax=srt[:, -1])
    assert np.array_equal(clipped[:, -1], srt[:, -1])
    assert np.all(clipped <= est) and np.all(clipped >= srt[:, :1])


def test_quantiles_outside_the_range_are_nan_unless_bounded(hjbdp):
    hist = np.array([[3, 1, 0, 2]])                                             # 3 under, bins (1, 0), 2 over; M = 6
    lo, hi = 0.0, 2.0
    est = hjbdp.campaign_quantiles(hist, lo, hi, (0.0, 0.5, 0.6, 0.7, 1.0))
    assert np.isnan(est[0, 0]) and np.isnan(est[0, 1]) and est[0, 2] == 1.0 and np.isnan(est[0, 3]) and np.isnan(est[0, 4])
    est = hjbdp.campaign_quantiles(hist, lo, hi, (0.0, 0.6, 1.0), cmin=-5.0, cmax=9.0)
    assert est[0].tolist() == [-5.0, 1.0, 9.0]
    assert hjbdp.campaign_quantiles(hist[0], lo, hi, 0.6).shape == (1, 1)
    with pytest.raises(ValueError):
        hjbdp.campaign_quantiles(hist, lo, hi, 1.5)


@pytest.mark.parametrize("n_bins", (1, 64))
def test_tail_mean_is_within_one_bin_width(hjbdp, n_bins):
    """every sample of the tail is replaced by the midpoint of its own bin, at most half a width away: so is their mean"""
    rng = np.random.default_rng(5)
    M, ns = 100, 4
    cost = rng.gamma(2.0, 3.0, size=(ns, M))
    lo, hi = refs.exact_range(cost, M)
    hist = hjbdp.campaign_hist_reduce(cost, M, lo, hi, n_bins)
    qs = (0.0, 0.5, 0.95, 1.0)
    est = hjbdp.campaign_tail_mean(hist, lo, hi, qs)
    srt = np.sort(cost, axis=1)
    for s in range(ns):
        for i, q in enumerate(qs):
            exact = srt[s, refs.rank_of(q, M) - 1:].mean()
            assert abs(est[s, i] - exact) <= (hi[s] - lo[s]) / n_bins, (s, q, est[s, i], exact)
    assert np.isnan(hjbdp.campaign_tail_mean(np.array([[0, 1, 1, 1]]), 0.0, 1.0, 0.5)[0, 0])     # a tail sample in the overflow
