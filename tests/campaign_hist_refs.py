"""numpy restatement of the campaign histogram's contract (include/hjbdp.h "campaign cost histograms"; csrc/hjbdp_campaign.h
campaign_bin), independent of the library: the bin of a cost, a start's record, the quantile estimator's bin and its edges.
Every operation is an IEEE double operation rounded once, as the contract states them."""
import math

import numpy as np


def bin_of(c, lo, hi, n_bins):
    """record index of one cost: 0 underflow, 1 .. n_bins the bins, n_bins + 1 overflow (a NaN lands there)"""
    c, lo, hi = np.float64(c), np.float64(lo), np.float64(hi)
    if c < lo:
        return 0
    if not c < hi:
        return n_bins + 1
    scale = np.float64(n_bins) / (hi - lo)
    b = (c - lo) * scale                                                        # the difference and the product each rounded
    return 1 + min(n_bins - 1, int(b))


def hist_of(cost, n_samples, lo, hi, n_bins):
    """[n_starts, n_bins + 2] int64 of cost [n_starts * n_samples]; lo, hi scalars or [n_starts]"""
    c = np.asarray(cost, dtype=np.float64).reshape(-1, n_samples)
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64).reshape(-1), (c.shape[0],))
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64).reshape(-1), (c.shape[0],))
    out = np.zeros((c.shape[0], n_bins + 2), dtype=np.int64)
    for s in range(c.shape[0]):
        for v in c[s]:
            out[s, bin_of(v, lo[s], hi[s], n_bins)] += 1
    return out


def rank_of(q, M):
    return max(1, math.ceil(q * M))


def quantile_column(row, q):
    """the first column of one record whose cumulative count, the underflow counted first, reaches the rank of q"""
    k = rank_of(q, int(row.sum()))
    cum = 0
    for j, n in enumerate(row):
        cum += int(n)
        if cum >= k:
            return j
    raise AssertionError("the record sums to less than the rank")


def edge(j, lo, hi, n_bins):
    """the upper edge of column j (the lower edge of column j + 1): lo + j * (hi - lo) / n_bins, hi itself at j = n_bins"""
    lo, hi = np.float64(lo), np.float64(hi)
    return hi if j == n_bins else lo + np.float64(j) * (hi - lo) / np.float64(n_bins)


def exact_range(cost, n_samples):
    """every start's [min, nextafter(max, +inf)]: the range the two-pass methods bin with"""
    c = np.asarray(cost, dtype=np.float64).reshape(-1, n_samples)
    return c.min(axis=1), np.nextafter(c.max(axis=1), np.inf)
