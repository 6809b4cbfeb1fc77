// hjbdp_campaign.h - the per-start statistics of a noisy campaign (K28, kernels_rollout_campaign.h): the slot values of one
// sample, the identities of a padding slot, the adjacent-pair tree of a block and the left-to-right fold of the block partials,
// shared by the kernel, the host reduce hjb_rollout_campaign_reduce (rollout_campaign_host.hip) and tests/campaign_harness.cpp,
// which compiles it as plain C++ (no HIP dependency).  Controller-agnostic: these functions see a sample's cost c, its final
// state xf and whether it left the grid, and nothing of the lookup that flew it.  The contract (stated in include/hjbdp.h):
//   slot values  v0 = c, v1 = c * c (rounded), v2 = c, v3 = c, v7 = settled ? c : +0.0; the flags e (c > threshold, strict),
//                l (some visited state outside [first knot, last knot] on some axis, a NaN counts as outside), t (|xf_a| <= tol_a
//                on every axis); a padding slot holds v0 = v1 = v7 = +0.0, v2 = +inf, v3 = -inf and counts 0;
//   op           sums a + b; min b < a ? b : a; max b > a ? b : a - `a` the earlier operand;
//   blocks       G = min(64, the smallest power of two >= M) consecutive samples of a start, the last block padded; a block's
//                partial is the tree over its G slots: at level L element i (a multiple of 2^(L+1)) becomes op(v[i], v[i + 2^L]);
//   fold         acc = p_0, then acc = op(acc, p_b) in block order.  Counts are integers.
// Nothing here depends on how a launch lays the slots out: the kernel runs the same op over wave shuffles.
//
// The per-start cost histogram (K30, kernels_rollout_campaign_hist.h; hjb_rollout_campaign_hist_reduce): n_bins in
// 1 .. kCampaignMaxBins equal bins between lo[s] < hi[s] (both finite), scale_s = (double)n_bins / (hi[s] - lo[s]) (finite), and a
// record of n_bins + 2 int64 counts per start: index 0 the underflow (c < lo), index n_bins + 1 the overflow (!(c < hi): a NaN
// lands here), otherwise 1 + min(n_bins - 1, (int)((c - lo) * scale)), the difference and the product each rounded
// (campaign_bin, the one function every caller bins with).  Padding slots and lanes past a launch's last block count nothing, so
// a start's record sums to M.
// Why atomics are allowed here: the eight statistics keep their fixed floating-point order.  Integer addition commutes, so integer
// atomics do not break K28's rule: the result is a function of (M, the samples) alone.  That licence covers the integer counts of
// the histogram and nothing else: no double is ever accumulated atomically.
//
// The paired difference of two controllers on one plant (K31, kernels_rollout_campaign_pair.h; hjb_rollout_campaign_pair_reduce):
// sample m of a start is flown by A and by B on the same stream, d = c_B - c_A (one rounded subtraction), and the record of d is
// K28's reduction over campaign_slot(d, t) with the flags e = d < 0 (B paid less), l = d > 0 (A paid less), t = neither flight left
// the grid; a NaN d sets neither e nor l.  Blocks, padding, tree and fold are the ones above: campaign_pair_start calls them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HJB_CAMPAIGN_FN __host__ __device__ __forceinline__
#else
#define HJB_CAMPAIGN_FN inline
#endif

namespace hjb {

constexpr int kCampaignMaxGroup = 64;

// the five values of a slot that the tree combines in double (stats 0, 1, 2, 3 and 7); the counts (stats 4, 5, 6) are integers
struct CampVals {
    double sum, sumsq, mn, mx, sum_settled;
};

struct CampCounts {
    int64_t exceed, left, settled;
};

HJB_CAMPAIGN_FN double campaign_inf() { return __builtin_huge_val(); }

// G and log2 G of n_samples >= 1 samples per start
HJB_CAMPAIGN_FN int campaign_group(int64_t n_samples, int *log2_out) {
    int g = 1, lg = 0;
    while (g < kCampaignMaxGroup && g < n_samples) {
        g *= 2;
        ++lg;
    }
    if (log2_out) *log2_out = lg;
    return g;
}

// The launch geometry of a campaign call and the device bytes it holds (host only; the device loop of rollout_campaign_host.hip
// and tests/campaign_harness.cpp): n_starts >= 1 starts of n_samples >= 1 samples, D axes, n_steps steps, launches of at most
// `chunk` lanes, `records` records of 8 doubles per start (1; the pair's 3) with as many partial arrays, `plane_lists` lists of the
// steps' planes (1; the pair's 2), n_bins bins or 0 for no histogram, the pair scratch and HJB_PAIR_GREEDY's one-node table.
struct CampaignGeometry {
    int G, log2G;                     // campaign_group's
    int64_t B, n_blocks;              // blocks per start, blocks of the call (<= n_starts * n_samples)
    int64_t nb_max, lanes_max;        // blocks and lanes of a launch at most: a launch is never smaller than one block
    // bytes: X0, the records, the thresholds, the partials, the plane lists (one entry each at least), the histogram's
    // [lo | hi | scale] and counts, the scratch's one double and one byte per lane of a launch, 16 for the table
    uint64_t need;
};

inline CampaignGeometry campaign_geometry(int64_t n_starts, int64_t n_samples, int D, int32_t n_steps, int64_t chunk, int records,
                                          int plane_lists, bool has_threshold, int n_bins, bool scratch, bool greedy) {
    CampaignGeometry g;
    g.G = campaign_group(n_samples, &g.log2G);
    g.B = (n_samples + g.G - 1) / g.G;
    g.n_blocks = n_starts * g.B;
    const int64_t per_launch = chunk / g.G;
    g.nb_max = per_launch < 1 ? 1 : per_launch;
    if (g.n_blocks < g.nb_max) g.nb_max = g.n_blocks;
    g.lanes_max = g.nb_max * g.G;
    const uint64_t ns = (uint64_t)n_starts, R = (uint64_t)records;
    g.need = 8 * (uint64_t)D * ns + R * 64 * ns + (has_threshold ? 8 * ns : 0) + R * 64 * (uint64_t)g.nb_max +
             (uint64_t)plane_lists * 4 * (uint64_t)(n_steps > 1 ? n_steps : 1) + (n_bins ? 24 * ns + 8 * (uint64_t)(n_bins + 2) * ns : 0) +
             (scratch ? 9 * (uint64_t)g.lanes_max : 0) + (greedy ? 16 : 0);
    return g;
}

HJB_CAMPAIGN_FN CampVals campaign_padding() {
    CampVals v;
    v.sum = 0.0;
    v.sumsq = 0.0;
    v.mn = campaign_inf();
    v.mx = -campaign_inf();
    v.sum_settled = 0.0;
    return v;
}

HJB_CAMPAIGN_FN CampVals campaign_slot(double c, bool settled) {
    CampVals v;
    v.sum = c;
    v.sumsq = c * c;
    v.mn = c;
    v.mx = c;
    v.sum_settled = settled ? c : 0.0;
    return v;
}

// e: has_threshold false = no threshold given
HJB_CAMPAIGN_FN bool campaign_exceeds(double c, bool has_threshold, double threshold) { return has_threshold && c > threshold; }

// one axis of one visited state against that axis' first and last knot; a NaN is outside
HJB_CAMPAIGN_FN bool campaign_outside(double x, double lo, double hi) { return !(lo <= x && x <= hi); }

// t: tol null = none given; |xf_a| <= tol_a on every axis (a NaN xf_a does not settle)
HJB_CAMPAIGN_FN bool campaign_settled(int D, const double *xf, const double *tol) {
    if (!tol) return false;
    bool t = true;
    for (int a = 0; a < D; ++a) t = t && (__builtin_fabs(xf[a]) <= tol[a]);
    return t;
}

// op(a, b), a the earlier operand: what the tree's levels and the fold both apply
HJB_CAMPAIGN_FN CampVals campaign_op(const CampVals &a, const CampVals &b) {
    CampVals v;
    v.sum = a.sum + b.sum;
    v.sumsq = a.sumsq + b.sumsq;
    v.mn = b.mn < a.mn ? b.mn : a.mn;
    v.mx = b.mx > a.mx ? b.mx : a.mx;
    v.sum_settled = a.sum_settled + b.sum_settled;
    return v;
}

// the adjacent-pair tree over v[0 .. G), G a power of two, in place: the partial is v[0] on return
HJB_CAMPAIGN_FN void campaign_tree(CampVals *v, int G) {
    for (int half = 1; half < G; half *= 2)
        for (int i = 0; i + half < G; i += 2 * half) v[i] = campaign_op(v[i], v[i + half]);
}

// The statistics of one start from its n_samples per-trajectory results (cost [M]; xf [D, M] column-major or null; left [M] or
// null; threshold: has_threshold false = none; tol [D] or null) into out[8]: the blocks, their trees and the fold, on one thread.
inline void campaign_reduce_start(int64_t n_samples, int D, const double *cost, const double *xf, const uint8_t *left,
                                  bool has_threshold, double threshold, const double *tol, double *out) {
    const int G = campaign_group(n_samples, nullptr);
    CampVals acc = campaign_padding(), v[kCampaignMaxGroup];
    CampCounts n = {0, 0, 0};
    for (int64_t m0 = 0; m0 < n_samples; m0 += G) {
        for (int j = 0; j < G; ++j) {
            const int64_t m = m0 + j;
            if (m >= n_samples) {
                v[j] = campaign_padding();
                continue;
            }
            const bool t = xf && campaign_settled(D, xf + (int64_t)D * m, tol);
            v[j] = campaign_slot(cost[m], t);
            n.exceed += campaign_exceeds(cost[m], has_threshold, threshold) ? 1 : 0;
            n.left += (left && left[m]) ? 1 : 0;
            n.settled += t ? 1 : 0;
        }
        campaign_tree(v, G);
        acc = m0 == 0 ? v[0] : campaign_op(acc, v[0]);
    }
    out[0] = acc.sum;
    out[1] = acc.sumsq;
    out[2] = acc.mn;
    out[3] = acc.mx;
    out[4] = (double)n.exceed;
    out[5] = (double)n.left;
    out[6] = (double)n.settled;
    out[7] = acc.sum_settled;
}

// ---- the histogram of a start's costs (K30) ----
constexpr int kCampaignMaxBins = 256;

// scale_s of a start's range; the caller refuses one that is not finite (campaign_hist_range_ok)
HJB_CAMPAIGN_FN double campaign_hist_scale(double lo, double hi, int n_bins) { return (double)n_bins / (hi - lo); }

// a start's range as the entry points accept it: lo and hi finite, lo < hi, a finite scale
HJB_CAMPAIGN_FN bool campaign_hist_range_ok(double lo, double hi, int n_bins) {
    const double inf = campaign_inf();
    if (!(lo > -inf && lo < inf && hi > -inf && hi < inf)) return false;
    if (!(lo < hi)) return false;
    const double sc = campaign_hist_scale(lo, hi, n_bins);
    return sc > -inf && sc < inf;
}

// the record index of a sample of cost c: 0 underflow, 1 .. n_bins the bins, n_bins + 1 overflow (a NaN lands there)
HJB_CAMPAIGN_FN int campaign_bin(double c, double lo, double hi, double scale, int n_bins) {
    if (c < lo) return 0;
    if (!(c < hi)) return n_bins + 1;
    const double d = c - lo;
    const double b = d * scale;                               // 0 <= b, and b <= n_bins up to the two roundings
    const int i = (int)b;
    return 1 + (i < n_bins - 1 ? i : n_bins - 1);
}

// one start's record hist[n_bins + 2] from its n_samples costs, on one thread
inline void campaign_hist_start(int64_t n_samples, const double *cost, double lo, double hi, int n_bins, int64_t *hist) {
    const double scale = campaign_hist_scale(lo, hi, n_bins);
    for (int j = 0; j < n_bins + 2; ++j) hist[j] = 0;
    for (int64_t m = 0; m < n_samples; ++m) ++hist[campaign_bin(cost[m], lo, hi, scale, n_bins)];
}

// ---- the paired difference of two controllers' costs (K31) ----
// d of one sample: B's cost less A's, one rounded subtraction (negative: B paid less)
HJB_CAMPAIGN_FN double campaign_pair_diff(double cost_a, double cost_b) { return cost_b - cost_a; }

// The difference record of one start from its n_samples costs under A and under B (cost_a, cost_b [M]; left_a, left_b [M] or null:
// none left) into out[8]: 0 sum d, 1 sum d*d, 2 min d, 3 max d, 4 n(d < 0), 5 n(d > 0), 6 n(both stayed in the grid), 7 sum d over
// those - campaign_reduce_start's blocks, trees and fold over campaign_slot(d, both_in), on one thread.
inline void campaign_pair_start(int64_t n_samples, const double *cost_a, const double *cost_b, const uint8_t *left_a,
                                const uint8_t *left_b, double *out) {
    const int G = campaign_group(n_samples, nullptr);
    CampVals acc = campaign_padding(), v[kCampaignMaxGroup];
    CampCounts n = {0, 0, 0};                                 // exceed: d < 0; left: d > 0; settled: both in
    for (int64_t m0 = 0; m0 < n_samples; m0 += G) {
        for (int j = 0; j < G; ++j) {
            const int64_t m = m0 + j;
            if (m >= n_samples) {
                v[j] = campaign_padding();
                continue;
            }
            const double d = campaign_pair_diff(cost_a[m], cost_b[m]);
            const bool t = !(left_a && left_a[m]) && !(left_b && left_b[m]);
            v[j] = campaign_slot(d, t);
            n.exceed += d < 0 ? 1 : 0;
            n.left += d > 0 ? 1 : 0;
            n.settled += t ? 1 : 0;
        }
        campaign_tree(v, G);
        acc = m0 == 0 ? v[0] : campaign_op(acc, v[0]);
    }
    out[0] = acc.sum;
    out[1] = acc.sumsq;
    out[2] = acc.mn;
    out[3] = acc.mx;
    out[4] = (double)n.exceed;
    out[5] = (double)n.left;
    out[6] = (double)n.settled;
    out[7] = acc.sum_settled;
}

}  // namespace hjb
