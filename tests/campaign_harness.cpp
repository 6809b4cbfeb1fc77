// campaign_harness.cpp - csrc/hjbdp_campaign.h as plain C++ (no HIP): its own checks of the group size, the launch geometry and
// device bytes of a call (campaign_geometry, against figures worked by hand), the identities, the tree's pairing and the fold, then the statistics of a fixed family of inputs printed as hex words for
// tests/test_campaign_refs.py to compare with the numpy restatement (tests/campaign_refs.py), which builds the same inputs.
// Exit status 0 and a line "<name>: ok" per check; a failed check prints what it saw and exits 1.
#include "hjbdp_campaign.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace hjb;

static int fail(const char *what, long long a, long long b) {
    std::printf("%s: FAILED (%lld, %lld)\n", what, a, b);
    return 1;
}

static unsigned long long bits(double x) {
    unsigned long long u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}

// the tree written the other way round: the partial of [i, i + n) is op(partial of the first half, partial of the second half)
static CampVals halves(const CampVals *v, int n) {
    if (n == 1) return v[0];
    return campaign_op(halves(v, n / 2), halves(v + n / 2, n / 2));
}

// the inputs of sample m of start s, exactly representable: the restatement's test builds the same numbers
static double cost_of(int s, long long m) { return (double)((m * 37 + s * 11) % 101) / 8.0 - 3.0; }
static double xf_of(int s, long long m, int a) { return (double)((m * 13 + s * 7 + a * 5) % 17) / 16.0 - 0.5; }
static unsigned char left_of(int s, long long m) { return (unsigned char)((m * 5 + s) % 7 == 0); }

int main() {
    // the group size
    const long long Ms[] = {1, 2, 3, 4, 5, 8, 9, 33, 63, 64, 65, 200, 1LL << 40};
    const int Gs[] = {1, 2, 4, 4, 8, 8, 16, 64, 64, 64, 64, 64, 64};
    for (int i = 0; i < 13; ++i) {
        int lg = -1;
        const int G = campaign_group(Ms[i], &lg);
        if (G != Gs[i] || (1 << lg) != G) return fail("group", Ms[i], G);
    }
    std::printf("group: ok\n");

    // the launch geometry and the device bytes of a call: D = 2, 3 starts of 100 samples, 5 steps, launches of at most 128 lanes, a
    // threshold.  G = 64 (100 > 64), log2 G = 6, B = ceil(100 / 64) = 2, n_blocks = 3 * 2 = 6, nb_max = min(6, max(128 / 64, 1)) = 2,
    // lanes_max = 2 * 64 = 128.  The bytes, by hand:
    //   X0 8 * 2 * 3 = 48, one record 64 * 3 = 192, the thresholds 8 * 3 = 24, one partial array 64 * 2 = 128, one plane list 4 * 5 = 20
    //   plain  48 + 192 + 24 + 128 + 20                                                             = 412
    //   hist   412 + [lo | hi | scale] 24 * 3 = 72 + counts 8 * (10 + 2) * 3 = 288                   = 772
    //   pair   48 + 3 * 192 + 24 + 3 * 128 + 2 * 20 + scratch 9 * 128 = 1152 + the greedy table 16   = 2240
    {
        const CampaignGeometry p = campaign_geometry(3, 100, 2, 5, 128, 1, 1, true, 0, false, false);
        if (p.G != 64 || p.log2G != 6 || p.B != 2 || p.n_blocks != 6 || p.nb_max != 2 || p.lanes_max != 128) return fail("plan", p.G, p.nb_max);
        if (p.need != 412) return fail("plan", 412, (long long)p.need);
        const CampaignGeometry h = campaign_geometry(3, 100, 2, 5, 128, 1, 1, true, 10, false, false);
        if (h.need != 772 || h.nb_max != 2) return fail("plan", 772, (long long)h.need);
        const CampaignGeometry q = campaign_geometry(3, 100, 2, 5, 128, 3, 2, true, 0, true, true);
        if (q.need != 2240 || q.nb_max != 2 || q.lanes_max != 128) return fail("plan", 2240, (long long)q.need);
        // without the threshold 24 bytes less; no steps still holds one plane entry per list: 412 - 24 - 20 + 4
        if (campaign_geometry(3, 100, 2, 0, 128, 1, 1, false, 0, false, false).need != 372) return fail("plan", 372, 0);
        // a chunk below one block still launches one block; a chunk above the call launches the call's blocks
        const CampaignGeometry c1 = campaign_geometry(3, 100, 2, 5, 1, 1, 1, true, 0, false, false);
        if (c1.nb_max != 1 || c1.lanes_max != 64 || c1.need != 412 - 64) return fail("plan", c1.nb_max, (long long)c1.need);
        if (campaign_geometry(3, 100, 2, 5, 1 << 20, 1, 1, true, 0, false, false).nb_max != 6) return fail("plan", 6, 0);
        const CampaignGeometry m1 = campaign_geometry(3, 1, 2, 5, 128, 1, 1, true, 0, false, false);
        if (m1.G != 1 || m1.log2G != 0 || m1.B != 1 || m1.n_blocks != 3 || m1.nb_max != 3 || m1.lanes_max != 3) return fail("plan", m1.G, m1.B);
        const CampaignGeometry m65 = campaign_geometry(3, 65, 2, 5, 128, 1, 1, true, 0, false, false);
        if (m65.G != 64 || m65.B != 2) return fail("plan", m65.G, m65.B);
    }
    std::printf("plan: ok\n");

    // the identities: op(x, padding) is x bit for bit, whatever x holds, -0.0 and the infinities included
    const double inf = std::numeric_limits<double>::infinity();
    const double probes[] = {0.0, -0.0, 1.5, -2.25, inf, -inf, 1e308, 5e-324};
    for (double c : probes) {
        const CampVals x = campaign_slot(c, true), y = campaign_op(x, campaign_padding());
        // a sum with +0.0 turns -0.0 into +0.0: the contract's rule, not an identity in the bits - every other field is kept
        if (bits(y.mn) != bits(x.mn) || bits(y.mx) != bits(x.mx) || y.sum != x.sum || y.sumsq != x.sumsq || y.sum_settled != x.sum_settled)
            return fail("identity", (long long)bits(c), 0);
    }
    const CampVals pad = campaign_padding();
    if (bits(pad.sum) != 0 || bits(pad.sumsq) != 0 || bits(pad.sum_settled) != 0 || pad.mn != inf || pad.mx != -inf) return fail("identity", -1, -1);
    if (bits(campaign_slot(2.0, false).sum_settled) != 0 || campaign_slot(2.0, true).sum_settled != 2.0) return fail("identity", -2, -2);
    std::printf("identity: ok\n");

    // the flags
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (campaign_exceeds(1.0, true, 1.0) || !campaign_exceeds(1.0 + 1e-15, true, 1.0) || campaign_exceeds(9.0, false, 1.0) ||
        campaign_exceeds(nan, true, 1.0))
        return fail("flags", 0, 0);
    if (campaign_outside(-1.0, -1.0, 1.0) || campaign_outside(1.0, -1.0, 1.0) || !campaign_outside(1.0 + 1e-15, -1.0, 1.0) ||
        !campaign_outside(nan, -1.0, 1.0))
        return fail("flags", 1, 0);
    const double xf[3] = {0.5, -0.25, 0.0}, tol_eq[3] = {0.5, 0.25, 0.0}, tol_lt[3] = {0.5, 0.2, 0.0}, xn[3] = {0.5, nan, 0.0};
    if (!campaign_settled(3, xf, tol_eq) || campaign_settled(3, xf, tol_lt) || campaign_settled(3, xf, nullptr) || campaign_settled(3, xn, tol_eq))
        return fail("flags", 2, 0);
    std::printf("flags: ok\n");

    // the tree pairs adjacent elements: equal to the recursion over halves at every G, on values whose sums do round
    for (int G = 1; G <= 64; G *= 2) {
        std::vector<CampVals> v(G), w;
        for (int j = 0; j < G; ++j) v[j] = campaign_slot(1.0 / (j + 3.0) + (j % 3 == 0 ? 1e10 : 0.0), j % 2 == 0);
        w = v;
        campaign_tree(w.data(), G);
        const CampVals h = halves(v.data(), G);
        if (std::memcmp(&w[0], &h, sizeof h) != 0) return fail("tree", G, 0);
    }
    // a NaN in the first or in the second operand: min and max keep the earlier operand unless the later one compares
    {
        CampVals a = campaign_slot(nan, false), b = campaign_slot(1.0, false);
        const CampVals ab = campaign_op(a, b), ba = campaign_op(b, a);
        if (!std::isnan(ab.mn) || !std::isnan(ab.mx) || ba.mn != 1.0 || ba.mx != 1.0 || !std::isnan(ab.sum) || !std::isnan(ba.sum))
            return fail("tree", -1, 0);
    }
    std::printf("tree: ok\n");

    // the family the restatement's test rebuilds: D = 2, three starts, thresholds and tol given
    const double tol[2] = {0.25, 0.375};
    for (long long M : {1LL, 2LL, 3LL, 5LL, 63LL, 64LL, 65LL, 200LL}) {
        for (int s = 0; s < 3; ++s) {
            std::vector<double> cost((size_t)M), xfin((size_t)(2 * M));
            std::vector<unsigned char> left((size_t)M);
            for (long long m = 0; m < M; ++m) {
                cost[(size_t)m] = cost_of(s, m);
                xfin[(size_t)(2 * m)] = xf_of(s, m, 0);
                xfin[(size_t)(2 * m + 1)] = xf_of(s, m, 1);
                left[(size_t)m] = left_of(s, m);
            }
            double out[8];
            campaign_reduce_start(M, 2, cost.data(), xfin.data(), left.data(), true, 1.0 + s, tol, out);
            std::printf("stats %lld %d", M, s);
            for (int j = 0; j < 8; ++j) std::printf(" %016llx", bits(out[j]));
            std::printf("\n");
        }
    }
    return 0;
}
