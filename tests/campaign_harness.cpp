// campaign_harness.cpp - csrc/hjbdp_campaign.h as plain C++ (no HIP): its own checks of the group size, the identities, the tree's
// pairing and the fold, then the statistics of a fixed family of inputs printed as hex words for
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
