// campaign_pair_harness.cpp - csrc/hjbdp_campaign.h's paired difference (campaign_pair_diff, campaign_pair_start) as plain C++ (no
// HIP): its own checks of the difference and its flags, then the difference records of a fixed family of inputs printed as hex
// words for tests/test_campaign_pair_refs.py to compare with the numpy restatement (tests/campaign_pair_refs.py, harness_inputs),
// which builds the same inputs.  Exit status 0 and a line "<name>: ok" per check; a failed check prints what it saw and exits 1.
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

static double cost_a_of(int s, long long m) { return (double)((m * 37 + s * 11) % 101) / 8.0 - 3.0; }
static double cost_b_of(int s, long long m) { return m % 5 == 0 ? cost_a_of(s, m) : (double)((m * 29 + s * 5) % 103) / 8.0 - 3.0; }
static unsigned char left_a_of(int s, long long m) { return (unsigned char)((m * 5 + s) % 7 == 0); }
static unsigned char left_b_of(int s, long long m) { return (unsigned char)((m * 3 + s) % 11 == 0); }

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // d = c_B - c_A: negative where B paid less
    if (campaign_pair_diff(3.0, 1.0) != -2.0 || campaign_pair_diff(1.0, 3.0) != 2.0 || bits(campaign_pair_diff(1.5, 1.5)) != 0)
        return fail("diff", 0, 0);
    if (!std::isnan(campaign_pair_diff(inf, inf)) || campaign_pair_diff(1.0, inf) != inf || campaign_pair_diff(inf, 1.0) != -inf)
        return fail("diff", 1, 0);
    std::printf("diff: ok\n");

    // one sample: the flags and the record; a NaN d is neither lower, a null left array means none left
    {
        const double ca[1] = {2.0}, cb[1] = {0.5}, cn[1] = {nan};
        const unsigned char yes[1] = {1}, no[1] = {0};
        double out[8];
        campaign_pair_start(1, ca, cb, nullptr, nullptr, out);
        if (out[0] != -1.5 || out[1] != 2.25 || out[2] != -1.5 || out[3] != -1.5 || out[4] != 1 || out[5] != 0 || out[6] != 1 || out[7] != -1.5)
            return fail("flags", 0, 0);
        campaign_pair_start(1, cb, ca, yes, no, out);
        if (out[0] != 1.5 || out[4] != 0 || out[5] != 1 || out[6] != 0 || bits(out[7]) != 0) return fail("flags", 1, 0);
        campaign_pair_start(1, ca, cb, no, yes, out);
        if (out[6] != 0 || bits(out[7]) != 0) return fail("flags", 2, 0);
        campaign_pair_start(1, ca, cn, no, no, out);
        if (!std::isnan(out[0]) || out[4] != 0 || out[5] != 0 || out[6] != 1) return fail("flags", 3, 0);
        campaign_pair_start(1, ca, ca, nullptr, no, out);
        if (bits(out[0]) != 0 || out[4] != 0 || out[5] != 0 || out[2] != 0.0 || out[3] != 0.0) return fail("flags", 4, 0);
    }
    std::printf("flags: ok\n");

    // the family the restatement's test rebuilds: three starts
    for (long long M : {1LL, 2LL, 3LL, 5LL, 63LL, 64LL, 65LL, 200LL}) {
        for (int s = 0; s < 3; ++s) {
            std::vector<double> ca((size_t)M), cb((size_t)M);
            std::vector<unsigned char> la((size_t)M), lb((size_t)M);
            for (long long m = 0; m < M; ++m) {
                ca[(size_t)m] = cost_a_of(s, m);
                cb[(size_t)m] = cost_b_of(s, m);
                la[(size_t)m] = left_a_of(s, m);
                lb[(size_t)m] = left_b_of(s, m);
            }
            double out[8];
            campaign_pair_start(M, ca.data(), cb.data(), la.data(), lb.data(), out);
            std::printf("stats %lld %d", M, s);
            for (int j = 0; j < 8; ++j) std::printf(" %016llx", bits(out[j]));
            std::printf("\n");
        }
    }
    return 0;
}
