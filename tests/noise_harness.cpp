// noise_harness.cpp - csrc/hjbdp_noise.h compiled as plain C++ (tests/test_rollout_noisy_abi.py): the header the K25 kernel and the
// host twins include, without HIP.  Prints
//   three lines "kat <c0..c3> <k0 k1> -> <four words>": Philox4x32-10 on the three known-answer inputs;
//   "block: ok"   noise_block(seed, s, b) is Philox((lo s, hi s, b, 0), (lo seed, hi seed)) and noise_next_word hands out words 0..3;
//   "search: ok"  noise_node (the binary search) equals the count it is defined as, for every table size 1..128 on tables with
//                 runs of equal thresholds, zeros at the front and 2^32 at the end, at the thresholds, beside them and at both ends;
//   "table: ok"   noise_table on (1/4, 1/2, 1/4) is exactly (2^30, 3 * 2^30), a trailing zero weight gives 2^32, null weights
//                 give floor(2^32 (w + 1) / W).
#include <cstdio>
#include <vector>

#include "hjbdp_noise.h"

using namespace hjb;

static int fails = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            if (++fails < 10) printf("  line %d: %s\n", __LINE__, #c); \
        }                                                              \
    } while (0)

static int count_le(const std::vector<double> &T, uint32_t word) {
    int n = 0;
    for (double t : T) n += t <= (double)word;
    return n;
}

int main() {
    const uint32_t in[3][6] = {{0u, 0u, 0u, 0u, 0u, 0u},
                               {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                               {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
    for (const auto &v : in) {
        uint32_t c[4] = {v[0], v[1], v[2], v[3]};
        philox4x32_10(c, v[4], v[5]);
        printf("kat %08x %08x %08x %08x / %08x %08x -> %08x %08x %08x %08x\n", v[0], v[1], v[2], v[3], v[4], v[5], c[0], c[1], c[2], c[3]);
    }

    fails = 0;
    {
        const uint64_t seed = 0x299f31d0a4093822ull, s = 0x85a308d3243f6a88ull;
        uint32_t r[4], c[4] = {0x243f6a88u, 0x85a308d3u, 7u, 0u};
        noise_block(seed, s, 7u, r);
        philox4x32_10(c, 0xa4093822u, 0x299f31d0u);
        const uint32_t want[4] = {c[0], c[1], c[2], c[3]};
        for (int j = 0; j < 4; ++j) CHECK(noise_next_word(r) == want[j]);
    }
    printf("block: %s\n", fails ? "FAILED" : "ok");

    fails = 0;
    uint64_t lcg = 12345;
    for (int n = 0; n <= 127; ++n) {                       // n thresholds = W - 1
        for (int rep = 0; rep < 8; ++rep) {
            std::vector<double> T(n);
            double t = 0.0;
            for (int w = 0; w < n; ++w) {
                lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
                const unsigned kind = (unsigned)(lcg >> 60);
                if (kind >= 6) t += (double)((lcg >> 20) % ((4294967296ull - (uint64_t)t) / (unsigned)(n - w) + 1));    // else: a run of equal values
                if (rep == 7 && w >= n - 2) t = 4294967296.0;
                T[w] = t;
            }
            CHECK(noise_node(T.data(), n, 0u) == count_le(T, 0u));
            CHECK(noise_node(T.data(), n, 0xffffffffu) == count_le(T, 0xffffffffu));
            for (int w = 0; w < n; ++w)
                for (int d = -1; d <= 1; ++d) {
                    const double v = T[w] + d;
                    if (v < 0 || v > 4294967295.0) continue;
                    CHECK(noise_node(T.data(), n, (uint32_t)v) == count_le(T, (uint32_t)v));
                }
        }
    }
    printf("search: %s\n", fails ? "FAILED" : "ok");

    fails = 0;
    {
        const double p[3] = {0.25, 0.5, 0.25}, z[3] = {1.0, 1.0, 0.0};
        double T[127];
        CHECK(noise_table(3, p, T) == 1.0 && T[0] == 1073741824.0 && T[1] == 3221225472.0);
        CHECK(noise_table(3, z, T) == 2.0 && T[0] == 2147483648.0 && T[1] == 4294967296.0);
        CHECK(noise_node(T, 2, 0xffffffffu) == 1);
        CHECK(noise_table(128, nullptr, T) == 128.0);
        for (int w = 0; w < 127; ++w) CHECK(T[w] == (double)(w + 1) * 33554432.0);
        CHECK(noise_table(1, nullptr, T) == 1.0 && noise_node(T, 0, 123u) == 0);
    }
    printf("table: %s\n", fails ? "FAILED" : "ok");
    return 0;
}
