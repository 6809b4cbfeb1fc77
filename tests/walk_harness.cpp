// walk_harness.cpp - host check of the grid-stride walk's integer arithmetic (csrc/hjbdp_walk.h), compiled as plain C++ by
// tests/test_walk_arithmetic.py.  Prints one line per check and returns the number of checks that failed.
//   walk_harness             the library's own xcd_share and launch_spans
//   walk_harness --mutants   the same checks on deliberately wrong copies: every one of them must be REJECTED (the line says so)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hjbdp_walk.h"

typedef unsigned (*share_fn)(unsigned, unsigned);
typedef int64_t (*spans_fn)(int64_t, int64_t);

// For every G in 1 .. 8200: b -> f(b, G) is a permutation of [0, G), and the values of one XCD's workgroups (b % 8 == x) form one
// contiguous range.  -> the first G that violates either (0: none); *what says which.
static unsigned check_share(share_fn f, const char **what) {
    std::vector<unsigned char> seen;
    for (unsigned G = 1; G <= 8200; ++G) {
        seen.assign(G, 0);
        for (unsigned b = 0; b < G; ++b) {
            const unsigned v = f(b, G);
            if (v >= G) { *what = "a value outside [0, G)"; return G; }
            if (seen[v]) { *what = "a value taken twice"; return G; }
            seen[v] = 1;
        }
        for (unsigned x = 0; x < 8 && x < G; ++x) {
            unsigned lo = ~0u, hi = 0, cnt = 0;
            for (unsigned b = x; b < G; b += 8) {
                const unsigned v = f(b, G);
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
                ++cnt;
            }
            if (hi - lo + 1 != cnt) { *what = "an XCD's share is not contiguous"; return G; }
        }
    }
    return 0;
}

static bool spans_ok(spans_fn f, int64_t work, int64_t cap) {
    const int64_t g = f(work, cap), spans = (work + cap - 1) / cap;
    if (work <= cap) return g == work;
    return g % 8 == 0 && g <= cap && g * spans >= work && g * spans - work < 8 * spans;
}

// caps 4096, 2^18, 2^20: every work in 1 .. 3 * 4096 (at every cap), every work within 64 of a multiple of the cap up to 40 caps, and
// a seeded sample of 200,000 larger values up to 2^36.  -> the first work that violates (0: none); *cap_out its cap.
static int64_t check_spans(spans_fn f, int64_t *cap_out) {
    const int64_t caps[3] = {4096, (int64_t)1 << 18, (int64_t)1 << 20};
    for (int64_t cap : caps) {
        *cap_out = cap;
        for (int64_t w = 1; w <= 3 * 4096; ++w)
            if (!spans_ok(f, w, cap)) return w;
        for (int64_t k = 1; k <= 40; ++k)
            for (int64_t d = -64; d <= 64; ++d)
                if (!spans_ok(f, k * cap + d, cap)) return k * cap + d;
        uint64_t s = 0x9e3779b97f4a7c15ull ^ (uint64_t)cap;           // (splitmix64: the sample is the same on every machine)
        for (int i = 0; i < 200000; ++i) {
            s += 0x9e3779b97f4a7c15ull;
            uint64_t z = s;
            z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
            z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
            z ^= z >> 31;
            const int64_t w = 1 + (int64_t)(z >> (28 + (z & 31)));    // magnitudes from 2^5 to 2^36
            if (!spans_ok(f, w, cap)) return w;
        }
    }
    return 0;
}

// ---- the wrong copies ----------------------------------------------------------------------------------------------------------------
static unsigned share_no_remainder(unsigned b, unsigned G) {           // the `x < r` term dropped
    const unsigned x = b & 7u, q = G >> 3;
    return x * q + (b >> 3);
}
static unsigned share_remainder_last(unsigned b, unsigned G) {         // the extra workgroups given to the LAST XCDs' shares
    const unsigned x = b & 7u, q = G >> 3, r = G & 7u;
    return x * q + (x >= 8u - r ? x - (8u - r) : 0u) + (b >> 3);
}
static unsigned share_identity(unsigned b, unsigned) { return b; }     // a permutation, but no XCD's share is contiguous
static int64_t spans_not_rounded(int64_t work, int64_t cap) {          // no multiple of 8
    if (work <= cap) return work;
    const int64_t spans = (work + cap - 1) / cap;
    return (work + spans - 1) / spans;
}
static int64_t spans_cap(int64_t work, int64_t cap) { return work <= cap ? work : cap; }      // a short last span
static int64_t spans_floor(int64_t work, int64_t cap) {                // rounded DOWN to a multiple of 8: one span more
    if (work <= cap) return work;
    const int64_t spans = (work + cap - 1) / cap;
    return work / spans / 8 * 8;
}

int main(int argc, char **argv) {
    int failed = 0;
    const char *what = "";
    int64_t cap = 0;
    if (argc > 1 && !strcmp(argv[1], "--mutants")) {
        const struct { const char *name; share_fn f; } sm[] = {{"share_no_remainder", share_no_remainder},
                                                               {"share_remainder_last", share_remainder_last},
                                                               {"share_identity", share_identity}};
        for (const auto &m : sm) {
            const unsigned G = check_share(m.f, &what);
            printf("%s: %s\n", m.name, G ? "REJECTED" : "accepted");
            if (G) printf("  G = %u: %s\n", G, what);
            failed += G ? 0 : 1;
        }
        const struct { const char *name; spans_fn f; } pm[] = {{"spans_not_rounded", spans_not_rounded}, {"spans_cap", spans_cap},
                                                               {"spans_floor", spans_floor}};
        for (const auto &m : pm) {
            const int64_t w = check_spans(m.f, &cap);
            printf("%s: %s\n", m.name, w ? "REJECTED" : "accepted");
            if (w) printf("  work = %lld, cap = %lld\n", (long long)w, (long long)cap);
            failed += w ? 0 : 1;
        }
        return failed;
    }
    const unsigned G = check_share(hjb::xcd_share, &what);
    printf("xcd_share: %s\n", G ? "FAILED" : "ok");
    if (G) { printf("  G = %u: %s\n", G, what); ++failed; }
    const int64_t w = check_spans(hjb::launch_spans, &cap);
    printf("launch_spans: %s\n", w ? "FAILED" : "ok");
    if (w) { printf("  work = %lld, cap = %lld -> %lld\n", (long long)w, (long long)cap, (long long)hjb::launch_spans(w, cap)); ++failed; }
    return failed;
}
