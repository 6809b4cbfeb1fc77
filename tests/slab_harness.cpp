// slab_harness.cpp - host check of the multi-GPU partition's integer arithmetic (csrc/hjbdp_slab.h), compiled as plain C++ by
// tests/test_slab_arithmetic.py.  Every last-axis length nl in 1 .. 64, every number of slabs in 1 .. nl, every (need_lo, need_hi)
// in 0 .. 4 x 0 .. 4.  Prints one line per rule set and returns the number of checks that failed.
//   slab_harness             the library's own rules
//   slab_harness --mutants   the same checks on deliberately wrong copies: every one of them must be REJECTED (the line says so)
//   slab_harness --ranges    "nl world b0:e0 b1:e1 ..." for every nl and world: the test compares them with hjbdp.sharded.partition
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "hjbdp_slab.h"

using namespace hjb;

struct Rules {
    SlabRange (*range)(int, int, int);
    SlabHalo (*halo)(int, int, int, int, int);
    SlabSplit (*split)(int, int, int, int, SlabHalo, bool, int);
    bool (*cover)(const SlabSplit &, int, int);
};

static char g_where[256];
static const char *at(const char *what, int nl, int world, int k, int need_lo, int need_hi) {
    snprintf(g_where, sizeof g_where, "%s (nl = %d, world = %d, slab %d, need %d/%d)", what, nl, world, k, need_lo, need_hi);
    return g_where;
}

// -> nullptr: every rule holds; else the first violation
static const char *check(const Rules &R) {
    for (int nl = 1; nl <= 64; ++nl)
        for (int world = 1; world <= nl; ++world) {
            // the ranges tile [0, nl) in order; sizes nl / world, the first nl % world one longer
            int b = 0;
            for (int k = 0; k < world; ++k) {
                const SlabRange r = R.range(nl, world, k);
                if (r.begin != b) return at("the ranges do not tile the axis in order", nl, world, k, 0, 0);
                if (r.end - r.begin != nl / world + (k < nl % world ? 1 : 0)) return at("a slab's size is not the balanced one, longer slabs first", nl, world, k, 0, 0);
                b = r.end;
            }
            if (b != nl) return at("the ranges do not end at nl", nl, world, world - 1, 0, 0);
            for (int need_lo = 0; need_lo <= 4; ++need_lo)
                for (int need_hi = 0; need_hi <= 4; ++need_hi) {
                    bool fits = true;        // every halo is no wider than the slab that supplies it
                    for (int k = 0; k < world; ++k) {
                        const SlabRange r = R.range(nl, world, k);
                        const SlabHalo h = R.halo(need_lo, need_hi, r.begin, r.end, nl);
                        if (h.lo < 0 || h.hi < 0 || r.begin - h.lo < 0 || r.end + h.hi > nl) return at("a halo leaves [0, nl)", nl, world, k, need_lo, need_hi);
                        if (h.lo != (need_lo < r.begin ? need_lo : r.begin) || h.hi != (need_hi < nl - r.end ? need_hi : nl - r.end))
                            return at("a halo is not the need, clipped at the grid's end", nl, world, k, need_lo, need_hi);
                        if (k > 0) { const SlabRange p = R.range(nl, world, k - 1); fits = fits && h.lo <= p.end - p.begin; }
                        if (k + 1 < world) { const SlabRange n = R.range(nl, world, k + 1); fits = fits && h.hi <= n.end - n.begin; }
                        // what the neighbours need of slab k is what they hold as halos
                        const int up = slab_up_needs(need_lo, r.end, k, world), dn = slab_dn_needs(need_hi, r.begin, nl, k);
                        const SlabRange n = R.range(nl, world, k + 1 < world ? k + 1 : k), p = R.range(nl, world, k > 0 ? k - 1 : k);
                        if (up != (k + 1 < world ? R.halo(need_lo, need_hi, n.begin, n.end, nl).lo : 0)) return at("up_needs is not the upper neighbour's low halo", nl, world, k, need_lo, need_hi);
                        if (dn != (k > 0 ? R.halo(need_lo, need_hi, p.begin, p.end, nl).hi : 0)) return at("dn_needs is not the lower neighbour's high halo", nl, world, k, need_lo, need_hi);
                        for (int overlap = 0; overlap <= 1; ++overlap) {
                            const SlabSplit s = R.split(need_lo, need_hi, r.begin, r.end, h, overlap != 0, world);
                            const int lo_w = h.lo ? need_lo : 0, hi_w = h.hi ? need_hi : 0, owned = r.end - r.begin;
                            const bool want = overlap && world > 1 && owned - lo_w - hi_w >= 1 && (lo_w || hi_w);
                            if (s.split && owned - lo_w - hi_w < 1) return at("a slab without an interior plane splits", nl, world, k, need_lo, need_hi);
                            if (s.split != want || s.split != s.part[0].on) return at("the split decision", nl, world, k, need_lo, need_hi);
                            if (!s.split) {
                                if (s.part[1].on || s.part[2].on || s.lo_w || s.hi_w) return at("strips without a split", nl, world, k, need_lo, need_hi);
                            } else {
                                if (s.lo_w != lo_w || s.hi_w != hi_w || s.part[1].on != (lo_w > 0) || s.part[2].on != (hi_w > 0))
                                    return at("the strips are not the planes that read a halo", nl, world, k, need_lo, need_hi);
                                // low strip, interior, high strip tile the owned planes
                                int e = r.begin;
                                const int order[3] = {1, 0, 2};
                                for (int i : order) {
                                    const SlabPart &c = s.part[i];
                                    if (!c.on) continue;
                                    if (c.begin != e || c.end <= c.begin) return at("the parts do not tile the slab", nl, world, k, need_lo, need_hi);
                                    e = c.end;
                                    if (c.begin - c.halo_lo < r.begin - h.lo || c.end + c.halo_hi > r.end + h.hi) return at("a part's view leaves the slab's view", nl, world, k, need_lo, need_hi);
                                    if (c.row0 != (c.begin - c.halo_lo) - (r.begin - h.lo)) return at("row0 is not the part's first viewed plane inside the slab's buffer", nl, world, k, need_lo, need_hi);
                                    if (c.own0 != c.begin - r.begin) return at("own0 is not the part's first owned plane", nl, world, k, need_lo, need_hi);
                                }
                                if (e != r.end) return at("the parts do not end at the slab's end", nl, world, k, need_lo, need_hi);
                                const SlabPart &in = s.part[0];
                                if (in.halo_lo != (need_lo < lo_w ? need_lo : lo_w) || in.halo_hi != (need_hi < hi_w ? need_hi : hi_w))
                                    return at("the interior's halos are not min(need, strip width)", nl, world, k, need_lo, need_hi);
                                if ((lo_w && s.part[1].halo_lo != h.lo) || (hi_w && s.part[2].halo_hi != h.hi)) return at("a strip's outer halo is not the slab's", nl, world, k, need_lo, need_hi);
                            }
                            for (int d = 0; d <= 5; ++d)
                                for (int u = 0; u <= 5; ++u) {
                                    const bool cov = s.split && (s.part[1].on || d == 0) && (s.part[2].on || u == 0) && d <= s.lo_w && u <= s.hi_w;
                                    if (R.cover(s, d, u) != cov) return at("strips-cover", nl, world, k, need_lo, need_hi);
                                }
                        }
                    }
                    if ((slab_partition_check(nl, world, need_lo, need_hi) == 0) != fits && R.range == slab_range && R.halo == slab_halo)
                        return at("the partition check disagrees with the halos and the neighbours' sizes", nl, world, 0, need_lo, need_hi);
                }
        }
    return nullptr;
}

// ---- the wrong copies ----------------------------------------------------------------------------------------------------------------
static SlabRange range_remainder_last(int nl, int world, int k) {          // the remainder given to the LAST slabs
    const int base = nl / world, rem = nl % world, first = world - rem;
    const int b = k * base + (k > first ? k - first : 0);
    return {b, b + base + (k >= first ? 1 : 0)};
}
static SlabHalo halo_unclipped(int need_lo, int need_hi, int begin, int end, int nl) {      // the high halo not clipped at the grid's end
    (void)end; (void)nl;
    return {slab_min(need_lo, begin), need_hi};
}
static SlabSplit split_row0_no_halo(int need_lo, int need_hi, int begin, int end, SlabHalo halo, bool overlap, int n_slabs) {
    SlabSplit s = slab_split(need_lo, need_hi, begin, end, halo, overlap, n_slabs);
    for (SlabPart &c : s.part)
        if (c.on) c.row0 = c.begin - (begin - halo.lo);                    // row0 without the part's own halo term
    return s;
}
static SlabSplit split_empty_interior(int need_lo, int need_hi, int begin, int end, SlabHalo halo, bool overlap, int n_slabs) {
    SlabSplit s = slab_split(need_lo, need_hi, begin, end, halo, overlap, n_slabs);
    const int lo_w = halo.lo ? need_lo : 0, hi_w = halo.hi ? need_hi : 0;
    if (!s.split && overlap && n_slabs > 1 && end - begin - lo_w - hi_w >= 0 && (lo_w || hi_w)) {      // `>= 0` for `>= 1`
        s.split = true;
        s.lo_w = lo_w;
        s.hi_w = hi_w;
        s.part[0] = {true, begin + lo_w, end - hi_w, slab_min(need_lo, lo_w), slab_min(need_hi, hi_w), 0, lo_w};
    }
    return s;
}
static bool cover_ignores_dn(const SlabSplit &s, int, int up_needs) { return s.split && up_needs <= s.hi_w; }

int main(int argc, char **argv) {
    const Rules lib = {slab_range, slab_halo, slab_split, slab_strips_cover};
    if (argc > 1 && !strcmp(argv[1], "--ranges")) {
        for (int nl = 1; nl <= 64; ++nl)
            for (int world = 1; world <= nl; ++world) {
                printf("%d %d", nl, world);
                for (int k = 0; k < world; ++k) printf(" %d:%d", slab_range(nl, world, k).begin, slab_range(nl, world, k).end);
                printf("\n");
            }
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "--mutants")) {
        int failed = 0;
        Rules m[5] = {lib, lib, lib, lib, lib};
        const char *names[5] = {"range_remainder_last", "halo_unclipped", "split_row0_no_halo", "split_empty_interior", "cover_ignores_dn"};
        m[0].range = range_remainder_last;
        m[1].halo = halo_unclipped;
        m[2].split = split_row0_no_halo;
        m[3].split = split_empty_interior;
        m[4].cover = cover_ignores_dn;
        for (int i = 0; i < 5; ++i) {
            const char *why = check(m[i]);
            printf("%s: %s\n", names[i], why ? "REJECTED" : "accepted");
            if (why) printf("  %s\n", why);
            failed += why ? 0 : 1;
        }
        return failed;
    }
    const char *why = check(lib);
    printf("slab arithmetic: %s\n", why ? "FAILED" : "ok");
    if (why) printf("  %s\n", why);
    return why ? 1 : 0;
}
