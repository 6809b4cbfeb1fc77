// hjbdp_slab.h - the integer arithmetic of the multi-GPU partition: which planes of the LAST state axis a slab owns, which halo
// planes it reads, how a slab divides into an interior and two boundary strips, and what a rank's neighbours need of it.  The one
// statement of each rule for hjb_create_multi and hjb_rank_create (hjbdp_slab.hip builds the handles from it).  No HIP dependency:
// tests/slab_harness.cpp compiles it as plain C++ and checks every rule exhaustively on small grids.
#pragma once
#include <stdint.h>

namespace hjb {

inline int slab_min(int a, int b) { return a < b ? a : b; }

// The balanced contiguous partition of nl planes over `world` slabs: slab k owns [begin, end); the first nl % world slabs are one
// plane longer.
struct SlabRange { int begin, end; };
inline SlabRange slab_range(int nl, int world, int k) {
    const int base = nl / world, rem = nl % world;
    const int b = k * base + slab_min(k, rem);
    return {b, b + base + (k < rem ? 1 : 0)};
}

// A slab's halos: the need_lo planes below `begin` and the need_hi planes above `end` that its stage reads, clipped at the grid's
// ends.  A slab handle sees planes [begin - lo, end + hi).
struct SlabHalo { int lo, hi; };
inline SlabHalo slab_halo(int need_lo, int need_hi, int begin, int end, int nl) {
    return {slab_min(need_lo, begin), slab_min(need_hi, nl - end)};
}

// A halo must come from the immediate neighbour only: no slab's clipped halo is wider than the slab that supplies it.
// -> 0: the partition holds; kSlabLoWide / kSlabHiWide: the first slab's side that does not (*slab: which slab, if wanted).
enum { kSlabLoWide = 1, kSlabHiWide = 2 };
inline int slab_partition_check(int nl, int world, int need_lo, int need_hi, int *slab = nullptr) {
    for (int k = 0; k < world; ++k) {
        const SlabRange r = slab_range(nl, world, k);
        const SlabHalo h = slab_halo(need_lo, need_hi, r.begin, r.end, nl);
        int why = 0;
        if (k > 0) { const SlabRange p = slab_range(nl, world, k - 1); if (h.lo > p.end - p.begin) why = kSlabLoWide; }
        if (!why && k + 1 < world) { const SlabRange n = slab_range(nl, world, k + 1); if (h.hi > n.end - n.begin) why = kSlabHiWide; }
        if (why) { if (slab) *slab = k; return why; }
    }
    return 0;
}

// A slab as interior + boundary strips.  The low strip is the need_lo owned planes whose stage reads the low halo, the high strip
// the need_hi planes that read the high halo; the interior's next states stay inside the owned planes, so it runs while the halos
// travel.  Each part is a slab of its own over the SAME buffers: part k owns [begin, end) and sees halo_lo / halo_hi planes of its
// neighbours in the slab; row0 = first plane of its view inside the slab's haloed buffer, own0 = its first owned plane relative
// to the slab's `begin`.  part[0] interior, part[1] low strip, part[2] high strip (on: the part exists).
struct SlabPart { bool on; int begin, end, halo_lo, halo_hi; int64_t row0, own0; };
struct SlabSplit {
    bool split;          // an interior of at least one plane and at least one strip: part[0].on
    int lo_w, hi_w;      // planes the strips cover (0: no such strip, or no split)
    SlabPart part[3];
};
inline SlabSplit slab_split(int need_lo, int need_hi, int begin, int end, SlabHalo halo, bool overlap, int n_slabs) {
    SlabSplit s{};
    const int lo_w = halo.lo ? need_lo : 0, hi_w = halo.hi ? need_hi : 0, owned = end - begin;
    s.split = overlap && n_slabs > 1 && owned - lo_w - hi_w >= 1 && (lo_w || hi_w);
    if (!s.split) return s;
    s.lo_w = lo_w;
    s.hi_w = hi_w;
    const int view0 = begin - halo.lo;
    auto sub = [&](int k, int sb, int se, int hl, int hh) {
        s.part[k] = {true, sb, se, hl, hh, (int64_t)((sb - hl) - view0), (int64_t)(sb - begin)};
    };
    sub(0, begin + lo_w, end - hi_w, slab_min(need_lo, lo_w), slab_min(need_hi, hi_w));
    if (lo_w) sub(1, begin, begin + lo_w, halo.lo, slab_min(need_hi, end - (begin + lo_w)));
    if (hi_w) sub(2, end - hi_w, end, slab_min(need_lo, (end - hi_w) - begin), halo.hi);
    return s;
}

// What a rank's neighbours need of it after a stage: its top up_needs planes are rank + 1's lower halo, its bottom dn_needs
// planes rank - 1's upper halo.
inline int slab_up_needs(int need_lo, int end, int rank, int world) { return rank + 1 < world ? slab_min(need_lo, end) : 0; }
inline int slab_dn_needs(int need_hi, int begin, int nl, int rank) { return rank > 0 ? slab_min(need_hi, nl - begin) : 0; }

// The strips cover every plane a neighbour needs: the exchange of a stage's output may start behind the strips alone, under the
// rest of the interior.  (A side without a strip covers nothing: it must need nothing.)
inline bool slab_strips_cover(const SlabSplit &s, int dn_needs, int up_needs) { return s.split && dn_needs <= s.lo_w && up_needs <= s.hi_w; }

}  // namespace hjb
