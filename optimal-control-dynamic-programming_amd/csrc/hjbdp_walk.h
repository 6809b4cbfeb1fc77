// hjbdp_walk.h - the integer arithmetic of the grid-stride walk, shared by the stage kernels (xcd_share) and the host's launch
// choice (launch_spans), and division by a launch-invariant divisor (magic_div / magic_quot).  No HIP dependency: tests/walk_harness.cpp
// compiles it as plain C++ and checks the first two exhaustively, tests/magicdiv_harness.cpp the division.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HJB_WALK_FN __host__ __device__ __forceinline__
#else
#define HJB_WALK_FN inline
#endif

namespace hjb {

// Workgroup b runs on XCD b % 8 (each XCD has its own L2).  With "workgroup b takes states [256 b, 256 b + 256)" every XCD walks the
// whole grid and its L2 holds all of J; here XCD x takes the x-th CONTIGUOUS share of every grid-sized span of workgroups instead
// (its workgroups b = x, x + 8, ...: G / 8 of them, one more for x < G % 8), so an L2 holds one region of J and its halo.  The host
// sizes the launch so that the spans are equally long (choose_launch): a short last span would fall to the first XCDs alone.
HJB_WALK_FN unsigned xcd_share(unsigned b, unsigned G) {
    const unsigned x = b & 7u, q = G >> 3, r = G & 7u;
    return x * q + (x < r ? x : r) + (b >> 3);
}

// The launch for `work` workgroup-sized units under a cap on workgroups.  A launch smaller than the work walks it in grid-sized
// spans.  Equally long spans: a short last span runs on part of the chip (Solver_attitude.run's 5199 chunks as 4096 + 1103: 3.63 ms
// per 19 stages; as 2 x 2600: 2.53), and the kernels that give XCD x the x-th contiguous share of every span (kernels_packed2.h,
// xcd_share above) would hand a short one to the first XCDs alone.
inline int64_t launch_spans(int64_t work, int64_t cap) {
    if (work <= cap) return work;
    const int64_t spans = (work + cap - 1) / cap;
    const int64_t g = ((work + spans - 1) / spans + 7) / 8 * 8;      // (a multiple of 8: the window modes' walk asks for it)
    return cap < g ? cap : g;
}

// Division of a 32-bit index by a launch-invariant divisor d >= 1 without a divide (Granlund & Montgomery, "Division by invariant
// integers using multiplication", 1994, figure 4.1 with N = 32): l = ceil(log2 d), m = floor(2^32 (2^l - d) / d) + 1,
// t = mulhi(m, n), q = (t + ((n - t) >> min(l, 1))) >> max(l - 1, 0) - exact for every n < 2^32.  The host forms (m, s1, s2) once per
// launch (magic_div); a kernel that takes a state index apart pays one multiply-high and four simple operations per axis
// (magic_quot) instead of the ~25 instructions of an emulated 32-bit divide (kernels_evaluate.h).
struct MagicDiv { uint32_t m, s1, s2, d; };
inline MagicDiv magic_div(uint32_t d) {
    uint32_t l = 0;
    while (l < 32 && ((uint64_t)1 << l) < d) ++l;
    MagicDiv k;
    k.m = (uint32_t)(((((uint64_t)1 << l) - d) << 32) / d + 1);
    k.s1 = l < 1 ? l : 1;
    k.s2 = l < 1 ? 0 : l - 1;
    k.d = d;
    return k;
}
HJB_WALK_FN uint32_t magic_quot(uint32_t n, const MagicDiv &k) {
    const uint32_t t = (uint32_t)(((uint64_t)k.m * n) >> 32);
    return (t + ((n - t) >> k.s1)) >> k.s2;
}

}  // namespace hjb
