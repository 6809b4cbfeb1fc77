// kernels_disturb.h - variant 8 (K24): the stage kernel of a handle with a disturbance (hjb_set_disturbance, include/hjbdp.h).
//
//   J_k(x) = min_u  g(x, u) + COMBINE_w F_{k+1}(x_next(x, u) + d_w)      COMBINE = sum_w p_w (.) (HJB_DIST_EXPECT) or max_w (.) (HJB_DIST_WORST)
//
// One thread per owned state, grid-stride, as k_backup_generic: controls are the outer loop (control dim 0 slowest, first minimum
// wins), the W nodes the inner loop.  Per state the control-independent prefixes of the term sums and of the cost are formed once;
// per control the term sums q_a, the stage cost g and - for the axes no node offsets (DDisturb::axes, a launch constant: wave-uniform
// branches) - the cell and weight; per node only the offset axes are located again, q_aw = (TQ)(q_a + d[a][w]), then the 2^D corners
// are gathered (axis-0 neighbours in one load: jstride[0] == 1) and lerped by HJB_LERP_AXES (hjbdp_canon.h, as every other piece here).
//   EXPECT: acc = (T)(p_0 v_0), acc = fma(p_w, v_w, acc) in node order.   WORST: acc = v_0, acc = v_w > acc ? v_w : acc.
//   candidate = (T)(g + acc).  With one node, no offset axis and p_0 = 1 every operation is k_backup_generic's: the same bits.
// The node offsets and weights sit in one small device block behind a kernel-argument pointer and are indexed by the node counter
// only: scalar loads into scalar registers, no per-lane traffic, no LDS.
//   TQ: the type queries are formed, located and weighted in.  HJB_TAB_F64: double - PQ is the handle's float64 shadow of the axes
//   (knots, 1/dx, next-state terms: Handle::dp64), the weight is rounded to float once; the stage-invariant (cell, weight) tables the
//   other kernels read for this typing cannot serve an offset query.  Otherwise TQ = T and PQ = P.
//   HJB_COST_F64: state part of the cost summed once per state in double, each control adds its part and rounds once.
//   FIXED: the fixed-label form (hjb_evaluate*): the thread reads its label, decodes it column-major and forms that ONE candidate -
//   the same operations on the same operands, so the same bits as the candidate the min form compares.  A label out of range: nothing
//   is read, NaN is stored, *bad_label is raised (kernels_evaluate.h's rule).
//   IX: int64_t serves any size; uint32_t is the same kernel where the host found every state index and J offset below 2^31
//   (eval_runs_i32).  The floating-point operations do not depend on it.
// Whole grids only (hjb_set_disturbance refuses slab handles): no halo, no plane window.  No LDS.
// The body is kernels_disturb_body.inc, the one text this kernel and the per-control form (K32, kernels_ctrldist.h) are made of;
// what differs is where a node's offset is read from (HJB_DIST_OFFSET).
#pragma once
#include "hjbdp_dev.h"
#include "hjbdp_canon.h"

namespace hjb {

// the device block of one handle's disturbance, typed as the kernel reads it (the host fills it once per hjb_set_disturbance)
template <typename TQ, typename T>
struct DDisturb {
    int32_t n_nodes;
    int32_t mode;                               // HJB_DIST_EXPECT / HJB_DIST_WORST
    uint32_t axes;                              // bit a: some node offsets axis a
    int32_t pad;
    TQ off[HJB_MAX_D][HJB_DIST_MAX_NODES];      // d[a][w], rounded once to TQ
    T p[HJB_DIST_MAX_NODES];                    // weights, rounded once to T (EXPECT)
};

template <typename TQ, typename IX, int D>
__device__ __forceinline__ TQ dist_term(const DTerm &t, const int (&si)[D], const int (&cj)[HJB_MAX_C]) {
    return as_global<TQ>(t.data)[eval_term_off<IX, false, D>(t, si, cj)];
}

template <typename T, typename TJ, typename TQ, int D, typename IX, bool FIXED>
__global__ void __launch_bounds__(256)
k_backup_disturb(const DParams *__restrict__ P, const DParams *__restrict__ PQ, const DDisturb<TQ, T> *__restrict__ DW,
                 const TJ *__restrict__ Jn, TJ *__restrict__ Jout, void *__restrict__ idx_out,
                 const void *__restrict__ labels, int32_t *__restrict__ bad_label) {
#define HJB_DIST_OFFSET(a, w) DW->off[a][w]
#include "kernels_disturb_body.inc"
#undef HJB_DIST_OFFSET
}

}  // namespace hjb
