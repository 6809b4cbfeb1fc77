// kernels_ctrldist.h - variant 8, per-control form (K32): the stage kernel of a handle with a control-dependent disturbance
// (hjb_set_control_disturbance, include/hjbdp.h).
//
//   J_k(x) = min_u  g(x, u) + COMBINE_w F_{k+1}(x_next(x, u) + d_w(u))      COMBINE as in K24 (kernels_disturb.h)
//
// The kernel IS K24's: the same body text (kernels_disturb_body.inc), every operation of steps 2 - 5 on the same operands in the same
// order.  What differs is the one read of a node's offset: d[a][w] of the handle's block there, here entry (u, w, a) of the
// per-control table DT behind the block:
//     DT[(row * W + w) * D + a]        row = the control's VISITING index (control dim 0 slowest), the D entries of one
//                                      (control, node) contiguous, rounded once to TQ by the host.
//   min form: row is the control loop's counter.  The control loop is wave-uniform (its bounds are launch constants, no lane leaves
//   it early), so the index is formed from loop counters only and the offsets stay scalar operands: scalar loads into scalar
//   registers, no per-lane traffic, no LDS - as K24's.
//   FIXED: the label is per lane; row is formed from the decoded cj[] (after the label's range check: a label out of range reads
//   nothing) and the D offsets of a node are per-lane global loads of one table row - lanes with equal labels read one address.
// The index fits an int: the host refuses a table of more than 2^26 entries.  The block's own off[][] is not read; n_nodes, mode,
// the axis mask (bit a: some (w, l) entry of row a is not zero) and the weights are the block's, as in K24.
#pragma once
#include "kernels_disturb.h"

namespace hjb {

// the table row of a control: its visiting index (control dim 0 slowest) - the loop counter, or rebuilt from a decoded label
template <bool FIXED, typename IX>
__device__ __forceinline__ int ctrldist_row(const DParams *__restrict__ P, int C, const int (&cj)[HJB_MAX_C], IX u) {
    if (!FIXED) return (int)u;
    if (C == 1) return cj[0];
    if (C == 2) return cj[0] * P->m[1] + cj[1];
    return (cj[0] * P->m[1] + cj[1]) * P->m[2] + cj[2];
}

template <typename T, typename TJ, typename TQ, int D, typename IX, bool FIXED>
__global__ void __launch_bounds__(256)
k_backup_ctrldist(const DParams *__restrict__ P, const DParams *__restrict__ PQ, const DDisturb<TQ, T> *__restrict__ DW,
                  const TQ *__restrict__ DT, const TJ *__restrict__ Jn, TJ *__restrict__ Jout, void *__restrict__ idx_out,
                  const void *__restrict__ labels, int32_t *__restrict__ bad_label) {
#define HJB_DIST_OFFSET(a, w) DT[(ctrldist_row<FIXED, IX>(P, C, cj, u) * W + w) * D + a]
#include "kernels_disturb_body.inc"
#undef HJB_DIST_OFFSET
}

}  // namespace hjb
