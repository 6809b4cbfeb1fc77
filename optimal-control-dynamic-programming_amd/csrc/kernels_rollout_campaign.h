// kernels_rollout_campaign.h - K28: the campaign form of K25 (kernels_rollout_noisy.h).  n_starts starts are each flown M times
// under the object's noise node set by the stored-label controller, and the per-trajectory results are reduced on the device to
// eight doubles per start (hjb_rollout_run_campaign; the statistics and their order: hjbdp_campaign.h).  No array of a call has
// a dimension of n_starts * M.
//
// The call's samples form blocks of G = min(64, pow2 >= M) consecutive samples of one start (the last block of a start padded);
// start s owns blocks s * B .. s * B + B - 1, B = ceil(M / G).  A launch takes n_blocks consecutive blocks from block0 on, and its
// lanes are (block, slot) in order: lane t of the launch is slot t % G of block block0 + t / G.  A wave of 64 lanes therefore holds
// 64 / G whole blocks and no block straddles a wave.
//   k_rollout_campaign  one lane per slot.  A live lane (sample m = blk * G + slot < M) flies K25's trajectory from X0[:, s] on the
//       stream N.first + s * M + m: K25's step by K25's own statements (HJB_ROLLOUT_LOOKUP, _AFFINE_STEP, _NOISE_STEP), no path stores,
//       plus the left-the-grid flag on every visited state.  Lanes of padding slots and lanes past the launch's last block fly
//       nothing and draw nothing, but stay alive: they join the cross-lane steps with the identities.  The block tree is
//       log2 G levels of wave shuffles (lane i takes lane i + 2^L and applies campaign_op, its own value first: the lanes that
//       are multiples of 2^(L+1) hold exactly the tree's elements; what the others compute is never read); the counts are three
//       ballots and a popcount under the segment's mask.  Slot 0 of a block writes its partial, 8 doubles, to Cp.partials.
//   k_campaign_fold     (rollout_campaign.hip) one thread per start the launch touches: the start's partials of this launch folded
//       in block order into stats[:, s], which persists across launches - a start whose blocks straddle launches continues from what the earlier
//       launch left.  The first block of a start initialises the accumulator (acc = p_0).
// No atomics, and no floating-point order that depends on the schedule: the result is a function of (M, the samples) alone.
// X0 is read once per start: the lanes of a segment read one address.
// The flight up to the block partial is kernels_rollout_campaign_body.inc, the one text this kernel and K30's histogram form
// (k_rollout_campaign_hist, kernels_rollout_campaign_hist.h) are made of.
#pragma once
#include "kernels_rollout_noisy.h"
#include "hjbdp_campaign.h"

namespace hjb {

struct DCampaign {
    int64_t n_blocks, block0;         // this launch: blocks block0 .. block0 + n_blocks of the call's block list
    int64_t B, M;                     // blocks per start, samples per start
    int32_t G, log2G;
    int32_t has_tol, reserved_;
    const double *threshold;          // [n_starts] (global) or null
    double tol[HJB_MAX_D];
    double lo[HJB_MAX_D], hi[HJB_MAX_D];      // the first and the last knot of every axis
    double *partials;                 // [8, n_blocks] (global): the launch's block partials, stats order, counts as doubles
};

// what the kernel reads: one argument, so that its layout is C++'s (K26's DGreedy, for its reason)
struct DCampaignArgs {
    DRollout R;
    DNoise N;                         // N.first: the CALL's first stream; N.Wp unused
    DCampaign C;
    const double *X0;                 // [D, n_starts] (global)
};

// The launch record is read where it lies, in the argument segment (record_reread, hjbdp_dev.h) - and again inside a step where
// that is needed: from D = 3 on.  Below that the step's scalars fit beside the loop's own, one read of the record per step
// (`step`) serves the whole body, and the further reads would only lengthen the step (measured: + 10 % at D = 2).
template <int D, typename T>
__device__ __forceinline__ const T &campaign_reread_in_step(const T &r, const T &step) {
    if constexpr (D >= 3) return record_reread(r);
    else return step;
}

// The campaign frame, the ONE statement K28 and K29 (kernels_rollout_lookahead_campaign.h) stand in.
// The lane layout: lane t of the launch is slot t % G of block C.block0 + t / G -> its block in the launch, its slot, its start and
// its sample; true for a lane that flies (a block of the launch, a sample below M)
template <typename CAMP>
__device__ __forceinline__ bool campaign_lane(const CAMP &C, int64_t t, int64_t &lb, int &slot, int &G, int64_t &s, int64_t &m) {
    G = C.G;
    lb = t >> C.log2G;
    slot = (int)(t & (G - 1));
    const int64_t gb = C.block0 + lb;
    s = gb / C.B;
    m = (gb - s * C.B) * G + slot;
    return lb < C.n_blocks && m < C.M;
}

// The block partial, by every lane of the wave: the block tree (level L pairs element i with element i + 2^L) on v_, the three
// counts as ballots under the segment's mask, and slot 0 of a block of the launch writes the 8 doubles to C_.partials.  C_ is an
// EXPRESSION for the DCampaign, evaluated once, after the ballots: K28 passes a reread of its record there, K29 the one it took
// before the tree.  A macro: as a force-inlined function, with the record read before the tree, 4,876 lines of K28's unit
// changed.  Its names (half, o, b_exceed, b_left, b_settled, camp_c_, lane, seg, out) live inside its own block.
#define HJB_CAMPAIGN_BLOCK_PARTIAL(v_, f_exceed_, f_left_, f_settled_, G_, slot_, lb_, C_)                                      \
    {                                                                                                                           \
        for (int half = 1; half < G_; half *= 2) {                                                                              \
            CampVals o;                                                                                                         \
            o.sum = __shfl_down(v_.sum, half);                                                                                  \
            o.sumsq = __shfl_down(v_.sumsq, half);                                                                              \
            o.mn = __shfl_down(v_.mn, half);                                                                                    \
            o.mx = __shfl_down(v_.mx, half);                                                                                    \
            o.sum_settled = __shfl_down(v_.sum_settled, half);                                                                  \
            v_ = campaign_op(v_, o);                                                                                            \
        }                                                                                                                       \
        const unsigned long long b_exceed = __ballot(f_exceed_), b_left = __ballot(f_left_), b_settled = __ballot(f_settled_);  \
        const auto &camp_c_ = C_;                                                                                               \
        if (slot_ == 0 && lb_ < camp_c_.n_blocks) {                                                                             \
            const int lane = threadIdx.x & 63;                /* the segment's first lane: G divides 64 and the block size */   \
            const unsigned long long seg = (G_ == 64 ? ~0ull : (1ull << G_) - 1ull) << lane;                                    \
            double *out = camp_c_.partials + 8 * lb_;                                                                           \
            out[0] = v_.sum;                                                                                                    \
            out[1] = v_.sumsq;                                                                                                  \
            out[2] = v_.mn;                                                                                                     \
            out[3] = v_.mx;                                                                                                     \
            out[4] = (double)__popcll(b_exceed & seg);                                                                          \
            out[5] = (double)__popcll(b_left & seg);                                                                            \
            out[6] = (double)__popcll(b_settled & seg);                                                                         \
            out[7] = v_.sum_settled;                                                                                            \
        }                                                                                                                       \
    }

template <int D, typename TL, int METHOD, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_campaign(const DCampaignArgs K) {
#include "kernels_rollout_campaign_body.inc"
    // every lane of the wave from here on
    HJB_CAMPAIGN_BLOCK_PARTIAL(v, f_exceed, f_left, f_settled, G, slot, lb, record_reread(K0).C)
}

// rollout_campaign.hip instantiates the 72 kernels (label type x method x LDS x D, as K25) and launches the one asked for, then
// the fold; lds: the bytes of the channel's tables and the node block together; stats: [8, n_starts] on the device
hipError_t launch_rollout_campaign(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, const DNoise &N,
                                   const DCampaign &Cp, size_t lds, hipStream_t st, const double *X0, double *stats);

// the fold alone (k_campaign_fold over the starts the launch Cp touches), behind a kernel that wrote Cp.partials on `st`: what
// launch_rollout_campaign ends in, and what the campaigns of other controllers (K29, kernels_rollout_lookahead_campaign.h) call
hipError_t launch_campaign_fold(const DCampaign &Cp, hipStream_t st, double *stats);

}  // namespace hjb
