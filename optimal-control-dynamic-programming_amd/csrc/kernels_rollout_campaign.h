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
    extern __shared__ double smem[];
    const double *kn, *rd, *ut, *nt;
    HJB_ROLLOUT_PLACE(p, K.R, K.R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, K.R, kn, rd, ut)
    HJB_ROLLOUT_STAGE_NOISE(LDS, p, K.N, nt)
    if constexpr (LDS) __syncthreads();
    typedef __attribute__((address_space(4))) DCampaignArgs KArgs;
    const KArgs &K0 = *(const KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int64_t lb, s, m;
    int slot, G;
    const bool live = campaign_lane(record_reread(K0).C, t, lb, slot, G, s, m);
    CampVals v = campaign_padding();
    bool f_exceed = false, f_left = false, f_settled = false;
    if (live) {
        double x[D];
        uint64_t stream;
        {
            const KArgs &Kk = record_reread(K0);
            stream = Kk.N.first + (uint64_t)(s * Kk.C.M + m);
#pragma unroll
            for (int a = 0; a < D; ++a) x[a] = Kk.X0[a + (int64_t)D * s];
#pragma unroll
            for (int a = 0; a < D; ++a) f_left = f_left || campaign_outside(x[a], Kk.C.lo[a], Kk.C.hi[a]);
        }
        uint32_t rw[4] = {0u, 0u, 0u, 0u};
        double J = 0.0;
        for (int k = 0; k < record_reread(K0).R.n_steps; ++k) {
            const KArgs &Kl = record_reread(K0);              // the lookup's part of the record
            const TL *__restrict__ lab = static_cast<const TL *>(Kl.R.labels);
            const int nu = Kl.R.n_u;
            const int64_t nl = Kl.R.n_labels;
            HJB_ROLLOUT_LOOKUP(D, HJB_ROLLOUT_MAX_U, METHOD, Kl.R, kn, rd, ut, lab, k, x, nu, nl, u)
            // the record again for the cost, and again for each row of A and of B
            HJB_ROLLOUT_AFFINE_STEP(D, HJB_ROLLOUT_MAX_U, campaign_reread_in_step<D>(K0, Kl).R, campaign_reread_in_step<D>(K0, Kl).R,
                                    x, u, nu, g, xn)
            J = J + g;
            const KArgs &Kn = campaign_reread_in_step<D>(K0, Kl);      // the noise set and the grid's extent
            const int n_nodes = Kn.N.n_nodes;
            int w;
            HJB_ROLLOUT_NOISE_STEP(D, Kn.N.seed, stream, k, rw, nt, nt + (n_nodes - 1), n_nodes, Kn.N.mask, xn, w)
#pragma unroll
            for (int a = 0; a < D; ++a) x[a] = xn[a];
#pragma unroll
            for (int a = 0; a < D; ++a) f_left = f_left || campaign_outside(x[a], Kn.C.lo[a], Kn.C.hi[a]);
        }
        const KArgs &Kk = record_reread(K0);
        double tol[D];
#pragma unroll
        for (int a = 0; a < D; ++a) tol[a] = Kk.C.tol[a];
        f_settled = campaign_settled(D, x, Kk.C.has_tol ? tol : nullptr);
        f_exceed = campaign_exceeds(J, Kk.C.threshold != nullptr, Kk.C.threshold ? Kk.C.threshold[s] : 0.0);
        v = campaign_slot(J, f_settled);
    }
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
