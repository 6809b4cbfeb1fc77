// kernels_rollout_lookahead_campaign.h - K29: the campaign form of K27's flown lookahead (kernels_rollout_lookahead.h, FLY = true).
// n_starts starts are each flown M times under the object's noise node set by the one-step lookahead on the object's value planes
// under its lookahead node set, and the per-trajectory results are reduced on the device to eight doubles per start
// (hjb_rollout_run_lookahead_campaign; the statistics and their order: hjbdp_campaign.h).  It is K28's frame
// (kernels_rollout_campaign.h) around K27's step: no array of a call has a dimension of n_starts * M.
//
// The lane layout is K28's: blocks of G = min(64, pow2 >= M) consecutive samples of one start, lane t of a launch slot t % G of block
// block0 + t / G, padding lanes alive with campaign_padding().  A live lane (sample m of start s) runs K27's flown step from
// X0[:, s] on the stream N.first + s * M + m - the stream K28 gives the same (s, m), so a label campaign and a lookahead campaign
// of one seed fly common random numbers.  Every part of the step is called, none restated:
//   look_step<D, TV> (hjbdp_lookahead.h) on the plane of plane_of_step[k] (-1: the zero function);
//   K25's sampler (hjbdp_noise.h): a Philox block when (k & 3) == 0, noise_node, the flight set's offsets on the flight mask alone;
//   the left-the-grid flag (campaign_outside) on every visited state k = 0 .. n_steps, as flown, after the noise.
// There are no path stores.  After the flight: campaign_slot, the log2 G shuffle levels with campaign_op (own value first), three
// ballots under the segment mask, slot 0 writes the block's 8 doubles to C.partials; k_campaign_fold (rollout_campaign.hip, K28's,
// launched through launch_campaign_fold) folds them into stats[:, s].
// Table placement is K27's: the lookahead block [p | e] through scalar loads (look_read), the flight block per lane and staged in
// LDS behind knots, 1/dx and u_table under the 32 KiB rule, the launch record where it lies in the argument segment
// (greedy_reread / campaign_reread): per step for the plane, and again after look_step for the sampler and the extent, so that
// nothing of the record is live across the candidate loop.
#pragma once
#include "kernels_rollout_campaign.h"
#include "kernels_rollout_lookahead.h"

namespace hjb {

// what the kernel reads: one argument, so that its layout is C++'s (K26's DGreedy, for its reason)
struct DLookCampaignArgs {
    DRollout R;                       // plane_of_step: the VALUE plane of every step (-1: the zero function)
    const void *values;               // [nS, n_planes] column-major, TV (global); null when every plane of the run is -1
    LookSet L;                        // the lookahead set, L.tab on the device
    DNoise N;                         // the flight set; N.first: the CALL's first stream; N.Wp unused
    DCampaign C;
    const double *X0;                 // [D, n_starts] (global)
};

// K28's lane layout: lane t of the launch is slot t % G of block C.block0 + t / G -> its block in the launch, its slot, its start and
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

template <int D, typename TV, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_lookahead_campaign(const DLookCampaignArgs K) {
    extern __shared__ double smem[];
    const double *kn, *rd, *ut, *nt;
    HJB_ROLLOUT_PLACE(p, K.R, K.R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, K.R, kn, rd, ut)
    if constexpr (LDS) {
        double *lds_n = HJB_ROLLOUT_PLACE_END(p);
        for (int e = threadIdx.x; e < K.N.n_tab; e += blockDim.x) lds_n[e] = K.N.tab[e];
        nt = lds_n;
        __syncthreads();
    } else {
        nt = K.N.tab;
    }
    typedef __attribute__((address_space(4))) DLookCampaignArgs KArgs;
    const KArgs &K0 = *(const KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int64_t lb, s, m;
    int slot, G;
    const bool live = campaign_lane(campaign_reread(K0).C, t, lb, slot, G, s, m);
    CampVals v = campaign_padding();
    bool f_exceed = false, f_settled = false;
    uint32_t n_out = 0u;                                      // 1 once a visited state lay outside the grid, as a word per lane: a vector register,
                                                              // where a flag carried round the step loop is a pair of scalar ones
    if (live) {
        double x[D];
        uint64_t stream;
        {
            const KArgs &Kk = campaign_reread(K0);
            stream = Kk.N.first + (uint64_t)(s * Kk.C.M + m);
#pragma unroll
            for (int a = 0; a < D; ++a) x[a] = Kk.X0[a + (int64_t)D * s];
#pragma unroll
            for (int a = 0; a < D; ++a) n_out |= campaign_outside(x[a], Kk.C.lo[a], Kk.C.hi[a]) ? 1u : 0u;
        }
        uint32_t rw[4] = {0u, 0u, 0u, 0u};
        double J = 0.0;
        for (int k = 0; k < campaign_reread(K0).R.n_steps; ++k) {
            double u[HJB_ROLLOUT_MAX_U], g, best;
            int label;
            {
                const KArgs &Kk = campaign_reread(K0);
                const int32_t p = Kk.R.plane_of_step[k];
                const TV *plane = p < 0 ? nullptr : static_cast<const TV *>(Kk.values) + (int64_t)p * Kk.R.nS;
                look_step<D, TV>(K0.R, K0.L, kn, rd, ut, plane, x, u, g, label, best);
            }
            J = J + g;
            {
                const KArgs &Kn = campaign_reread(K0);            // the flight set
                if ((k & 3) == 0) noise_block(Kn.N.seed, stream, (uint32_t)k >> 2, rw);
                const int n_thr = Kn.N.n_nodes - 1;
                const double *ntk = LDS ? nt : Kn.N.tab;          // the global form holds no pointer to the block across look_step
                const int w = noise_node(ntk, n_thr, noise_next_word(rw));
                const double *row = ntk + n_thr + w;              // the next masked axis' offsets, at this lane's node
#pragma unroll
                for (int a = 0; a < D; ++a)
                    if (Kn.N.mask & (1 << a)) {
                        x[a] = x[a] + row[0];
                        row += Kn.N.n_nodes;
                    }
            }
            const KArgs &Kc = campaign_reread(K0);                // the grid's extent
#pragma unroll
            for (int a = 0; a < D; ++a) n_out |= campaign_outside(x[a], Kc.C.lo[a], Kc.C.hi[a]) ? 1u : 0u;
        }
        const KArgs &Kk = campaign_reread(K0);
        (void)campaign_lane(Kk.C, t, lb, slot, G, s, m);          // the start again: not held across the flight
        double tol[D];
#pragma unroll
        for (int a = 0; a < D; ++a) tol[a] = Kk.C.tol[a];
        f_settled = campaign_settled(D, x, Kk.C.has_tol ? tol : nullptr);
        f_exceed = campaign_exceeds(J, Kk.C.threshold != nullptr, Kk.C.threshold ? Kk.C.threshold[s] : 0.0);
        v = campaign_slot(J, f_settled);
    }
    // every lane of the wave from here on, its place taken from the record again: nothing of it is held across the flight
    const KArgs &Kk = campaign_reread(K0);
    (void)campaign_lane(Kk.C, t, lb, slot, G, s, m);
    // the block tree: level L pairs element i with element i + 2^L
    for (int half = 1; half < G; half *= 2) {
        CampVals o;
        o.sum = __shfl_down(v.sum, half);
        o.sumsq = __shfl_down(v.sumsq, half);
        o.mn = __shfl_down(v.mn, half);
        o.mx = __shfl_down(v.mx, half);
        o.sum_settled = __shfl_down(v.sum_settled, half);
        v = campaign_op(v, o);
    }
    const unsigned long long b_exceed = __ballot(f_exceed), b_left = __ballot(n_out != 0u), b_settled = __ballot(f_settled);
    if (slot == 0 && lb < Kk.C.n_blocks) {
        const int lane = threadIdx.x & 63;                    // the segment's first lane: G divides 64 and the block size
        const unsigned long long seg = (G == 64 ? ~0ull : (1ull << G) - 1ull) << lane;
        double *out = Kk.C.partials + 8 * lb;
        out[0] = v.sum;
        out[1] = v.sumsq;
        out[2] = v.mn;
        out[3] = v.mx;
        out[4] = (double)__popcll(b_exceed & seg);
        out[5] = (double)__popcll(b_left & seg);
        out[6] = (double)__popcll(b_settled & seg);
        out[7] = v.sum_settled;
    }
}

// rollout_lookahead_campaign.hip instantiates the 24 kernels (D x value type x LDS) and launches the one asked for, then K28's
// fold; val_bytes: 4 or 8; lds: the bytes of the channel's tables and the flight block together; stats: [8, n_starts] on the device
hipError_t launch_rollout_lookahead_campaign(int val_bytes, bool lds_on, int D, const DLookCampaignArgs &K, size_t lds, hipStream_t st,
                                             double *stats);

}  // namespace hjb
