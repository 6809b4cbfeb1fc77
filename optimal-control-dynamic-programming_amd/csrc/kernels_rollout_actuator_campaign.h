// kernels_rollout_actuator_campaign.h - K34: the campaign form of K33 (kernels_rollout_actuator.h).  n_starts starts are each flown
// M times under the object's actuator node set by the stored-label controller, and the per-trajectory results are reduced on the
// device to eight doubles per start (hjb_rollout_run_actuator_campaign).  K28's frame (kernels_rollout_campaign.h) word for word:
// the slots, the padding, the blocks of G = min(64, pow2 >= M), campaign_lane, the block tree and the ballots of
// HJB_CAMPAIGN_BLOCK_PARTIAL, the fold of launch_campaign_fold, and the launch record reread where it lies in the argument segment.
// A live lane flies K33's trajectory from X0[:, s] on the stream N.first + s * M + m: K33's step by K33's own statements
// (HJB_ROLLOUT_LOOKUP, _AFFINE_STEP, _ACTUATOR_STEP), no path stores, plus the left-the-grid flag on every visited state.
// The flight is this kernel's own text and not a hook in kernels_rollout_campaign_body.inc: K28's and K30's units are then the
// preprocessed text they were, and their code objects do not move.
#pragma once
#include "kernels_rollout_actuator.h"
#include "kernels_rollout_campaign.h"

namespace hjb {

// what the kernel reads: one argument, so that its layout is C++'s (DCampaignArgs, for its reason)
struct DActCampaignArgs {
    DRollout R;
    DActuator N;                      // N.first: the CALL's first stream; N.Wp unused
    DCampaign C;
    const double *X0;                 // [D, n_starts] (global)
};

// The occupancy the register allocation aims at: K28's waves per SIMD at the 'nearest' forms of D = 5 (8) and D = 6 (7), where
// the default schedule takes 6 to 12 vector registers more than K28 and lands one tier below it, and at the D = 5 'linear' LDS
// form (5; default 100 registers against K28's 88); with the target stated the same text fits (no spill, no private segment:
// tests/test_kernel_budget_actuator.py).  1 elsewhere: no constraint.
constexpr int actuator_campaign_waves(int D, int METHOD, bool LDS) {
    return METHOD != HJB_LOOKUP_NEAREST ? (D == 5 && LDS ? 5 : 1) : D == 5 ? 8 : D == 6 ? 7 : 1;
}
// The D = 5 'linear' LDS form needs five registers more than its target of 96 leaves (its peak is the 32-corner lookup): there
// the lane's block, slot and start are not held across the flight but formed again behind it, from the thread index, by
// campaign_lane's own expressions (the asm makes the index opaque, so the two computations are not merged).  Every other form is
// the text it was without this.
constexpr bool actuator_campaign_relocate(int D, int METHOD, bool LDS) { return D == 5 && METHOD == HJB_LOOKUP_LINEAR && LDS; }

template <int D, typename TL, int METHOD, bool LDS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(actuator_campaign_waves(D, METHOD, LDS))))
k_rollout_actuator_campaign(const DActCampaignArgs K) {
    extern __shared__ double smem[];
    const double *kn, *rd, *ut, *nt;
    HJB_ROLLOUT_PLACE(p, K.R, K.R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, K.R, kn, rd, ut)
    HJB_ROLLOUT_STAGE_NOISE(LDS, p, K.N, nt)
    if constexpr (LDS) __syncthreads();
    typedef __attribute__((address_space(4))) DActCampaignArgs KArgs;
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
            const KArgs &Kn = campaign_reread_in_step<D>(K0, Kl);      // the node set and the grid's extent
            const int n_nodes = Kn.N.n_nodes;
            int w;
            HJB_ROLLOUT_ACTUATOR_STEP(D, HJB_ROLLOUT_MAX_U, Kn.N.seed, stream, k, rw, nt, nt + (n_nodes - 1), n_nodes, Kn.N.live,
                                      Kn.N.base_mask, Kn.N.terms, campaign_reread_in_step<D>(K0, Kl).R, u, xn, w)
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
        if constexpr (actuator_campaign_relocate(D, METHOD, LDS)) {
            unsigned tx = threadIdx.x;
            asm volatile("" : "+v"(tx));
            const int64_t t2 = blockIdx.x * (int64_t)blockDim.x + tx;
            s = (Kk.C.block0 + (t2 >> Kk.C.log2G)) / Kk.C.B;                    // campaign_lane's s
        }
        f_exceed = campaign_exceeds(J, Kk.C.threshold != nullptr, Kk.C.threshold ? Kk.C.threshold[s] : 0.0);
        v = campaign_slot(J, f_settled);
    }
    // every lane of the wave from here on
    if constexpr (actuator_campaign_relocate(D, METHOD, LDS)) {
        unsigned tx = threadIdx.x;
        asm volatile("" : "+v"(tx));
        const int64_t t2 = blockIdx.x * (int64_t)blockDim.x + tx;
        const auto &Cc = record_reread(K0).C;
        lb = t2 >> Cc.log2G;                                  // campaign_lane's lb and slot
        slot = (int)(t2 & (Cc.G - 1));
    }
    HJB_CAMPAIGN_BLOCK_PARTIAL(v, f_exceed, f_left, f_settled, G, slot, lb, record_reread(K0).C)
}

// rollout_actuator_campaign.hip instantiates the 72 kernels (label type x method x LDS x D, as K28) and launches the one asked
// for, then K28's fold (launch_campaign_fold); lds: the bytes of the channel's tables and the node block together; stats:
// [8, n_starts] on the device
hipError_t launch_rollout_actuator_campaign(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, const DActuator &N,
                                            const DCampaign &Cp, size_t lds, hipStream_t st, const double *X0, double *stats);

}  // namespace hjb
