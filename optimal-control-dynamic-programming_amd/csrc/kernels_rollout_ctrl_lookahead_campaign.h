// kernels_rollout_ctrl_lookahead_campaign.h - K36: the campaign form of K35's flown lookahead (kernels_rollout_ctrl_lookahead.h,
// FLY = true).  n_starts starts are each flown M times on the object's ACTUATOR plant by the one-step lookahead on the object's
// value planes under its per-control lookahead set, and the per-trajectory results are reduced on the device to eight doubles per
// start (hjb_rollout_run_control_lookahead_campaign; the statistics and their order: hjbdp_campaign.h).  It is K29's frame
// (kernels_rollout_lookahead_campaign.h) around K35's flown step: no array of a call has a dimension of n_starts * M.
//
// The lane layout is K28's: blocks of G = min(64, pow2 >= M) consecutive samples of one start, lane t of a launch slot t % G of block
// block0 + t / G, padding lanes alive with campaign_padding().  A live lane (sample m of start s) runs K35's flown step from
// X0[:, s] on the stream N.first + s * M + m - the stream K34 gives the same (s, m), so a label campaign on the actuator plant and
// this one fly common random numbers.  Every part of the step is called, none restated:
//   ctrl_look_step<D, TV> (hjbdp_ctrl_lookahead.h) on the plane of plane_of_step[k] (-1: the zero function);
//   K33's drawn-node step (HJB_ROLLOUT_ACTUATOR_STEP, kernels_rollout_actuator.h) on the actuator set, the cost on the commanded u;
//   the left-the-grid flag (campaign_outside) on every visited state k = 0 .. n_steps, as flown, after the noise.
// There are no path stores.  After the flight: campaign_slot and K28's block partial (HJB_CAMPAIGN_BLOCK_PARTIAL); k_campaign_fold
// (rollout_campaign.hip, K28's, launched through launch_campaign_fold) folds them into stats[:, s].
// Table placement is K35's: the lookahead block through scalar loads (look_read), the actuator block per lane and staged in LDS
// behind knots, 1/dx and u_table under the 32 KiB rule, the launch record where it lies in the argument segment (record_reread):
// per step for the plane, and again after the step for the sampler and the extent, so that nothing of the record is live
// across the candidate loop.  The flight is this kernel's own text and not a hook in kernels_rollout_lookahead_campaign_body.inc:
// K29's and K30's units are then the preprocessed text they were.
#pragma once
#include "kernels_rollout_campaign.h"
#include "kernels_rollout_ctrl_lookahead.h"

namespace hjb {

// what the kernel reads: one argument, so that its layout is C++'s (K26's DGreedy, for its reason)
struct DCtrlLookCampaignArgs {
    DRollout R;                       // plane_of_step: the VALUE plane of every step (-1: the zero function)
    const void *values;               // [nS, n_planes] column-major, TV (global); null when every plane of the run is -1
    CtrlLookSet L;                    // the per-control lookahead set, L.tab on the device
    DActuator N;                      // the plant; N.first: the CALL's first stream; N.Wp unused
    DCampaign C;
    const double *X0;                 // [D, n_starts] (global)
};

template <int D, typename TV, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_ctrl_lookahead_campaign(const DCtrlLookCampaignArgs K) {
    extern __shared__ double smem[];
    const double *kn, *rd, *ut, *nt;
    HJB_ROLLOUT_PLACE(p, K.R, K.R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, K.R, kn, rd, ut)
    HJB_ROLLOUT_STAGE_NOISE(LDS, p, K.N, nt)
    if constexpr (LDS) __syncthreads();
    typedef __attribute__((address_space(4))) DCtrlLookCampaignArgs KArgs;
    const KArgs &K0 = *(const KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int64_t lb, s, m;
    int slot, G;
    const bool live = campaign_lane(record_reread(K0).C, t, lb, slot, G, s, m);
    CampVals v = campaign_padding();
    bool f_exceed = false, f_settled = false;
    uint32_t n_out = 0u;                                      // 1 once a visited state lay outside the grid, as a word per lane (K29's form)
    if (live) {
        double x[D];
        uint64_t stream;
        {
            const KArgs &Kk = record_reread(K0);
            stream = Kk.N.first + (uint64_t)(s * Kk.C.M + m);
#pragma unroll
            for (int a = 0; a < D; ++a) x[a] = Kk.X0[a + (int64_t)D * s];
#pragma unroll
            for (int a = 0; a < D; ++a) n_out |= campaign_outside(x[a], Kk.C.lo[a], Kk.C.hi[a]) ? 1u : 0u;
        }
        uint32_t rw[4] = {0u, 0u, 0u, 0u};
        double J = 0.0;
        for (int k = 0; k < record_reread(K0).R.n_steps; ++k) {
            double u[HJB_ROLLOUT_MAX_U], g, best;
            int label;
            {
                const KArgs &Kk = record_reread(K0);
                const int32_t p = Kk.R.plane_of_step[k];
                const TV *plane = p < 0 ? nullptr : static_cast<const TV *>(Kk.values) + (int64_t)p * Kk.R.nS;
                ctrl_look_step<D, TV>(K0.R, K0.L, kn, rd, ut, plane, x, u, g, label, best);
            }
            J = J + g;
            {
                const KArgs &Kn = record_reread(K0);              // the actuator set
                const int n_nodes = Kn.N.n_nodes;
                const double *blk = LDS ? nt : Kn.N.tab;          // the global form takes the block from the record here
                int w;
                HJB_ROLLOUT_ACTUATOR_STEP(D, HJB_ROLLOUT_MAX_U, Kn.N.seed, stream, k, rw, blk, blk + (n_nodes - 1), n_nodes, Kn.N.live,
                                          Kn.N.base_mask, Kn.N.terms, record_reread(K0).R, u, x, w)
            }
            const KArgs &Kc = record_reread(K0);              // the grid's extent
#pragma unroll
            for (int a = 0; a < D; ++a) n_out |= campaign_outside(x[a], Kc.C.lo[a], Kc.C.hi[a]) ? 1u : 0u;
        }
        const KArgs &Kk = record_reread(K0);
        (void)campaign_lane(Kk.C, t, lb, slot, G, s, m);          // the start again: not held across the flight
        double tol[D];
#pragma unroll
        for (int a = 0; a < D; ++a) tol[a] = Kk.C.tol[a];
        f_settled = campaign_settled(D, x, Kk.C.has_tol ? tol : nullptr);
        f_exceed = campaign_exceeds(J, Kk.C.threshold != nullptr, Kk.C.threshold ? Kk.C.threshold[s] : 0.0);
        v = campaign_slot(J, f_settled);
    }
    // every lane of the wave from here on, its place taken from the record again: nothing of it is held across the flight
    const KArgs &Kk = record_reread(K0);
    (void)campaign_lane(Kk.C, t, lb, slot, G, s, m);
    HJB_CAMPAIGN_BLOCK_PARTIAL(v, f_exceed, n_out != 0u, f_settled, G, slot, lb, Kk.C)
}

// rollout_ctrl_lookahead_campaign.hip instantiates the 24 kernels (D x value type x LDS) and launches the one asked for, then
// K28's fold; val_bytes: 4 or 8; lds: the bytes of the channel's tables and the actuator block together; stats: [8, n_starts] on
// the device
hipError_t launch_rollout_ctrl_lookahead_campaign(int val_bytes, bool lds_on, int D, const DCtrlLookCampaignArgs &K, size_t lds,
                                                  hipStream_t st, double *stats);

}  // namespace hjb
