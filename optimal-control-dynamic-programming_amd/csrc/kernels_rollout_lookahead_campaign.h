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
//   K25's drawn-node step (HJB_ROLLOUT_NOISE_STEP, kernels_rollout_noisy.h) on the flight set and the flight mask alone;
//   the left-the-grid flag (campaign_outside) on every visited state k = 0 .. n_steps, as flown, after the noise.
// There are no path stores.  After the flight: campaign_slot and K28's block partial (HJB_CAMPAIGN_BLOCK_PARTIAL: the log2 G shuffle
// levels, three ballots under the segment mask, slot 0's 8 doubles to C.partials); k_campaign_fold (rollout_campaign.hip, K28's,
// launched through launch_campaign_fold) folds them into stats[:, s].
// Table placement is K27's: the lookahead block [p | e] through scalar loads (look_read), the flight block per lane and staged in
// LDS behind knots, 1/dx and u_table under the 32 KiB rule, the launch record where it lies in the argument segment
// (record_reread): per step for the plane, and again after look_step for the sampler and the extent, so that
// nothing of the record is live across the candidate loop.
// The flight up to the block partial is kernels_rollout_lookahead_campaign_body.inc, the one text this kernel and K30's histogram
// form (k_rollout_lookahead_campaign_hist, kernels_rollout_lookahead_campaign_hist.h) are made of.
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

template <int D, typename TV, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_lookahead_campaign(const DLookCampaignArgs K) {
#include "kernels_rollout_lookahead_campaign_body.inc"
    // every lane of the wave from here on, its place taken from the record again: nothing of it is held across the flight
    const KArgs &Kk = record_reread(K0);
    (void)campaign_lane(Kk.C, t, lb, slot, G, s, m);
    HJB_CAMPAIGN_BLOCK_PARTIAL(v, f_exceed, n_out != 0u, f_settled, G, slot, lb, Kk.C)
}

// rollout_lookahead_campaign.hip instantiates the 24 kernels (D x value type x LDS) and launches the one asked for, then K28's
// fold; val_bytes: 4 or 8; lds: the bytes of the channel's tables and the flight block together; stats: [8, n_starts] on the device
hipError_t launch_rollout_lookahead_campaign(int val_bytes, bool lds_on, int D, const DLookCampaignArgs &K, size_t lds, hipStream_t st,
                                             double *stats);

}  // namespace hjb
