// kernels_rollout_lookahead_campaign_hist.h - K30 for the lookahead controller: K29's campaign (kernels_rollout_lookahead_campaign.h)
// with the per-start histogram of the costs beside the eight statistics (hjb_rollout_run_lookahead_campaign_hist).
// k_rollout_lookahead_campaign_hist is K29's flight (kernels_rollout_lookahead_campaign_body.inc, the same text) and K28's block
// partial, unchanged, plus between the two the count of every live lane's cost: campaign_hist_count
// (kernels_rollout_campaign_hist.h, which states the two accumulation forms and where they are decided).  The campaign frame sees
// only a sample's cost, so the bin rule, the record and the forms are the label campaign's, word for word.
#pragma once
#include "kernels_rollout_lookahead_campaign.h"
#include "kernels_rollout_campaign_hist.h"

namespace hjb {

// what the kernel reads: K29's record first, where K29's flight rereads it, then the histogram's
struct DLookCampaignHistArgs {
    DLookCampaignArgs A;
    DCampHist H;
};

template <int D, typename TV, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_lookahead_campaign_hist(const DLookCampaignHistArgs KH) {
    const DLookCampaignArgs &K = KH.A;
#include "kernels_rollout_lookahead_campaign_body.inc"
    // every lane of the wave from here on, its place taken from the record again: nothing of it is held across the flight
    const KArgs &Kk = record_reread(K0);
    const bool counts = campaign_lane(Kk.C, t, lb, slot, G, s, m);
    {
        typedef __attribute__((address_space(4))) DLookCampaignHistArgs KHArgs;
        const KHArgs &KH0 = *(const KHArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        campaign_hist_count(record_reread(KH0).H, Kk.C, smem, counts, v.mn, s);
    }
    HJB_CAMPAIGN_BLOCK_PARTIAL(v, f_exceed, n_out != 0u, f_settled, G, slot, lb, Kk.C)
}

// rollout_lookahead_campaign_hist.hip instantiates the 24 kernels (K29's set) and launches the one asked for, then K28's fold;
// lds: the launch's dynamic LDS bytes (campaign_hist_form)
hipError_t launch_rollout_lookahead_campaign_hist(int val_bytes, bool lds_on, int D, const DLookCampaignHistArgs &K, size_t lds,
                                                  hipStream_t st, double *stats);

}  // namespace hjb
