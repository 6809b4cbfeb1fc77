// kernels_rollout_lookahead_campaign_pair.h - K31 for the lookahead controller: K29's flight
// (kernels_rollout_lookahead_campaign_body.inc, the same text) followed by the pair tail of kernels_rollout_campaign_pair.h, which
// states the two roles, the scratch and why the two flights of a pair are two kernels.  The campaign frame sees only a sample's cost
// and its left flag (n_out != 0u here), so the tail is the label kernel's, word for word.  HJB_PAIR_LOOKAHEAD and HJB_PAIR_GREEDY
// are this one kernel: the host hands it the object's lookahead set or the one-node zero set.
#pragma once
#include "kernels_rollout_lookahead_campaign.h"
#include "kernels_rollout_campaign_pair.h"

namespace hjb {

// what the kernel reads: K29's record first, where K29's flight rereads it, then the pair's
struct DLookCampaignPairArgs {
    DLookCampaignArgs A;
    DCampPair P;
};

template <int D, typename TV, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_lookahead_campaign_pair(const DLookCampaignPairArgs KP) {
    const DLookCampaignArgs &K = KP.A;
#include "kernels_rollout_lookahead_campaign_body.inc"
    // every lane of the wave from here on, its place taken from the record again: nothing of it is held across the flight
    const KArgs &Kk = record_reread(K0);
    const bool flew = campaign_lane(Kk.C, t, lb, slot, G, s, m);
    typedef __attribute__((address_space(4))) DLookCampaignPairArgs KPArgs;
    const KPArgs &KP0 = *(const KPArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const double c_own = v.sum;                               // before the tree runs in place on v
    campaign_pair_store(record_reread(KP0).P, flew, t, c_own, n_out != 0u);
    HJB_CAMPAIGN_BLOCK_PARTIAL(v, f_exceed, n_out != 0u, f_settled, G, slot, lb, Kk.C)
    if (record_reread(KP0).P.in) {
        CampVals vd = campaign_padding();
        bool d_neg = false, d_pos = false, d_in = false;
        campaign_pair_load(record_reread(KP0).P, flew, t, c_own, n_out != 0u, vd, d_neg, d_pos, d_in);
        HJB_CAMPAIGN_BLOCK_PARTIAL(vd, d_neg, d_pos, d_in, G, slot, lb, (DCampPairOut{Kk.C.n_blocks, record_reread(KP0).P.dpartials}))
    }
}

// rollout_lookahead_campaign_pair.hip instantiates the 24 kernels (K29's set) and launches the one asked for: the kernel alone, no
// fold (see launch_rollout_campaign_pair).  lds: K29's bytes
hipError_t launch_rollout_lookahead_campaign_pair(int val_bytes, bool lds_on, int D, const DLookCampaignPairArgs &K, size_t lds,
                                                  hipStream_t st);

}  // namespace hjb
