// kernels_rollout_campaign_pair.h - K31: two controllers A and B on one plant, flown sample by sample on the same streams, and the
// record of the per-sample cost difference d = c_B - c_A reduced on the device beside the two plain records
// (hjb_rollout_run_campaign_pair; the difference record: campaign_pair_start, hjbdp_campaign.h).  The two flights are NOT fused
// into one thread: a label step costs about 1/400 of a lookahead step, so fusing buys nothing and would put K25's state into K27's
// register budget.  Each launch of a call runs A's flight kernel and then B's with one geometry (the same DCampaign but for the
// partials, the same block0 and n_blocks) on one stream, and the two talk through the pair scratch: one double and one byte per
// lane of the LAUNCH, indexed by t - never by anything of size n_starts * M.
//
// k_rollout_campaign_pair is K28's flight (kernels_rollout_campaign_body.inc, the same text) followed by the pair tail
// (campaign_pair_store, K28's block partial, campaign_pair_load and the block partial of d).  One kernel serves both roles,
// decided by wave-uniform fields of DCampPair:
//   first role  (P.out)  every live lane stores its cost (v.sum, before the tree runs in place on v) and its left flag to the
//       scratch at t; then its own block partial, as the plain kernel does.
//   second role (P.in)   every live lane loads A's cost and flag at t and forms d, e = d < 0, l = d > 0, t = neither left, and
//       campaign_slot(d, t); padding lanes keep campaign_padding().  Its own block partial, then a second
//       HJB_CAMPAIGN_BLOCK_PARTIAL over the difference values into P.dpartials.
// k_campaign_fold (K28's, unchanged) then folds the three partial arrays into stats_a, stats_b and stats_d.  No atomics.  The tail
// lies outside the step loop: nothing of it is live across the flight.
#pragma once
#include "kernels_rollout_campaign.h"

namespace hjb {

struct DCampPair {
    double *cost;                     // [lanes of a launch] (global): A's cost of lane t
    uint8_t *left;                    // [lanes of a launch] (global): A's left-the-grid flag of lane t
    double *dpartials;                // [8, n_blocks] (global): the launch's difference partials (second role)
    int32_t out, in;                  // first role: store to the scratch; second role: load from it and reduce d
};

// what the second block partial of the second role writes through: the launch's blocks and the difference partials
struct DCampPairOut {
    int64_t n_blocks;
    double *partials;
};

// The first role's part of a lane, by every lane of the wave, before the tree runs in place on the lane's values: c the lane's cost
// and f_left its left flag (read only where it flew), t the lane of the launch
template <typename PAIR>
__device__ __forceinline__ void campaign_pair_store(const PAIR &P, bool flew, int64_t t, double c, bool f_left) {
    if (P.out && flew) {
        P.cost[t] = c;
        P.left[t] = f_left ? 1 : 0;
    }
}

// The second role's part of a lane, behind the lane's own block partial: A's cost and flag at t, d and its three flags into vd,
// d_neg, d_pos and d_in, which otherwise keep the padding
template <typename PAIR>
__device__ __forceinline__ void campaign_pair_load(const PAIR &P, bool flew, int64_t t, double c, bool f_left, CampVals &vd, bool &d_neg,
                                                   bool &d_pos, bool &d_in) {
    if (flew) {
        const double ca = P.cost[t];
        const bool la = P.left[t] != 0;
        const double d = campaign_pair_diff(ca, c);
        d_neg = d < 0;
        d_pos = d > 0;
        d_in = !la && !f_left;
        vd = campaign_slot(d, d_in);
    }
}

// what the kernel reads: K28's record first, where K28's flight rereads it, then the pair's
struct DCampaignPairArgs {
    DCampaignArgs A;
    DCampPair P;
};

template <int D, typename TL, int METHOD, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_campaign_pair(const DCampaignPairArgs KP) {
    const DCampaignArgs &K = KP.A;
#include "kernels_rollout_campaign_body.inc"
    // every lane of the wave from here on: the scratch (v.sum = c in a live lane, before the tree), K28's block partial, and in the
    // second role the block partial of the difference
    typedef __attribute__((address_space(4))) DCampaignPairArgs KPArgs;
    const KPArgs &KP0 = *(const KPArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    // the lane's place taken from the record again, as K29's kernel does: the block, the slot and whether the lane flew are then not
    // held across the flight, where the forms from D = 3 on would spill the scalar ones
    const bool flew = campaign_lane(record_reread(K0).C, t, lb, slot, G, s, m);
    const double c_own = v.sum;
    campaign_pair_store(record_reread(KP0).P, flew, t, c_own, f_left);
    HJB_CAMPAIGN_BLOCK_PARTIAL(v, f_exceed, f_left, f_settled, G, slot, lb, record_reread(K0).C)
    if (record_reread(KP0).P.in) {
        CampVals vd = campaign_padding();
        bool d_neg = false, d_pos = false, d_in = false;
        campaign_pair_load(record_reread(KP0).P, flew, t, c_own, f_left, vd, d_neg, d_pos, d_in);
        HJB_CAMPAIGN_BLOCK_PARTIAL(vd, d_neg, d_pos, d_in, G, slot, lb, (DCampPairOut{record_reread(K0).C.n_blocks, record_reread(KP0).P.dpartials}))
    }
}

// rollout_campaign_pair.hip instantiates the 72 kernels (K28's set) and launches the one asked for: the kernel alone, no fold -
// the pair's host loop (rollout_campaign_pair_host.hip) folds after both kernels of a launch.  lds: K28's bytes
hipError_t launch_rollout_campaign_pair(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, const DNoise &N,
                                        const DCampaign &Cp, const DCampPair &P, size_t lds, hipStream_t st, const double *X0);

}  // namespace hjb
