// rollout_lookahead_campaign_pair.hip - K31's 24 instantiations of k_rollout_lookahead_campaign_pair
// (kernels_rollout_lookahead_campaign_pair.h: K29's set, D x value type x LDS) in a unit of their own, behind
// launch_rollout_lookahead_campaign_pair (called by hjb_rollout_run_campaign_pair in rollout_campaign_pair_host.hip).  The kernel
// alone: the folds come after both kernels of a launch, from the host loop.
#include "kernels_rollout_lookahead_campaign_pair.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_lookahead_campaign_pair(int val_bytes, bool lds_on, int D, const DLookCampaignPairArgs &K, size_t lds,
                                                  hipStream_t st) {
    const int64_t lanes = K.A.C.n_blocks * K.A.C.G;
    const dim3 b(256), g((unsigned)((lanes + 255) / 256));
    with_bool(val_bytes == 4, [&](auto f) {
        with_bool(lds_on, [&](auto l) {
            with_dim(D, [&](auto d) {
                using TV = std::conditional_t<decltype(f)::value, float, double>;
                constexpr bool LDS = decltype(l)::value;
                hipLaunchKernelGGL((k_rollout_lookahead_campaign_pair<decltype(d)::value, TV, LDS>), g, b, LDS ? lds : 0, st, K);
            });
        });
    });
    return hipGetLastError();
}

}  // namespace hjb
