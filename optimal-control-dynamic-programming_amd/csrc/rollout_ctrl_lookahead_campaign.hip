// rollout_ctrl_lookahead_campaign.hip - K36's 24 instantiations (kernels_rollout_ctrl_lookahead_campaign.h: D x value type x LDS) in
// a unit of their own, behind launch_rollout_ctrl_lookahead_campaign (called by hjb_rollout_run_control_lookahead_campaign in
// rollout_ctrl_lookahead_host.hip).  The fold is K28's kernel, launched through launch_campaign_fold (rollout_campaign.hip).
#include "kernels_rollout_ctrl_lookahead_campaign.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_ctrl_lookahead_campaign(int val_bytes, bool lds_on, int D, const DCtrlLookCampaignArgs &K, size_t lds,
                                                  hipStream_t st, double *stats) {
    const int64_t lanes = K.C.n_blocks * K.C.G;
    const dim3 b(256), g((unsigned)((lanes + 255) / 256));
    with_bool(val_bytes == 4, [&](auto f) {
        with_bool(lds_on, [&](auto l) {
            with_dim(D, [&](auto d) {
                using TV = std::conditional_t<decltype(f)::value, float, double>;
                constexpr bool LDS = decltype(l)::value;
                hipLaunchKernelGGL((k_rollout_ctrl_lookahead_campaign<decltype(d)::value, TV, LDS>), g, b, LDS ? lds : 0, st, K);
            });
        });
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_campaign_fold(K.C, st, stats);
}

}  // namespace hjb
