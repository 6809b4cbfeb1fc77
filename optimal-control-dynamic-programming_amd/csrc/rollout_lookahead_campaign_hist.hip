// rollout_lookahead_campaign_hist.hip - K30's 24 instantiations of k_rollout_lookahead_campaign_hist
// (kernels_rollout_lookahead_campaign_hist.h: K29's set, D x value type x LDS) in a unit of their own, behind
// launch_rollout_lookahead_campaign_hist (called by hjb_rollout_run_lookahead_campaign_hist in rollout_campaign_hist_host.hip).
// The fold is K28's kernel, launched through launch_campaign_fold (rollout_campaign.hip).
#include "kernels_rollout_lookahead_campaign_hist.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_lookahead_campaign_hist(int val_bytes, bool lds_on, int D, const DLookCampaignHistArgs &K, size_t lds,
                                                  hipStream_t st, double *stats) {
    const int64_t lanes = K.A.C.n_blocks * K.A.C.G;
    const dim3 b(256), g((unsigned)((lanes + 255) / 256));
    with_bool(val_bytes == 4, [&](auto f) {
        with_bool(lds_on, [&](auto l) {
            with_dim(D, [&](auto d) {
                using TV = std::conditional_t<decltype(f)::value, float, double>;
                // lds: the tables (LDS form only) and the wave histograms (wave form only), as campaign_hist_form sized them
                hipLaunchKernelGGL((k_rollout_lookahead_campaign_hist<decltype(d)::value, TV, decltype(l)::value>), g, b, lds, st, K);
            });
        });
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_campaign_fold(K.A.C, st, stats);
}

}  // namespace hjb
