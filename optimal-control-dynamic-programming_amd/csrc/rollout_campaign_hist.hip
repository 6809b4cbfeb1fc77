// rollout_campaign_hist.hip - K30's 72 instantiations of k_rollout_campaign_hist (kernels_rollout_campaign_hist.h: K28's set, label
// type x method x LDS x D) in a unit of their own, behind launch_rollout_campaign_hist (called by hjb_rollout_run_campaign_hist in
// rollout_campaign_hist_host.hip).  The fold is K28's kernel, launched through launch_campaign_fold (rollout_campaign.hip).
#include "kernels_rollout_campaign_hist.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_campaign_hist(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, const DNoise &N,
                                        const DCampaign &Cp, const DCampHist &H, size_t lds, hipStream_t st, const double *X0,
                                        double *stats) {
    const int64_t lanes = Cp.n_blocks * Cp.G;
    const dim3 b(256), g((unsigned)((lanes + 255) / 256));
    const DCampaignHistArgs K{{R, N, Cp, X0}, H};
    with_label_type(idx_bytes, [&](auto tl) {
        with_int<HJB_LOOKUP_NEAREST, HJB_LOOKUP_LINEAR>(method, [&](auto m) {
            with_bool(lds_on, [&](auto l) {
                with_dim(D, [&](auto d) {
                    using TL = typename decltype(tl)::type;
                    // lds: the tables (LDS form only) and the wave histograms (wave form only), as campaign_hist_form sized them
                    hipLaunchKernelGGL((k_rollout_campaign_hist<decltype(d)::value, TL, decltype(m)::value, decltype(l)::value>), g, b, lds, st,
                                       K);
                });
            });
        });
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_campaign_fold(Cp, st, stats);
}

}  // namespace hjb
