// rollout_campaign_pair.hip - K31's 72 instantiations of k_rollout_campaign_pair (kernels_rollout_campaign_pair.h: K28's set, label
// type x method x LDS x D) in a unit of their own, behind launch_rollout_campaign_pair (called by hjb_rollout_run_campaign_pair in
// rollout_campaign_pair_host.hip).  The kernel alone: the folds come after both kernels of a launch, from the host loop.
#include "kernels_rollout_campaign_pair.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_campaign_pair(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, const DNoise &N,
                                        const DCampaign &Cp, const DCampPair &P, size_t lds, hipStream_t st, const double *X0) {
    const int64_t lanes = Cp.n_blocks * Cp.G;
    const dim3 b(256), g((unsigned)((lanes + 255) / 256));
    const DCampaignPairArgs K{{R, N, Cp, X0}, P};
    with_label_type(idx_bytes, [&](auto tl) {
        with_int<HJB_LOOKUP_NEAREST, HJB_LOOKUP_LINEAR>(method, [&](auto m) {
            with_bool(lds_on, [&](auto l) {
                with_dim(D, [&](auto d) {
                    using TL = typename decltype(tl)::type;
                    constexpr bool LDS = decltype(l)::value;
                    hipLaunchKernelGGL((k_rollout_campaign_pair<decltype(d)::value, TL, decltype(m)::value, LDS>), g, b, LDS ? lds : 0, st, K);
                });
            });
        });
    });
    return hipGetLastError();
}

}  // namespace hjb
