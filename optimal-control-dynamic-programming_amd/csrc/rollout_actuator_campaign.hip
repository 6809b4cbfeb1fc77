// rollout_actuator_campaign.hip - K34's 72 instantiations (kernels_rollout_actuator_campaign.h: label type x method x LDS x D, the
// set K28 has) in a unit of their own, behind launch_rollout_actuator_campaign (called by hjb_rollout_run_actuator_campaign in
// rollout_campaign_host.hip).  The fold is K28's kernel (launch_campaign_fold, rollout_campaign.hip).
#include "kernels_rollout_actuator_campaign.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_actuator_campaign(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, const DActuator &N,
                                            const DCampaign &Cp, size_t lds, hipStream_t st, const double *X0, double *stats) {
    const int64_t lanes = Cp.n_blocks * Cp.G;
    const dim3 b(256), g((unsigned)((lanes + 255) / 256));
    const DActCampaignArgs K{R, N, Cp, X0};
    with_label_type(idx_bytes, [&](auto tl) {
        with_int<HJB_LOOKUP_NEAREST, HJB_LOOKUP_LINEAR>(method, [&](auto m) {
            with_bool(lds_on, [&](auto l) {
                with_dim(D, [&](auto d) {
                    using TL = typename decltype(tl)::type;
                    constexpr bool LDS = decltype(l)::value;
                    hipLaunchKernelGGL((k_rollout_actuator_campaign<decltype(d)::value, TL, decltype(m)::value, LDS>), g, b,
                                       LDS ? lds : 0, st, K);
                });
            });
        });
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_campaign_fold(Cp, st, stats);
}

}  // namespace hjb
