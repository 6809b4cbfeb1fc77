// rollout_attitude_simplified.hip - K20's 12 instantiations (kernels_rollout_attitude_simplified.h: label type x LDS x dynamics)
// in a unit of their own, behind launch_rollout_attitude_simplified (called by hjb_rollout_run_attitude_simplified in rollout_channels.hip).
#include "kernels_rollout_attitude_simplified.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_attitude_simplified(int idx_bytes, bool lds_on, int dynamics, const DPaChan &C1, const DPaChan &C2,
                                              const DPaChan &C3, const DAttSimplified &M, int64_t nc, size_t lds, hipStream_t st,
                                              const double *X0, double *Xf, double *cost, double *Xp, double *Up, double *Ap) {
    const dim3 b(256), g((unsigned)((nc + 255) / 256));
    with_label_type(idx_bytes, [&](auto tl) {
        with_int<HJB_ATTS_FULL, HJB_ATTS_DIAGONAL>(dynamics, [&](auto dyn) {
            with_bool(lds_on, [&](auto l) {
                using TL = typename decltype(tl)::type;
                constexpr bool LDS = decltype(l)::value;
                hipLaunchKernelGGL((k_rollout_attitude_simplified<TL, LDS, decltype(dyn)::value>), g, b, LDS ? lds : 0, st, C1, C2, C3,
                                   M, nc, X0, Xf, cost, Xp, Up, Ap);
            });
        });
    });
    return hipGetLastError();
}

}  // namespace hjb
