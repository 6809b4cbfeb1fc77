// rollout_position.hip - K19's 6 instantiations (kernels_rollout_position.h: label type x LDS) in a unit of their own, behind
// launch_rollout_position (called by hjb_rollout_run_position in rollout_channels.hip).
#include "kernels_rollout_position.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_position(int idx_bytes, bool lds_on, const DPaChan &CX, const DPaChan &CY, const DPaChan &CZ,
                                   const DPosition &M, int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf, double *Xp,
                                   double *Ap, int32_t *off) {
    const dim3 b(256), g((unsigned)((nc + 255) / 256));
    with_label_type(idx_bytes, [&](auto tl) {
        with_bool(lds_on, [&](auto l) {
            using TL = typename decltype(tl)::type;
            constexpr bool LDS = decltype(l)::value;
            hipLaunchKernelGGL((k_rollout_position<TL, LDS>), g, b, LDS ? lds : 0, st, CX, CY, CZ, M, nc, X0, Xf, Xp, Ap, off);
        });
    });
    return hipGetLastError();
}

}  // namespace hjb
