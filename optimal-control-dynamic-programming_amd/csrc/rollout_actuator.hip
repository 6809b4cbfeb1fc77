// rollout_actuator.hip - K33's 72 instantiations (kernels_rollout_actuator.h: label type x method x LDS x D, the set K25 has) in a
// unit of their own, behind launch_rollout_actuator (called by hjb_rollout_run_actuator in rollout.hip).
#include "kernels_rollout_actuator.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_actuator(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, const DActuator &N, int64_t nc,
                                   size_t lds, hipStream_t st, const double *X0, double *Xf, double *cost, double *Xp, double *Up) {
    const dim3 b(256), g((unsigned)((nc + 255) / 256));
    const DActuatorArgs K{R, N, nc, X0, Xf, cost, Xp, Up};
    with_label_type(idx_bytes, [&](auto tl) {
        with_int<HJB_LOOKUP_NEAREST, HJB_LOOKUP_LINEAR>(method, [&](auto m) {
            with_bool(lds_on, [&](auto l) {
                with_dim(D, [&](auto d) {
                    using TL = typename decltype(tl)::type;
                    constexpr bool LDS = decltype(l)::value;
                    hipLaunchKernelGGL((k_rollout_actuator<decltype(d)::value, TL, decltype(m)::value, LDS>), g, b, LDS ? lds : 0, st,
                                       K);
                });
            });
        });
    });
    return hipGetLastError();
}

}  // namespace hjb
