// rollout_attitude.hip - K17's 24 instantiations (kernels_rollout_attitude.h: label type x method x LDS x integrator) in a unit
// of their own, behind launch_rollout_attitude (called by hjb_rollout_run_attitude in rollout.hip).
#include "kernels_rollout_attitude.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_attitude(int idx_bytes, int method, bool lds_on, int integrator, const DRollout &R, const DAttitude &M,
                                   int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf, double *cost, double *Xp,
                                   double *Up, double *Ap) {
    const dim3 b(256), g((unsigned)((nc + 255) / 256));
    with_label_type(idx_bytes, [&](auto tl) {
        with_int<HJB_LOOKUP_NEAREST, HJB_LOOKUP_LINEAR>(method, [&](auto m) {
            with_bool(lds_on, [&](auto l) {
                with_int<HJB_ATT_RK4, HJB_ATT_TAYLOR>(integrator, [&](auto integ) {
                    using TL = typename decltype(tl)::type;
                    constexpr bool LDS = decltype(l)::value;
                    hipLaunchKernelGGL((k_rollout_attitude<TL, decltype(m)::value, LDS, decltype(integ)::value>), g, b, LDS ? lds : 0,
                                       st, R, M, nc, X0, Xf, cost, Xp, Up, Ap);
                });
            });
        });
    });
    return hipGetLastError();
}

}  // namespace hjb
