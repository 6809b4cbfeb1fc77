// rollout_attitude_linear.hip - K21's 4 instantiations (kernels_rollout_attitude_linear.h: integrator x cost form) in a unit of
// their own, behind launch_rollout_attitude_linear (called by hjb_attitude_linear_response in rollout.hip).
#include "kernels_rollout_attitude_linear.h"
#include "rollout_dispatch.h"

namespace hjb {

hipError_t launch_rollout_attitude_linear(int integrator, int cost_form, const DAttLinear &M, int64_t nc, hipStream_t st,
                                          const double *X0, double *Xf, double *cost, double *Xp, double *Up, double *Ap) {
    const dim3 b(256), g((unsigned)((nc + 255) / 256));
    with_int<HJB_ATT_RK4, HJB_ATT_TAYLOR>(integrator, [&](auto integ) {
        with_int<HJB_ATTL_COST_ANGLE, HJB_ATTL_COST_QUAT>(cost_form, [&](auto cf) {
            hipLaunchKernelGGL((k_rollout_attitude_linear<decltype(integ)::value, decltype(cf)::value>), g, b, 0, st, M, nc, X0, Xf,
                               cost, Xp, Up, Ap);
        });
    });
    return hipGetLastError();
}

}  // namespace hjb
