// rollout_attitude_linear.hip - K21's 4 instantiations (kernels_rollout_attitude_linear.h: integrator x cost form) in a unit of
// their own, behind launch_rollout_attitude_linear (called by hjb_attitude_linear_response in rollout.hip).
#include "kernels_rollout_attitude_linear.h"

namespace hjb {

namespace {

template <int INTEG, int COST>
void launch_i(const DAttLinear &M, int64_t nc, hipStream_t st, const double *X0, double *Xf, double *cost, double *Xp, double *Up,
              double *Ap) {
    dim3 b(256), g((unsigned)((nc + 255) / 256));
    hipLaunchKernelGGL((k_rollout_attitude_linear<INTEG, COST>), g, b, 0, st, M, nc, X0, Xf, cost, Xp, Up, Ap);
}

template <int INTEG>
void launch_c(int cost_form, const DAttLinear &M, int64_t nc, hipStream_t st, const double *X0, double *Xf, double *cost, double *Xp,
              double *Up, double *Ap) {
    if (cost_form == HJB_ATTL_COST_ANGLE) launch_i<INTEG, HJB_ATTL_COST_ANGLE>(M, nc, st, X0, Xf, cost, Xp, Up, Ap);
    else launch_i<INTEG, HJB_ATTL_COST_QUAT>(M, nc, st, X0, Xf, cost, Xp, Up, Ap);
}

}  // namespace

hipError_t launch_rollout_attitude_linear(int integrator, int cost_form, const DAttLinear &M, int64_t nc, hipStream_t st,
                                          const double *X0, double *Xf, double *cost, double *Xp, double *Up, double *Ap) {
    if (integrator == HJB_ATT_RK4) launch_c<HJB_ATT_RK4>(cost_form, M, nc, st, X0, Xf, cost, Xp, Up, Ap);
    else launch_c<HJB_ATT_TAYLOR>(cost_form, M, nc, st, X0, Xf, cost, Xp, Up, Ap);
    return hipGetLastError();
}

}  // namespace hjb
