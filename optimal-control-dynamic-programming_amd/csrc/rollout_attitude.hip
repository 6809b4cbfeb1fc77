// rollout_attitude.hip - K17's 24 instantiations (kernels_rollout_attitude.h: label type x method x LDS x integrator) in a unit
// of their own, behind launch_rollout_attitude (called by hjb_rollout_run_attitude in rollout.hip).
#include "kernels_rollout_attitude.h"

namespace hjb {

namespace {

template <typename TL, int M, bool LDS, int INTEG>
void launch_i(const DRollout &R, const DAttitude &A, int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf,
              double *cost, double *Xp, double *Up, double *Ap) {
    dim3 b(256), g((unsigned)((nc + 255) / 256));
    hipLaunchKernelGGL((k_rollout_attitude<TL, M, LDS, INTEG>), g, b, LDS ? lds : 0, st, R, A, nc, X0, Xf, cost, Xp, Up, Ap);
}

template <typename TL, int M>
void launch_l(bool lds_on, int integ, const DRollout &R, const DAttitude &A, int64_t nc, size_t lds, hipStream_t st,
              const double *X0, double *Xf, double *cost, double *Xp, double *Up, double *Ap) {
    if (lds_on) {
        if (integ == HJB_ATT_RK4) launch_i<TL, M, true, HJB_ATT_RK4>(R, A, nc, lds, st, X0, Xf, cost, Xp, Up, Ap);
        else launch_i<TL, M, true, HJB_ATT_TAYLOR>(R, A, nc, lds, st, X0, Xf, cost, Xp, Up, Ap);
    } else {
        if (integ == HJB_ATT_RK4) launch_i<TL, M, false, HJB_ATT_RK4>(R, A, nc, lds, st, X0, Xf, cost, Xp, Up, Ap);
        else launch_i<TL, M, false, HJB_ATT_TAYLOR>(R, A, nc, lds, st, X0, Xf, cost, Xp, Up, Ap);
    }
}

template <typename TL>
void launch_m(int method, bool lds_on, int integ, const DRollout &R, const DAttitude &A, int64_t nc, size_t lds, hipStream_t st,
              const double *X0, double *Xf, double *cost, double *Xp, double *Up, double *Ap) {
    if (method == HJB_LOOKUP_NEAREST) launch_l<TL, HJB_LOOKUP_NEAREST>(lds_on, integ, R, A, nc, lds, st, X0, Xf, cost, Xp, Up, Ap);
    else launch_l<TL, HJB_LOOKUP_LINEAR>(lds_on, integ, R, A, nc, lds, st, X0, Xf, cost, Xp, Up, Ap);
}

}  // namespace

hipError_t launch_rollout_attitude(int idx_bytes, int method, bool lds_on, int integrator, const DRollout &R, const DAttitude &M,
                                   int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf, double *cost, double *Xp,
                                   double *Up, double *Ap) {
    switch (idx_bytes) {
        case 1: launch_m<uint8_t>(method, lds_on, integrator, R, M, nc, lds, st, X0, Xf, cost, Xp, Up, Ap); break;
        case 2: launch_m<uint16_t>(method, lds_on, integrator, R, M, nc, lds, st, X0, Xf, cost, Xp, Up, Ap); break;
        default: launch_m<int32_t>(method, lds_on, integrator, R, M, nc, lds, st, X0, Xf, cost, Xp, Up, Ap); break;
    }
    return hipGetLastError();
}

}  // namespace hjb
