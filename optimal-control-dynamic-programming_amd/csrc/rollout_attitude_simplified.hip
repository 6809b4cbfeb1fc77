// rollout_attitude_simplified.hip - K20's 12 instantiations (kernels_rollout_attitude_simplified.h: label type x LDS x dynamics)
// in a unit of their own, behind launch_rollout_attitude_simplified (called by hjb_rollout_run_attitude_simplified in rollout.hip).
#include "kernels_rollout_attitude_simplified.h"

namespace hjb {

namespace {

template <typename TL, bool LDS, int DYN>
void launch_i(const DPaChan &C1, const DPaChan &C2, const DPaChan &C3, const DAttSimplified &M, int64_t nc, size_t lds, hipStream_t st,
              const double *X0, double *Xf, double *cost, double *Xp, double *Up, double *Ap) {
    dim3 b(256), g((unsigned)((nc + 255) / 256));
    hipLaunchKernelGGL((k_rollout_attitude_simplified<TL, LDS, DYN>), g, b, LDS ? lds : 0, st, C1, C2, C3, M, nc, X0, Xf, cost, Xp, Up,
                       Ap);
}

template <typename TL>
void launch_l(bool lds_on, int dynamics, const DPaChan &C1, const DPaChan &C2, const DPaChan &C3, const DAttSimplified &M, int64_t nc,
              size_t lds, hipStream_t st, const double *X0, double *Xf, double *cost, double *Xp, double *Up, double *Ap) {
    if (dynamics == HJB_ATTS_FULL) {
        if (lds_on) launch_i<TL, true, HJB_ATTS_FULL>(C1, C2, C3, M, nc, lds, st, X0, Xf, cost, Xp, Up, Ap);
        else launch_i<TL, false, HJB_ATTS_FULL>(C1, C2, C3, M, nc, lds, st, X0, Xf, cost, Xp, Up, Ap);
    } else {
        if (lds_on) launch_i<TL, true, HJB_ATTS_DIAGONAL>(C1, C2, C3, M, nc, lds, st, X0, Xf, cost, Xp, Up, Ap);
        else launch_i<TL, false, HJB_ATTS_DIAGONAL>(C1, C2, C3, M, nc, lds, st, X0, Xf, cost, Xp, Up, Ap);
    }
}

}  // namespace

hipError_t launch_rollout_attitude_simplified(int idx_bytes, bool lds_on, int dynamics, const DPaChan &C1, const DPaChan &C2,
                                              const DPaChan &C3, const DAttSimplified &M, int64_t nc, size_t lds, hipStream_t st,
                                              const double *X0, double *Xf, double *cost, double *Xp, double *Up, double *Ap) {
    switch (idx_bytes) {
        case 1: launch_l<uint8_t>(lds_on, dynamics, C1, C2, C3, M, nc, lds, st, X0, Xf, cost, Xp, Up, Ap); break;
        case 2: launch_l<uint16_t>(lds_on, dynamics, C1, C2, C3, M, nc, lds, st, X0, Xf, cost, Xp, Up, Ap); break;
        default: launch_l<int32_t>(lds_on, dynamics, C1, C2, C3, M, nc, lds, st, X0, Xf, cost, Xp, Up, Ap); break;
    }
    return hipGetLastError();
}

}  // namespace hjb
