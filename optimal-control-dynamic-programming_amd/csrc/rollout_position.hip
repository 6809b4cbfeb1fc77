// rollout_position.hip - K19's 6 instantiations (kernels_rollout_position.h: label type x LDS) in a unit of their own, behind
// launch_rollout_position (called by hjb_rollout_run_position in rollout.hip).
#include "kernels_rollout_position.h"

namespace hjb {

namespace {

template <typename TL, bool LDS>
void launch_i(const DPaChan &CX, const DPaChan &CY, const DPaChan &CZ, const DPosition &M, int64_t nc, size_t lds, hipStream_t st,
              const double *X0, double *Xf, double *Xp, double *Ap, int32_t *off) {
    dim3 b(256), g((unsigned)((nc + 255) / 256));
    hipLaunchKernelGGL((k_rollout_position<TL, LDS>), g, b, LDS ? lds : 0, st, CX, CY, CZ, M, nc, X0, Xf, Xp, Ap, off);
}

template <typename TL>
void launch_l(bool lds_on, const DPaChan &CX, const DPaChan &CY, const DPaChan &CZ, const DPosition &M, int64_t nc, size_t lds,
              hipStream_t st, const double *X0, double *Xf, double *Xp, double *Ap, int32_t *off) {
    if (lds_on) launch_i<TL, true>(CX, CY, CZ, M, nc, lds, st, X0, Xf, Xp, Ap, off);
    else launch_i<TL, false>(CX, CY, CZ, M, nc, lds, st, X0, Xf, Xp, Ap, off);
}

}  // namespace

hipError_t launch_rollout_position(int idx_bytes, bool lds_on, const DPaChan &CX, const DPaChan &CY, const DPaChan &CZ,
                                   const DPosition &M, int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf, double *Xp,
                                   double *Ap, int32_t *off) {
    switch (idx_bytes) {
        case 1: launch_l<uint8_t>(lds_on, CX, CY, CZ, M, nc, lds, st, X0, Xf, Xp, Ap, off); break;
        case 2: launch_l<uint16_t>(lds_on, CX, CY, CZ, M, nc, lds, st, X0, Xf, Xp, Ap, off); break;
        default: launch_l<int32_t>(lds_on, CX, CY, CZ, M, nc, lds, st, X0, Xf, Xp, Ap, off); break;
    }
    return hipGetLastError();
}

}  // namespace hjb
