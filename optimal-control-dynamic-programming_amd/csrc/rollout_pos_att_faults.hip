// rollout_pos_att_faults.hip - K23's 6 instantiations (kernels_rollout_pos_att_faults.h: label type x LDS) in a unit of their own,
// behind launch_rollout_pos_att_faults (called by hjb_rollout_run_pos_att_faults in rollout.hip).
#include "kernels_rollout_pos_att_faults.h"

namespace hjb {

namespace {

template <typename TL, bool LDS>
void launch_i(const DPaChan &CX, const DPaChan &CY, const DPaChan &CZ, const DPaChan &CXF, const DPosAtt &M, const DPaFault &Q,
              int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf, double *Xp, double *Fp, double *FMp) {
    dim3 b(256), g((unsigned)((nc + 255) / 256));
    hipLaunchKernelGGL((k_rollout_pos_att_faults<TL, LDS>), g, b, LDS ? lds : 0, st, CX, CY, CZ, CXF, M, Q, nc, X0, Xf, Xp, Fp, FMp);
}

template <typename TL>
void launch_l(bool lds_on, const DPaChan &CX, const DPaChan &CY, const DPaChan &CZ, const DPaChan &CXF, const DPosAtt &M,
              const DPaFault &Q, int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf, double *Xp, double *Fp,
              double *FMp) {
    if (lds_on) launch_i<TL, true>(CX, CY, CZ, CXF, M, Q, nc, lds, st, X0, Xf, Xp, Fp, FMp);
    else launch_i<TL, false>(CX, CY, CZ, CXF, M, Q, nc, lds, st, X0, Xf, Xp, Fp, FMp);
}

}  // namespace

hipError_t launch_rollout_pos_att_faults(int idx_bytes, bool lds_on, const DPaChan &CX, const DPaChan &CY, const DPaChan &CZ,
                                         const DPaChan &CXF, const DPosAtt &M, const DPaFault &Q, int64_t nc, size_t lds, hipStream_t st,
                                         const double *X0, double *Xf, double *Xp, double *Fp, double *FMp) {
    switch (idx_bytes) {
        case 1: launch_l<uint8_t>(lds_on, CX, CY, CZ, CXF, M, Q, nc, lds, st, X0, Xf, Xp, Fp, FMp); break;
        case 2: launch_l<uint16_t>(lds_on, CX, CY, CZ, CXF, M, Q, nc, lds, st, X0, Xf, Xp, Fp, FMp); break;
        default: launch_l<int32_t>(lds_on, CX, CY, CZ, CXF, M, Q, nc, lds, st, X0, Xf, Xp, Fp, FMp); break;
    }
    return hipGetLastError();
}

}  // namespace hjb
