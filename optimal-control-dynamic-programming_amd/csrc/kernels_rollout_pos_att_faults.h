// kernels_rollout_pos_att_faults.h - K23: thruster-fault campaigns in the 13-state pos-att loop (hjb_rollout_run_pos_att_faults).
//
// K18's stage (kernels_rollout_pos_att_body.inc, the one text both kernels are made of: one thread per trajectory, all n_steps
// stages in one launch, everything in double, left to right, every product rounded) with its fault parts switched on: a fourth
// channel descriptor and three per-trajectory inputs.  Trajectory i at stage k:
//   t_i, xb, vb as in K18;
//   channel x's lookup reads the fault controller CXF (pos-att/Solver_pos_att.m:235-240, channel_x_controller_1_failure; a grid of
//     its own) when switch_stage[i] <= k, else CX: a branch around one HJB_ROLLOUT_LOOKUP each, so a wave whose lanes agree pays
//     for one lookup; channels y and z as in K18; every controller reads plane plane_of_step[k];
//   the commanded forces f[0..11] as in K18; the APPLIED forces fa[j] = (fault_stage[i] <= k && bit j of fault_mask[i]) ? +0.0
//     : f[j] - a select, not a product: a dead thruster applies exactly +0.0 whatever was commanded;
//   U_M, a_body, both inverses and the S RK4 sub-steps are K18's (the same lines) on fa; F_path holds fa (what the plant
//     got), FM_path is formed from fa;
//   impulse: s_k = ((((|fa0| + |fa1|) + |fa2|) + ...) + |fa11|), acc = acc + s_k in stage order, impulse[i] = acc * h after the
//     last stage (h as given to hjb_rollout_set_pos_att_model, not hs * substeps);
//   settling: X_m (m = 0 is X0, m = k + 1 follows stage k) is inside when ((x0 x0 + x1 x1) + x2 x2) <= p2 &&
//     ((q1 q1 + q2 q2) + q3 q3) <= a2 (a NaN state is not inside); settle_stage[i] = 1 + the last m whose X_m is outside (0 when
//     none is, n_steps + 1 when X_n_steps is): one running last_outside per thread.
// With no fault and no hand-over every operation on the state is K18's, so X_final and the paths are K18's bits.  A NULL
// fault_mask is no fault, a NULL fault_stage stage 0, a NULL switch_stage never; a stage >= n_steps never comes.  No atomic, no
// scratch; offsets int64, plain stores, trajectory index fastest.  The numpy restatement is tests/pos_att_fault_rollout_refs.py,
// the scalar host loop hjbdp/rollout.py::pos_att_fault_path_fixed.
#pragma once
#include "kernels_rollout_pos_att.h"

namespace hjb {

// The campaign's per-trajectory inputs and scalar outputs (device pointers of the current chunk; any of them may be null)
struct DPaFault {
    const int32_t *mask, *fault_stage, *switch_stage;     // [nc] each
    double *impulse;                                      // [nc]
    int32_t *settle;                                      // [nc]
    double h, p2, a2;                                     // the model's h; pos_tol^2, att_tol^2
};

__device__ __forceinline__ bool pa_inside(const double (&x)[HJB_PA_W], double p2, double a2) {
    return ((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) <= p2 && ((x[6] * x[6] + x[7] * x[7]) + x[8] * x[8]) <= a2;
}

template <typename TL, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_pos_att_faults(const DPaChan CX, const DPaChan CY, const DPaChan CZ, const DPaChan CXF, const DPosAtt M, const DPaFault Q,
                         int64_t nc, const double *__restrict__ X0, double *__restrict__ Xf, double *__restrict__ Xp,
                         double *__restrict__ Fp, double *__restrict__ FMp) {
#define HJB_PA_BODY_FAULTS 1
#include "kernels_rollout_pos_att_body.inc"
#undef HJB_PA_BODY_FAULTS
}

// rollout_pos_att_faults.hip instantiates the 6 kernels (label type x LDS) and launches the one asked for
hipError_t launch_rollout_pos_att_faults(int idx_bytes, bool lds_on, const DPaChan &CX, const DPaChan &CY, const DPaChan &CZ,
                                         const DPaChan &CXF, const DPosAtt &M, const DPaFault &Q, int64_t nc, size_t lds, hipStream_t st,
                                         const double *X0, double *Xf, double *Xp, double *Fp, double *FMp);

}  // namespace hjb
