// kernels_rollout_pos_att_faults.h - K23: thruster-fault campaigns in the 13-state pos-att loop (hjb_rollout_run_pos_att_faults).
//
// K18's stage (kernels_rollout_pos_att.h: one thread per trajectory, all n_steps stages in one launch, everything in double, left
// to right, every product rounded) with a fourth channel descriptor and three per-trajectory inputs.  Trajectory i at stage k:
//   t_i, xb, vb as in K18;
//   channel x's lookup reads the fault controller CXF (pos-att/Solver_pos_att.m:235-240, channel_x_controller_1_failure; a grid of
//     its own) when switch_stage[i] <= k, else CX: a branch around one HJB_ROLLOUT_LOOKUP each, so a wave whose lanes agree pays
//     for one lookup; channels y and z as in K18; every controller reads plane plane_of_step[k];
//   the commanded forces f[0..11] as in K18; the APPLIED forces fa[j] = (fault_stage[i] <= k && bit j of fault_mask[i]) ? +0.0
//     : f[j] - a select, not a product: a dead thruster applies exactly +0.0 whatever was commanded;
//   U_M, a_body, both inverses and the S RK4 sub-steps are K18's operations in K18's order on fa; F_path holds fa (what the plant
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
    extern __shared__ double smem[];
    const double *knx, *rdx_, *utx, *kny, *rdy, *uty, *knz, *rdz, *utz, *knf, *rdf, *utf;
    if constexpr (LDS) {
        // per channel [knots | 1/dx | u_table], x then y then z then the fault controller (nothing of it when none is attached)
        const int nkx = CX.n_knots, nky = CY.n_knots, nkz = CZ.n_knots, nkf = CXF.n_knots;
        const int nux = CX.n_labels * 4, nuy = CY.n_labels * 4, nuz = CZ.n_labels * 4, nuf = CXF.n_labels * 4;
        double *sx = smem, *sy = sx + 2 * nkx + nux, *sz = sy + 2 * nky + nuy, *sf = sz + 2 * nkz + nuz;
        for (int e = threadIdx.x; e < nkx; e += blockDim.x) {
            sx[e] = CX.knots[e];
            sx[nkx + e] = CX.rdx[e];
        }
        for (int e = threadIdx.x; e < nux; e += blockDim.x) sx[2 * nkx + e] = CX.u_table[e];
        for (int e = threadIdx.x; e < nky; e += blockDim.x) {
            sy[e] = CY.knots[e];
            sy[nky + e] = CY.rdx[e];
        }
        for (int e = threadIdx.x; e < nuy; e += blockDim.x) sy[2 * nky + e] = CY.u_table[e];
        for (int e = threadIdx.x; e < nkz; e += blockDim.x) {
            sz[e] = CZ.knots[e];
            sz[nkz + e] = CZ.rdx[e];
        }
        for (int e = threadIdx.x; e < nuz; e += blockDim.x) sz[2 * nkz + e] = CZ.u_table[e];
        for (int e = threadIdx.x; e < nkf; e += blockDim.x) {
            sf[e] = CXF.knots[e];
            sf[nkf + e] = CXF.rdx[e];
        }
        for (int e = threadIdx.x; e < nuf; e += blockDim.x) sf[2 * nkf + e] = CXF.u_table[e];
        __syncthreads();
        knx = sx;
        rdx_ = sx + nkx;
        utx = sx + 2 * nkx;
        kny = sy;
        rdy = sy + nky;
        uty = sy + 2 * nky;
        knz = sz;
        rdz = sz + nkz;
        utz = sz + 2 * nkz;
        knf = sf;
        rdf = sf + nkf;
        utf = sf + 2 * nkf;
    } else {
        knx = CX.knots;
        rdx_ = CX.rdx;
        utx = CX.u_table;
        kny = CY.knots;
        rdy = CY.rdx;
        uty = CY.u_table;
        knz = CZ.knots;
        rdz = CZ.rdx;
        utz = CZ.u_table;
        knf = CXF.knots;
        rdf = CXF.rdx;
        utf = CXF.u_table;
    }
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const TL *__restrict__ labx = static_cast<const TL *>(CX.labels);
    const TL *__restrict__ laby = static_cast<const TL *>(CY.labels);
    const TL *__restrict__ labz = static_cast<const TL *>(CZ.labels);
    const TL *__restrict__ labf = static_cast<const TL *>(CXF.labels);
    const int64_t nlx = CX.n_labels, nly = CY.n_labels, nlz = CZ.n_labels, nlf = CXF.n_labels;
    const double hs = M.hs;
    const int S = M.substeps;
    const int n_steps = M.n_steps;
    // a stage that never comes is n_steps: the host let a hand-over before n_steps through only with a fault controller attached
    const int mask = Q.mask ? Q.mask[i] : 0;
    const int fault_at = Q.fault_stage ? Q.fault_stage[i] : 0;
    const int switch_at = Q.switch_stage ? Q.switch_stage[i] : n_steps;
    double x[HJB_PA_W];
#pragma unroll
    for (int a = 0; a < HJB_PA_W; ++a) x[a] = X0[a + (int64_t)HJB_PA_W * i];
    if (Xp) {
#pragma unroll
        for (int a = 0; a < HJB_PA_W; ++a) Xp[i + nc * a] = x[a];
    }
    double imp = 0.0;
    int last_outside = pa_inside(x, Q.p2, Q.a2) ? -1 : 0;
    for (int k = 0; k < n_steps; ++k) {
        double th[3], xb[3], vb[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = x[6 + j];
            s = s > 1.0 ? 1.0 : s < -1.0 ? -1.0 : s;
            th[j] = 2.0 * canon_asin(s);
        }
        {
            double E[9], R[9];
            pa_eci2body(x[6], x[7], x[8], x[9], E);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) R[3 * r + c] = (E[3 * r] * M.RSW[c] + E[3 * r + 1] * M.RSW[3 + c]) + E[3 * r + 2] * M.RSW[6 + c];
            }
            pa_mul3(R, x[0], x[1], x[2], xb);
            pa_mul3(R, x[3], x[4], x[5], vb);
        }
        double f[HJB_PA_F];
        {
            const double p[4] = {xb[0], vb[0], th[1], x[11]};
            if (switch_at <= k) {                                  // the fault controller has taken over
                HJB_ROLLOUT_LOOKUP(4, 4, HJB_LOOKUP_NEAREST, CXF, knf, rdf, utf, labf, k, p, 4, nlf, u)
                f[0] = u[0];
                f[1] = u[1];
                f[6] = u[2];
                f[7] = u[3];
            } else {
                HJB_ROLLOUT_LOOKUP(4, 4, HJB_LOOKUP_NEAREST, CX, knx, rdx_, utx, labx, k, p, 4, nlx, u)
                f[0] = u[0];
                f[1] = u[1];
                f[6] = u[2];
                f[7] = u[3];
            }
        }
        {
            const double p[4] = {xb[1], vb[1], th[2], x[12]};
            HJB_ROLLOUT_LOOKUP(4, 4, HJB_LOOKUP_NEAREST, CY, kny, rdy, uty, laby, k, p, 4, nly, u)
            f[2] = u[0];
            f[3] = u[1];
            f[8] = u[2];
            f[9] = u[3];
        }
        {
            const double p[4] = {xb[2], vb[2], th[0], x[10]};
            HJB_ROLLOUT_LOOKUP(4, 4, HJB_LOOKUP_NEAREST, CZ, knz, rdz, utz, labz, k, p, 4, nlz, u)
            f[4] = u[0];
            f[5] = u[1];
            f[10] = u[2];
            f[11] = u[3];
        }
        // what the plant gets: a dead thruster applies +0.0
        {
            const int dead = fault_at <= k ? mask : 0;
#pragma unroll
            for (int j = 0; j < HJB_PA_F; ++j) f[j] = ((dead >> j) & 1) ? 0.0 : f[j];
        }
        {
            double s = fabs(f[0]) + fabs(f[1]);
#pragma unroll
            for (int j = 2; j < HJB_PA_F; ++j) s = s + fabs(f[j]);
            imp = imp + s;
        }
        double um[3], acc3[3];
        um[0] = (((f[4] - f[5]) + f[10]) - f[11]) * M.t_dist;
        um[1] = (((f[0] - f[1]) + f[6]) - f[7]) * M.t_dist;
        um[2] = (((f[2] - f[3]) + f[8]) - f[9]) * M.t_dist;
        {
            const double ab0 = (((f[0] + f[1]) + f[6]) + f[7]) / M.mass;
            const double ab1 = (((f[2] + f[3]) + f[8]) + f[9]) / M.mass;
            const double ab2 = (((f[4] + f[5]) + f[10]) + f[11]) / M.mass;
            double E[9], Ei[9], ae[3];
            pa_eci2body(x[6], x[7], x[8], x[9], E);
            pa_inv3(E, Ei);
            pa_mul3(Ei, ab0, ab1, ab2, ae);
            pa_mul3(M.RSWinv, ae[0], ae[1], ae[2], acc3);
        }
        if (Fp) {
#pragma unroll
            for (int j = 0; j < HJB_PA_F; ++j) Fp[i + nc * (j + (int64_t)HJB_PA_F * k)] = f[j];
        }
        if (FMp) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                FMp[i + nc * (j + (int64_t)HJB_PA_FM * k)] = acc3[j];
                FMp[i + nc * (3 + j + (int64_t)HJB_PA_FM * k)] = um[j];
            }
        }
        for (int s = 0; s < S; ++s) {
            const double *c = M.coef + 5 * (2 * ((int64_t)S * k + s));
            double r[HJB_PA_W], acc[HJB_PA_W], xt[HJB_PA_W];
            pa_rates(M, c, acc3, um, x, r);                           // k1
#pragma unroll
            for (int a = 0; a < HJB_PA_W; ++a) {
                acc[a] = r[a];
                xt[a] = x[a] + (r[a] * hs) / 2.0;
            }
            pa_rates(M, c + 5, acc3, um, xt, r);                      // k2
#pragma unroll
            for (int a = 0; a < HJB_PA_W; ++a) {
                acc[a] = acc[a] + 2.0 * r[a];
                xt[a] = x[a] + (r[a] * hs) / 2.0;
            }
            pa_rates(M, c + 5, acc3, um, xt, r);                      // k3
#pragma unroll
            for (int a = 0; a < HJB_PA_W; ++a) {
                acc[a] = acc[a] + 2.0 * r[a];
                xt[a] = x[a] + r[a] * hs;
            }
            pa_rates(M, c + 10, acc3, um, xt, r);                     // k4
#pragma unroll
            for (int a = 0; a < HJB_PA_W; ++a) x[a] = x[a] + (hs * (acc[a] + r[a])) / 6.0;
        }
        if (Xp) {
#pragma unroll
            for (int a = 0; a < HJB_PA_W; ++a) Xp[i + nc * (a + (int64_t)HJB_PA_W * (k + 1))] = x[a];
        }
        if (!pa_inside(x, Q.p2, Q.a2)) last_outside = k + 1;
    }
#pragma unroll
    for (int a = 0; a < HJB_PA_W; ++a) Xf[a + (int64_t)HJB_PA_W * i] = x[a];
    if (Q.impulse) Q.impulse[i] = imp * Q.h;
    if (Q.settle) Q.settle[i] = last_outside + 1;
}

// rollout_pos_att_faults.hip instantiates the 6 kernels (label type x LDS) and launches the one asked for
hipError_t launch_rollout_pos_att_faults(int idx_bytes, bool lds_on, const DPaChan &CX, const DPaChan &CY, const DPaChan &CZ,
                                         const DPaChan &CXF, const DPosAtt &M, const DPaFault &Q, int64_t nc, size_t lds, hipStream_t st,
                                         const double *X0, double *Xf, double *Xp, double *Fp, double *FMp);

}  // namespace hjb
