// kernels_rollout_position.h - K19: batched closed-loop rollouts of Solver_position's RKF45 loop (hjb_rollout_run_position).
//
// position-control/Solver_position.m:189-311 (get_optimal_path after simplified_run) for many initial states at once: one thread
// per trajectory, all n_steps stages in one launch, everything in double, left to right, every product rounded
// (-ffp-contract=off).  The state is y = [x(3) v(3)] in the target's co-moving frame.  Per stage k:
//   three 'nearest' lookups with K16's HJB_ROLLOUT_LOOKUP (D = 2, n_u = 1) on plane plane_of_step[k]: channel i at (y_i, y_3+i)
//     gives the acceleration a_i (:215-217), held over the stage;
//   the stage's n_sub[k] sub-steps of private/rkf45.m ON ITS SCHEDULE: at the reference's h every error test passes by seven
//     orders of magnitude, so every step is accepted and grows fourfold, and the step sizes depend on the stage's t0 and tf alone
//     (hjbdp/rollout.py::position_rkf45_schedule).  Sub-step s of stage k reads 32 doubles of the host-built table, the same
//     for the whole wave: h_form, h_apply and the five orbit scalars of pa_rates (K18) at the six times t_s + a_j h_form
//     (hjbdp/orbit.py stays the only Kepler solver).  With B, C4, C5 Fehlberg's tableau:
//       f_0 = F(c_0, y);  f_i = F(c_i, (..(y + (h_form B_i0) f_0) + ..) + (h_form B_i,i-1) f_i-1), i = 1..5
//       e_i = (((f_0i d_0 + f_2i d_2) + f_3i d_3) + f_4i d_4) + f_5i d_5, d = C4 - C5 (d_1 = 0: no term);  te = max_i |h_form e_i|
//       allowed = tol * max(max_i |y_i|, 1)        (both maxima keep a NaN once met)
//       on schedule iff allowed >= 1100 (te + eps): 1100 > 4^5 leaves room for the rounding of rkf45's pow(., 0.2), so a step
//         rkf45 would not have grown fourfold is never missed; NaN fails the test.  The first stage that fails goes to
//         off_schedule (-1: none); the run goes on along the schedule either way, so the work per trajectory is bounded.
//       y_i += h_apply ((((f_0i C5_0 + f_2i C5_2) + f_3i C5_3) + f_4i C5_4) + f_5i C5_5)
//     h_apply < h_form in a stage's last sub-step: rkf45 clips an accepted step to the end of the interval after its stage
//     derivatives were formed with the unclipped one, and so does this.
// The six stage derivatives (36 doubles) stay in registers.  Labels were range-checked by hjb_rollout_create and find_cell clamps
// every query (NaN -> cell 0), so a state that leaves the grids or stops being finite reads inside the label arrays.  The numpy
// restatement is tests/position_rollout_refs.py, the scalar host loop hjbdp/rollout.py::position_optimal_path_fixed.
#pragma once
#include "hjbdp_dev.h"
#include "kernels_rollout.h"
#include "kernels_rollout_pos_att.h"   // DPaChan: what HJB_ROLLOUT_LOOKUP reads of a channel (axes 0 and 1 used here)

namespace hjb {

#define HJB_POS_W 6                   // state width
#define HJB_POS_A 3                   // accelerations per stage
#define HJB_POS_ROW 32                // table doubles per sub-step: h_form, h_apply, 6 x 5 orbit scalars
#define HJB_POS_MAX_SUB 8             // sub-steps per stage the table may hold

struct DPosition {
    double tol;
    int32_t n_steps, max_sub;
    const int32_t *n_sub;             // [n_steps] (global)
    const double *table;              // [HJB_POS_ROW, max_sub, n_steps] column-major (global)
};

// the translational part of pa_rates at one table node c
__device__ __forceinline__ void pos_rates(const double *__restrict__ c, const double (&a)[3], const double (&y)[HJB_POS_W],
                                          double (&f)[HJB_POS_W]) {
    const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4];
    f[0] = y[3];
    f[1] = y[4];
    f[2] = y[5];
    f[3] = ((c0 * y[0] - c1 * y[1]) + c2 * y[4]) + a[0];
    f[4] = ((c1 * y[0] - c3 * y[1]) - c2 * y[3]) + a[1];
    f[5] = a[2] - c4 * y[2];
}

// max(m, |v|) that keeps a NaN once met (numpy's max, not fmax)
__device__ __forceinline__ double pos_absmax(double m, double v) {
    v = v < 0.0 ? -v : v;
    return (v > m || v != v) ? v : m;
}

template <typename TL, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_position(const DPaChan CX, const DPaChan CY, const DPaChan CZ, const DPosition M, int64_t nc, const double *__restrict__ X0,
                   double *__restrict__ Xf, double *__restrict__ Xp, double *__restrict__ Ap, int32_t *__restrict__ off) {
    // Fehlberg's 4(5) tableau (hjbdp/orbit.py _B, _C4, _C5); row i of B starts at i (i - 1) / 2
    constexpr double B[15] = {1.0 / 4,
                              3.0 / 32, 9.0 / 32,
                              1932.0 / 2197, -7200.0 / 2197, 7296.0 / 2197,
                              439.0 / 216, -8.0, 3680.0 / 513, -845.0 / 4104,
                              -8.0 / 27, 2.0, -3544.0 / 2565, 1859.0 / 4104, -11.0 / 40};
    constexpr double C4[6] = {25.0 / 216, 0.0, 1408.0 / 2565, 2197.0 / 4104, -1.0 / 5, 0.0};
    constexpr double C5[6] = {16.0 / 135, 0.0, 6656.0 / 12825, 28561.0 / 56430, -9.0 / 50, 2.0 / 55};
    constexpr double EPS = 2.220446049250313e-16;
    extern __shared__ double smem[];
    const double *knx, *rdx_, *utx, *kny, *rdy, *uty, *knz, *rdz, *utz;
    // per channel [knots | 1/dx | u_table], x then y then z
    HJB_ROLLOUT_PLACE(x, CX, 1, smem)
    HJB_ROLLOUT_PLACE(y, CY, 1, HJB_ROLLOUT_PLACE_END(x))
    HJB_ROLLOUT_PLACE(z, CZ, 1, HJB_ROLLOUT_PLACE_END(y))
    HJB_ROLLOUT_STAGE(LDS, x, CX, knx, rdx_, utx)
    HJB_ROLLOUT_STAGE(LDS, y, CY, kny, rdy, uty)
    HJB_ROLLOUT_STAGE(LDS, z, CZ, knz, rdz, utz)
    if constexpr (LDS) __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const TL *__restrict__ labx = static_cast<const TL *>(CX.labels);
    const TL *__restrict__ laby = static_cast<const TL *>(CY.labels);
    const TL *__restrict__ labz = static_cast<const TL *>(CZ.labels);
    const int64_t nlx = CX.n_labels, nly = CY.n_labels, nlz = CZ.n_labels;
    const double tol = M.tol;
    double y[HJB_POS_W];
#pragma unroll
    for (int a = 0; a < HJB_POS_W; ++a) y[a] = X0[a + (int64_t)HJB_POS_W * i];
    if (Xp) {
#pragma unroll
        for (int a = 0; a < HJB_POS_W; ++a) Xp[i + nc * a] = y[a];
    }
    int32_t first_off = -1;
    for (int k = 0; k < M.n_steps; ++k) {
        double acc[3];
        {
            const double p[2] = {y[0], y[3]};
            HJB_ROLLOUT_LOOKUP(2, 1, HJB_LOOKUP_NEAREST, CX, knx, rdx_, utx, labx, k, p, 1, nlx, u)
            acc[0] = u[0];
        }
        {
            const double p[2] = {y[1], y[4]};
            HJB_ROLLOUT_LOOKUP(2, 1, HJB_LOOKUP_NEAREST, CY, kny, rdy, uty, laby, k, p, 1, nly, u)
            acc[1] = u[0];
        }
        {
            const double p[2] = {y[2], y[5]};
            HJB_ROLLOUT_LOOKUP(2, 1, HJB_LOOKUP_NEAREST, CZ, knz, rdz, utz, labz, k, p, 1, nlz, u)
            acc[2] = u[0];
        }
        if (Ap) {
#pragma unroll
            for (int j = 0; j < HJB_POS_A; ++j) Ap[i + nc * (j + (int64_t)HJB_POS_A * k)] = acc[j];
        }
        const int ns = M.n_sub[k];
        bool on = true;
        for (int s = 0; s < ns; ++s) {
            const double *row = M.table + HJB_POS_ROW * ((int64_t)M.max_sub * k + s);
            const double hf = row[0], ha = row[1];
            double f[6][HJB_POS_W];
            pos_rates(row + 2, acc, y, f[0]);
#pragma unroll
            for (int st = 1; st < 6; ++st) {
                double yin[HJB_POS_W];
#pragma unroll
                for (int a = 0; a < HJB_POS_W; ++a) yin[a] = y[a];
#pragma unroll
                for (int j = 0; j < st; ++j) {
                    const double hb = hf * B[st * (st - 1) / 2 + j];
#pragma unroll
                    for (int a = 0; a < HJB_POS_W; ++a) yin[a] = yin[a] + hb * f[j][a];
                }
                pos_rates(row + 2 + 5 * st, acc, yin, f[st]);
            }
            double te = 0.0, ym = 1.0;
#pragma unroll
            for (int a = 0; a < HJB_POS_W; ++a) {
                const double e = (((f[0][a] * (C4[0] - C5[0]) + f[2][a] * (C4[2] - C5[2])) + f[3][a] * (C4[3] - C5[3])) +
                                  f[4][a] * (C4[4] - C5[4])) + f[5][a] * (C4[5] - C5[5]);
                te = pos_absmax(te, hf * e);
                ym = pos_absmax(ym, y[a]);
            }
            if (!(tol * ym >= 1100.0 * (te + EPS))) on = false;
#pragma unroll
            for (int a = 0; a < HJB_POS_W; ++a)
                y[a] = y[a] + ha * ((((f[0][a] * C5[0] + f[2][a] * C5[2]) + f[3][a] * C5[3]) + f[4][a] * C5[4]) + f[5][a] * C5[5]);
        }
        if (!on && first_off < 0) first_off = k;
        if (Xp) {
#pragma unroll
            for (int a = 0; a < HJB_POS_W; ++a) Xp[i + nc * (a + (int64_t)HJB_POS_W * (k + 1))] = y[a];
        }
    }
#pragma unroll
    for (int a = 0; a < HJB_POS_W; ++a) Xf[a + (int64_t)HJB_POS_W * i] = y[a];
    off[i] = first_off;
}

// rollout_position.hip instantiates the 6 kernels (label type x LDS) and launches the one asked for
hipError_t launch_rollout_position(int idx_bytes, bool lds_on, const DPaChan &CX, const DPaChan &CY, const DPaChan &CZ,
                                   const DPosition &M, int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf, double *Xp,
                                   double *Ap, int32_t *off);

}  // namespace hjb
