// kernels_rollout_attitude_simplified.h - K20: batched closed-loop rollouts of the simplified attitude loop
// (hjb_rollout_run_attitude_simplified).
//
// attitude-control/Solver_attitude.m:835-925 (get_optimal_path_simplified_testode45 after simplified_run) and
// attitude-control/test/test_simplified.m:188-218 ("test on REAL SYSTEM DYNAMICS") for many initial attitudes at once: one thread
// per trajectory, all n_steps stages in one launch, everything in double, left to right, every product rounded
// (-ffp-contract=off).  The state is the reference's X = [w1 w2 w3 q1 q2 q3 q4] (q4 scalar).  Per stage k, p = plane_of_step[k]:
//   t_i = 2 * canon_asin(clamp(X[3+i], -1, 1)), i = 0..2 (:847-849; K17's asin, K18's clamp: the reference would go complex);
//   u_i = channel i's 'nearest' lookup with K16's HJB_ROLLOUT_LOOKUP (D = 2, n_u = 1) on plane p at (X[i], t_i);
//   g_i = (qw_i * (X[i] * X[i]) + qt_i * (t_i * t_i)) + r_i * (u_i * u_i)   (the stage cost of the 2-D sweeps, :220);
//   cost = cost + ((g_0 + g_1) + g_2);
//   then, with u held over the stage,
//   HJB_ATTS_FULL: S classical RK4 sub-steps of hs = h / S in K18's form (xt = x + (f * hs) / 2, x = x + (hs * (acc + f)) / 6) of
//       w_dot = Jinv (u - w x (J w)), Jinv = pa_inv3(J) formed once on the host, both products by pa_mul3 (:912; K18's pa_rates),
//       q_dot in K18's operation order: 0.5 * (((w3 * q2) - (w2 * q3)) + (w1 * q4)), ... (:918-921).
//     The quaternion is NOT renormalised, as in the reference.
//   HJB_ATTS_DIAGONAL: ONE classical RK4 step of h in K17's form with K17's right-hand side attitude_rates at (J1, J2, J3) =
//       diag(inertia) (test_simplified.m:317-356), then X4..X7 /= sqrt(((X4*X4 + X5*X5) + X6*X6) + X7*X7) as K17 does.
// No RK4 temporary is live across the lookups.  Labels were range-checked by hjb_rollout_create and find_cell clamps every query
// (NaN -> cell 0), so a state that leaves the grids or stops being finite reads inside the label arrays.  The numpy restatement
// is tests/attitude_simplified_rollout_refs.py, the scalar host loop hjbdp/rollout.py::attitude_optimal_path_simplified_fixed.
#pragma once
#include "hjbdp_dev.h"
#include "kernels_rollout.h"
#include "kernels_rollout_attitude.h"   // canon_asin, DAttitude, attitude_rates
#include "kernels_rollout_pos_att.h"    // DPaChan (axes 0 and 1 used here), pa_mul3

namespace hjb {

struct DAttSimplified {
    double J[9], Jinv[9];             // row-major: J[3 r + c] (FULL)
    DAttitude A;                      // h, J[3] = diag(inertia) and c[3] (DIAGONAL); its q and r are not read
    double qw[3], qt[3], r[3];        // NULL on the host side = zeros
    double hs;                        // h / substeps
    int32_t substeps, n_steps;
};

// f(X, u) of Solver_attitude.m:902-922: the rotational part of K18's pa_rates
__device__ __forceinline__ void atts_rates(const DAttSimplified &M, const double (&u)[3], const double (&y)[HJB_ATT_W],
                                           double (&f)[HJB_ATT_W]) {
    const double w1 = y[0], w2 = y[1], w3 = y[2], q1 = y[3], q2 = y[4], q3 = y[5], q4 = y[6];
    double jw[3], t[3], wd[3];
    pa_mul3(M.J, w1, w2, w3, jw);
    t[0] = u[0] - (w2 * jw[2] - w3 * jw[1]);
    t[1] = u[1] - (w3 * jw[0] - w1 * jw[2]);
    t[2] = u[2] - (w1 * jw[1] - w2 * jw[0]);
    pa_mul3(M.Jinv, t[0], t[1], t[2], wd);
    f[0] = wd[0];
    f[1] = wd[1];
    f[2] = wd[2];
    f[3] = 0.5 * (((w3 * q2) - (w2 * q3)) + (w1 * q4));
    f[4] = 0.5 * (((w1 * q3) - (w3 * q1)) + (w2 * q4));
    f[5] = 0.5 * (((w2 * q1) - (w1 * q2)) + (w3 * q4));
    f[6] = 0.5 * (((-(w1 * q1)) - (w2 * q2)) - (w3 * q3));
}

template <typename TL, bool LDS, int DYN>
__global__ void __launch_bounds__(256)
k_rollout_attitude_simplified(const DPaChan C1, const DPaChan C2, const DPaChan C3, const DAttSimplified M, int64_t nc,
                              const double *__restrict__ X0, double *__restrict__ Xf, double *__restrict__ cost,
                              double *__restrict__ Xp, double *__restrict__ Up, double *__restrict__ Ap) {
    extern __shared__ double smem[];
    const double *kn1, *rd1, *ut1, *kn2, *rd2, *ut2, *kn3, *rd3, *ut3;
    // per channel [knots | 1/dx | u_table], 1 then 2 then 3
    HJB_ROLLOUT_PLACE(1, C1, 1, smem)
    HJB_ROLLOUT_PLACE(2, C2, 1, HJB_ROLLOUT_PLACE_END(1))
    HJB_ROLLOUT_PLACE(3, C3, 1, HJB_ROLLOUT_PLACE_END(2))
    HJB_ROLLOUT_STAGE(LDS, 1, C1, kn1, rd1, ut1)
    HJB_ROLLOUT_STAGE(LDS, 2, C2, kn2, rd2, ut2)
    HJB_ROLLOUT_STAGE(LDS, 3, C3, kn3, rd3, ut3)
    if constexpr (LDS) __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const TL *__restrict__ lab1 = static_cast<const TL *>(C1.labels);
    const TL *__restrict__ lab2 = static_cast<const TL *>(C2.labels);
    const TL *__restrict__ lab3 = static_cast<const TL *>(C3.labels);
    const int64_t nl1 = C1.n_labels, nl2 = C2.n_labels, nl3 = C3.n_labels;
    double x[HJB_ATT_W];
#pragma unroll
    for (int a = 0; a < HJB_ATT_W; ++a) x[a] = X0[a + (int64_t)HJB_ATT_W * i];
    if (Xp) {
#pragma unroll
        for (int a = 0; a < HJB_ATT_W; ++a) Xp[i + nc * a] = x[a];
    }
    double J = 0.0;
    for (int k = 0; k < M.n_steps; ++k) {
        double th[3], u[HJB_ATT_U];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = x[3 + j];
            s = s > 1.0 ? 1.0 : s < -1.0 ? -1.0 : s;
            th[j] = 2.0 * canon_asin(s);
        }
        if (Ap) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Ap[i + nc * (j + (int64_t)3 * k)] = th[j];
        }
        {
            const double p[2] = {x[0], th[0]};
            HJB_ROLLOUT_LOOKUP(2, 1, HJB_LOOKUP_NEAREST, C1, kn1, rd1, ut1, lab1, k, p, 1, nl1, uo)
            u[0] = uo[0];
        }
        {
            const double p[2] = {x[1], th[1]};
            HJB_ROLLOUT_LOOKUP(2, 1, HJB_LOOKUP_NEAREST, C2, kn2, rd2, ut2, lab2, k, p, 1, nl2, uo)
            u[1] = uo[0];
        }
        {
            const double p[2] = {x[2], th[2]};
            HJB_ROLLOUT_LOOKUP(2, 1, HJB_LOOKUP_NEAREST, C3, kn3, rd3, ut3, lab3, k, p, 1, nl3, uo)
            u[2] = uo[0];
        }
        {
            double g[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) g[j] = (M.qw[j] * (x[j] * x[j]) + M.qt[j] * (th[j] * th[j])) + M.r[j] * (u[j] * u[j]);
            J = J + ((g[0] + g[1]) + g[2]);
        }
        if (Up) {
#pragma unroll
            for (int j = 0; j < HJB_ATT_U; ++j) Up[i + nc * (j + (int64_t)HJB_ATT_U * k)] = u[j];
        }
        if constexpr (DYN == HJB_ATTS_FULL) {
            const double hs = M.hs;
            for (int s = 0; s < M.substeps; ++s) {
#define HJB_ATTS_RHS(j_, y_, r_) atts_rates(M, u, y_, r_)
                HJB_ROLLOUT_RK4_STEP(HJB_ATT_W, x, x, hs, HJB_ATTS_RHS)
#undef HJB_ATTS_RHS
            }
        } else {
            const double h = M.A.h;
#define HJB_ATTS_RHS(j_, y_, r_) attitude_rates(M.A, y_, u, r_)
            HJB_ROLLOUT_RK4_STEP(HJB_ATT_W, x, x, h, HJB_ATTS_RHS)
#undef HJB_ATTS_RHS
            const double nrm = __builtin_sqrt(((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) + x[6] * x[6]);
#pragma unroll
            for (int a = 3; a < HJB_ATT_W; ++a) x[a] = x[a] / nrm;
        }
        if (Xp) {
#pragma unroll
            for (int a = 0; a < HJB_ATT_W; ++a) Xp[i + nc * (a + (int64_t)HJB_ATT_W * (k + 1))] = x[a];
        }
    }
#pragma unroll
    for (int a = 0; a < HJB_ATT_W; ++a) Xf[a + (int64_t)HJB_ATT_W * i] = x[a];
    if (cost) cost[i] = J;
}

// rollout_attitude_simplified.hip instantiates the 12 kernels (label type x LDS x dynamics) and launches the one asked for
hipError_t launch_rollout_attitude_simplified(int idx_bytes, bool lds_on, int dynamics, const DPaChan &C1, const DPaChan &C2,
                                              const DPaChan &C3, const DAttSimplified &M, int64_t nc, size_t lds, hipStream_t st,
                                              const double *X0, double *Xf, double *cost, double *Xp, double *Up, double *Ap);

}  // namespace hjb
