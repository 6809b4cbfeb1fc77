// kernels_rollout_attitude_linear.h - K21: batched closed-loop rollouts of the linear attitude controller
// (hjb_attitude_linear_response).
//
// attitude-control/Solver_attitude.m:508-591 (linear_control_response, the PD law the DP controllers are judged against) for many
// initial attitudes at once: one thread per trajectory, all n_steps steps in one launch, everything in double, left to right,
// every product rounded (-ffp-contract=off).  No policy, no LDS, no labels: K17's kernel (kernels_rollout_attitude.h) with the
// lookup replaced by the control law.  The state is the reference's X = [w1 w2 w3 q1 q2 q3 q4] (q4 scalar).  Per step k:
//   qe_i = ((qc[i,0]*X4 + qc[i,1]*X5) + qc[i,2]*X6) + qc[i,3]*X7, i = 0..2 (:536; row 3 of qc is not used by the law);
//   u_i = (-((K[i,0]*qe_0 + K[i,1]*qe_1) + K[i,2]*qe_2)) - ((C[i,0]*X1 + C[i,1]*X2) + C[i,2]*X3)   (:538);
//   with a limit: u_i = u_i > L_i ? L_i : u_i < -L_i ? -L_i : u_i (a NaN passes through);
//   A_path[., k] = attitude_angles(X) (yaw, pitch, roll, :540), computed only when the path is asked for;
//   HJB_ATTL_COST_QUAT:  cost += ((w[0]*(X1*X1) + w[1]*(X2*X2)) + ... + w[6]*(X7*X7)) + w[7]*(u1*u1) + w[8]*(u2*u2) + w[9]*(u3*u3)
//                        (K17's sum);
//   HJB_ATTL_COST_ANGLE: t_i = 2 * canon_asin(clamp(X[3+i], -1, 1)); g_i = (w[i]*(X[i]*X[i]) + w[3+i]*(t_i*t_i)) + w[6+i]*(u_i*u_i);
//                        cost += (g_0 + g_1) + g_2   (K20's sum);
//   X+ = K17's step with u held: X + h f(X, u) ('taylor') or classical RK4, f = attitude_rates; then
//   X4..X7 /= sqrt(((X4*X4 + X5*X5) + X6*X6) + X7*X7).
// With K = 0.2 I, C = I, qc = I this is hjbdp/rollout.py::linear_control_response up to the sign of a zero torque; the numpy
// restatement is tests/attitude_linear_rollout_refs.py.
#pragma once
#include "hjbdp_dev.h"
#include "kernels_rollout_attitude.h"   // HJB_ATT_W / _U, DAttitude, canon_asin, attitude_angles, attitude_rates

namespace hjb {

struct DAttLinear {
    DAttitude A;                      // h, J[3], c[3]; its q and r are not read
    double K[9], C[9];                // row-major: K[3 i + j]
    double qc[12];                    // rows 0..2 of qc, row-major: qc[4 i + j]
    double L[3];                      // the torque limit, read when has_limit
    double w[10];                     // the stage-cost weights in the order of the cost form
    int32_t has_limit, n_steps;
};

template <int INTEG, int COST>
__global__ void __launch_bounds__(256)
k_rollout_attitude_linear(const DAttLinear M, int64_t nc, const double *__restrict__ X0, double *__restrict__ Xf,
                          double *__restrict__ cost, double *__restrict__ Xp, double *__restrict__ Up, double *__restrict__ Ap) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const double h = M.A.h;
    double x[HJB_ATT_W];
#pragma unroll
    for (int a = 0; a < HJB_ATT_W; ++a) x[a] = X0[a + (int64_t)HJB_ATT_W * i];
    if (Xp) {
#pragma unroll
        for (int a = 0; a < HJB_ATT_W; ++a) Xp[i + nc * a] = x[a];
    }
    double J = 0.0;
    for (int k = 0; k < M.n_steps; ++k) {
        double qe[3], u[HJB_ATT_U];
#pragma unroll
        for (int j = 0; j < 3; ++j)
            qe[j] = ((M.qc[4 * j] * x[3] + M.qc[4 * j + 1] * x[4]) + M.qc[4 * j + 2] * x[5]) + M.qc[4 * j + 3] * x[6];
#pragma unroll
        for (int j = 0; j < HJB_ATT_U; ++j)
            u[j] = (-((M.K[3 * j] * qe[0] + M.K[3 * j + 1] * qe[1]) + M.K[3 * j + 2] * qe[2])) -
                   ((M.C[3 * j] * x[0] + M.C[3 * j + 1] * x[1]) + M.C[3 * j + 2] * x[2]);
        if (M.has_limit) {
#pragma unroll
            for (int j = 0; j < HJB_ATT_U; ++j) u[j] = u[j] > M.L[j] ? M.L[j] : u[j] < -M.L[j] ? -M.L[j] : u[j];
        }
        if (Ap) {
            double ang[3];
            attitude_angles(x, ang[0], ang[1], ang[2]);
#pragma unroll
            for (int j = 0; j < 3; ++j) Ap[i + nc * (j + (int64_t)3 * k)] = ang[j];
        }
        if constexpr (COST == HJB_ATTL_COST_QUAT) {
            double g = M.w[0] * (x[0] * x[0]);
#pragma unroll
            for (int a = 1; a < HJB_ATT_W; ++a) g = g + M.w[a] * (x[a] * x[a]);
#pragma unroll
            for (int j = 0; j < HJB_ATT_U; ++j) g = g + M.w[HJB_ATT_W + j] * (u[j] * u[j]);
            J = J + g;
        } else {
            double g[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double s = x[3 + j];
                s = s > 1.0 ? 1.0 : s < -1.0 ? -1.0 : s;
                const double t = 2.0 * canon_asin(s);
                g[j] = (M.w[j] * (x[j] * x[j]) + M.w[3 + j] * (t * t)) + M.w[6 + j] * (u[j] * u[j]);
            }
            J = J + ((g[0] + g[1]) + g[2]);
        }
        if (Up) {
#pragma unroll
            for (int j = 0; j < HJB_ATT_U; ++j) Up[i + nc * (j + (int64_t)HJB_ATT_U * k)] = u[j];
        }
        double xn[HJB_ATT_W];
        if constexpr (INTEG == HJB_ATT_TAYLOR) {
            double f[HJB_ATT_W];
            attitude_rates(M.A, x, u, f);
#pragma unroll
            for (int a = 0; a < HJB_ATT_W; ++a) xn[a] = x[a] + h * f[a];
        } else {
#define HJB_ATTL_RHS(j_, y_, r_) attitude_rates(M.A, y_, u, r_)
            HJB_ROLLOUT_RK4_STEP(HJB_ATT_W, x, xn, h, HJB_ATTL_RHS)
#undef HJB_ATTL_RHS
        }
        const double nrm = __builtin_sqrt(((xn[3] * xn[3] + xn[4] * xn[4]) + xn[5] * xn[5]) + xn[6] * xn[6]);
#pragma unroll
        for (int a = 3; a < HJB_ATT_W; ++a) xn[a] = xn[a] / nrm;
#pragma unroll
        for (int a = 0; a < HJB_ATT_W; ++a) x[a] = xn[a];
        if (Xp) {
#pragma unroll
            for (int a = 0; a < HJB_ATT_W; ++a) Xp[i + nc * (a + (int64_t)HJB_ATT_W * (k + 1))] = x[a];
        }
    }
#pragma unroll
    for (int a = 0; a < HJB_ATT_W; ++a) Xf[a + (int64_t)HJB_ATT_W * i] = x[a];
    if (cost) cost[i] = J;
}

// rollout_attitude_linear.hip instantiates the 4 kernels (integrator x cost form) and launches the one asked for
hipError_t launch_rollout_attitude_linear(int integrator, int cost_form, const DAttLinear &M, int64_t nc, hipStream_t st,
                                          const double *X0, double *Xf, double *cost, double *Xp, double *Up, double *Ap);

}  // namespace hjb
