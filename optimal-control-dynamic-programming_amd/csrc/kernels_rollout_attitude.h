// kernels_rollout_attitude.h - K17: batched closed-loop rollouts of the 6-D attitude policy (hjb_rollout_run_attitude).
//
// attitude-control/Solver_attitude.m:744-833 (get_optimal_path after run) for many initial attitudes at once: one thread per
// trajectory, all n_steps steps in one launch, everything in double, left to right, every product rounded (-ffp-contract=off).
// The state is the reference's X = [w1 w2 w3 q1 q2 q3 q4] (q4 scalar).  Per step k, p = plane_of_step[k]:
//   (yaw, pitch, roll) = quat_to_yaw_pitch_roll([X7 X6 X5 X4]) (:757) with canon_atan2 / canon_asin below, not renormalised;
//   u = K16's lookup (HJB_ROLLOUT_LOOKUP, kernels_rollout.h) at (X1, X2, X3, yaw, pitch, roll) on plane p;
//   cost += ((q1*(X1*X1) + q2*(X2*X2)) + ... + q7*(X7*X7)) + r1*(u1*u1) + r2*(u2*u2) + r3*(u3*u3);
//   X+ = X + h f(X, u) ('taylor', :688) or classical RK4 with u held (:679-686), f = spacecraft_dynamics_list (:600-620);
//   X4..X7 /= sqrt(((X4*X4 + X5*X5) + X6*X6) + X7*X7) (a division, as next_stage_states does).
// Steps 4 - 6 are operation for operation hjbdp/rollout.py::next_stage_states; the numpy restatement is
// tests/attitude_rollout_refs.py.  No RK4 temporary is live across the lookup (one lookup per step), so the 64 corner labels of
// 'linear' and the four RK4 stages never share the register file.
#pragma once
#include "hjbdp_dev.h"
#include "kernels_rollout.h"

namespace hjb {

#define HJB_ATT_W 7                   // state width
#define HJB_ATT_U 3                   // torques

struct DAttitude {
    double h;
    double J[3];                      // J1, J2, J3
    double c[3];                      // (J2-J3)/J1, (J3-J1)/J2, (J1-J2)/J3, formed once on the host
    double q[HJB_ATT_W], r[HJB_ATT_U];   // NULL on the host side = zeros
};

// ---- canonical double atan2 / asin ----------------------------------------------------------------------------------------
// fdlibm's e_atan2.c / s_atan.c / e_asin.c restated with + - * /, __builtin_sqrt, comparisons and selects only (every one
// correctly rounded on gfx950: f64 '/' is div_scale / div_fmas / div_fixup, sqrt is rsq plus refinement), so
// tests/attitude_rollout_refs.py repeats them bit for bit in numpy.  They depart from fdlibm in two places, so fdlibm's 1-ulp
// bound is not inherited: asin's low-word clear of sqrt(t) (which makes its square exact) is a Veltkamp split here (26 leading
// bits instead of 21: the square is exact either way), and asin's last branch point is the constant 0.975 instead of fdlibm's
// high-word compare.  Tested: within 2 ulp of libm over 10^6 arguments and the edge cases (tests/test_rollout_attitude_abi.py).
// The sign of a zero is read with __builtin_signbit.
__device__ __forceinline__ double canon_atan_nonneg(double x) {     // x >= 0
    int id;
    double r;
    if (x < 0.4375) {
        id = -1;
        r = x;
    } else if (x < 0.6875) {
        id = 0;
        r = (2.0 * x - 1.0) / (2.0 + x);
    } else if (x < 1.1875) {
        id = 1;
        r = (x - 1.0) / (x + 1.0);
    } else if (x < 2.4375) {
        id = 2;
        r = (x - 1.5) / (1.0 + 1.5 * x);
    } else {
        id = 3;
        r = -1.0 / x;
    }
    const double z = r * r, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
                      w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
                      w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (id < 0) return r - r * (s1 + s2);
    const double hi = id == 0 ? 4.63647609000806093515e-01 : id == 1 ? 7.85398163397448278999e-01
                    : id == 2 ? 9.82793723247329054082e-01 : 1.57079632679489655800e+00;
    const double lo = id == 0 ? 2.26987774529616870924e-17 : id == 1 ? 3.06161699786838301793e-17
                    : id == 2 ? 1.39033110312309984516e-17 : 6.12323399573676603587e-17;
    return hi - ((r * (s1 + s2) - lo) - r);
}

__device__ __forceinline__ double canon_atan2(double y, double x) {
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
    double a;
    if (ax == 0.0) {
        a = ay == 0.0 ? (__builtin_signbit(x) ? 3.1415926535897931160e+00 : 0.0) : 1.5707963267948965580e+00;
    } else {
        const double z = canon_atan_nonneg(ay / ax);
        a = __builtin_signbit(x) ? 3.1415926535897931160e+00 - (z - 1.2246467991473531772e-16) : z;
    }
    return __builtin_signbit(y) ? -a : a;
}

__device__ __forceinline__ double canon_asin(double x) {           // |x| <= 1
    const double ax = __builtin_fabs(x);
    double v;
    if (ax < 0.5) {
        const double t = ax * ax;
        const double p = t * (1.66666666666666657415e-01 + t * (-3.25565818622400915405e-01 + t * (2.01212532134862925881e-01 +
                         t * (-4.00555345006794114027e-02 + t * (7.91534994289814532176e-04 + t * 3.47933107596021167570e-05)))));
        const double q = 1.0 + t * (-2.40339491173441421878e+00 + t * (2.02094576023350569471e+00 + t * (-6.88283971605453293030e-01 +
                         t * 7.70381505559019352791e-02)));
        v = ax + ax * (p / q);
    } else {
        const double t = (1.0 - ax) * 0.5;
        const double p = t * (1.66666666666666657415e-01 + t * (-3.25565818622400915405e-01 + t * (2.01212532134862925881e-01 +
                         t * (-4.00555345006794114027e-02 + t * (7.91534994289814532176e-04 + t * 3.47933107596021167570e-05)))));
        const double q = 1.0 + t * (-2.40339491173441421878e+00 + t * (2.02094576023350569471e+00 + t * (-6.88283971605453293030e-01 +
                         t * 7.70381505559019352791e-02)));
        const double s = __builtin_sqrt(t);
        if (ax >= 0.975) {
            v = 1.57079632679489655800e+00 - (2.0 * (s + s * (p / q)) - 6.12323399573676603587e-17);
        } else {
            const double cs = s * 134217729.0;                        // 2^27 + 1: s = sh + (s - sh), sh * sh exact
            const double sh = cs - (cs - s);
            const double c = (t - sh * sh) / (s + sh);
            const double pp = 2.0 * s * (p / q) - (6.12323399573676603587e-17 - 2.0 * c);
            const double qq = 7.85398163397448278999e-01 - 2.0 * sh;
            v = 7.85398163397448278999e-01 - (pp - qq);
        }
    }
    return __builtin_signbit(x) ? -v : v;
}

// (yaw, pitch, roll) of the quaternion part of X: the mirror's quat_to_yaw_pitch_roll([X7 X6 X5 X4]) (Solver_attitude.m:757)
__device__ __forceinline__ void attitude_angles(const double (&x)[HJB_ATT_W], double &yaw, double &pitch, double &roll) {
    const double x4 = x[3], x5 = x[4], x6 = x[5], x7 = x[6];
    yaw = canon_atan2(2.0 * (x6 * x5 + x7 * x4), ((x7 * x7 + x6 * x6) - x5 * x5) - x4 * x4);
    double s = -2.0 * (x6 * x4 - x7 * x5);
    s = s > 1.0 ? 1.0 : s < -1.0 ? -1.0 : s;
    pitch = canon_asin(s);
    roll = canon_atan2(2.0 * (x5 * x4 + x7 * x6), ((x7 * x7 - x6 * x6) - x5 * x5) + x4 * x4);
}

// f(X, u): spacecraft_dynamics_list (Solver_attitude.m:600-620), diagonal inertia
__device__ __forceinline__ void attitude_rates(const DAttitude &M, const double (&x)[HJB_ATT_W], const double (&u)[HJB_ATT_U],
                                               double (&f)[HJB_ATT_W]) {
    f[0] = ((M.c[0] * x[1]) * x[2]) + u[0] / M.J[0];
    f[1] = ((M.c[1] * x[2]) * x[0]) + u[1] / M.J[1];
    f[2] = ((M.c[2] * x[0]) * x[1]) + u[2] / M.J[2];
    f[3] = 0.5 * (((x[2] * x[4]) - (x[1] * x[5])) + (x[0] * x[6]));
    f[4] = 0.5 * (((-x[2] * x[3]) + (x[0] * x[5])) + (x[1] * x[6]));
    f[5] = 0.5 * (((x[1] * x[3]) - (x[0] * x[4])) + (x[2] * x[6]));
    f[6] = 0.5 * (((-x[0] * x[3]) - (x[1] * x[4])) - (x[2] * x[5]));
}

template <typename TL, int METHOD, bool LDS, int INTEG>
__global__ void __launch_bounds__(256)
k_rollout_attitude(const DRollout R, const DAttitude M, int64_t nc, const double *__restrict__ X0, double *__restrict__ Xf,
                   double *__restrict__ cost, double *__restrict__ Xp, double *__restrict__ Up, double *__restrict__ Ap) {
    extern __shared__ double smem[];
    const double *kn, *rd, *ut;
    HJB_ROLLOUT_PLACE(p, R, HJB_ATT_U, smem)
    HJB_ROLLOUT_STAGE(LDS, p, R, kn, rd, ut)
    if constexpr (LDS) __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const TL *__restrict__ lab = static_cast<const TL *>(R.labels);
    const int64_t nl = R.n_labels;
    const double h = M.h;
    double x[HJB_ATT_W];
#pragma unroll
    for (int a = 0; a < HJB_ATT_W; ++a) x[a] = X0[a + (int64_t)HJB_ATT_W * i];
    if (Xp) {
#pragma unroll
        for (int a = 0; a < HJB_ATT_W; ++a) Xp[i + nc * a] = x[a];
    }
    double J = 0.0;
    for (int k = 0; k < R.n_steps; ++k) {
        double p[6];
        p[0] = x[0];
        p[1] = x[1];
        p[2] = x[2];
        attitude_angles(x, p[3], p[4], p[5]);
        if (Ap) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Ap[i + nc * (j + (int64_t)3 * k)] = p[3 + j];
        }
        HJB_ROLLOUT_LOOKUP(6, HJB_ATT_U, METHOD, R, kn, rd, ut, lab, k, p, HJB_ATT_U, nl, u)
        double g = M.q[0] * (x[0] * x[0]);
#pragma unroll
        for (int a = 1; a < HJB_ATT_W; ++a) g = g + M.q[a] * (x[a] * x[a]);
#pragma unroll
        for (int j = 0; j < HJB_ATT_U; ++j) g = g + M.r[j] * (u[j] * u[j]);
        J = J + g;
        double xn[HJB_ATT_W];
        if constexpr (INTEG == HJB_ATT_TAYLOR) {
            double f[HJB_ATT_W];
            attitude_rates(M, x, u, f);
#pragma unroll
            for (int a = 0; a < HJB_ATT_W; ++a) xn[a] = x[a] + h * f[a];
        } else {
#define HJB_ATT_RHS(j_, y_, r_) attitude_rates(M, y_, u, r_)
            HJB_ROLLOUT_RK4_STEP(HJB_ATT_W, x, xn, h, HJB_ATT_RHS)
#undef HJB_ATT_RHS
        }
        const double nrm = __builtin_sqrt(((xn[3] * xn[3] + xn[4] * xn[4]) + xn[5] * xn[5]) + xn[6] * xn[6]);
#pragma unroll
        for (int a = 3; a < HJB_ATT_W; ++a) xn[a] = xn[a] / nrm;
        if (Up) {
#pragma unroll
            for (int j = 0; j < HJB_ATT_U; ++j) Up[i + nc * (j + (int64_t)HJB_ATT_U * k)] = u[j];
        }
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

// rollout_attitude.hip instantiates the 24 kernels (label type x method x LDS x integrator) and launches the one asked for
hipError_t launch_rollout_attitude(int idx_bytes, int method, bool lds_on, int integrator, const DRollout &R, const DAttitude &M,
                                   int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf, double *cost, double *Xp,
                                   double *Up, double *Ap);

}  // namespace hjb
