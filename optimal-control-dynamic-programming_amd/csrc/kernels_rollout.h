// kernels_rollout.h - K16: batched fixed-step closed-loop rollouts of a stored per-stage policy (hjb_rollout_*).
//
// One thread per trajectory; all n_steps steps run inside one launch (trajectories are independent).  Per step k:
//   p = plane_of_step[k]; locate the cell on every axis (find_cell, exact); read the label(s) of plane p;
//   u_j = u_table[L - index_base, j] at the nearer knot ('nearest': upper one at the midpoint, k_policy_lookup's rule)
//         or the N-linear interpolation of u_table[label, j] over the 2^D corners ('linear': k_policy_lookup's arithmetic,
//         fma lerps axis 0 first, pairwise);
//   g = ((q0*(x0*x0) + q1*(x1*x1)) + ...) + r0*(u0*u0) + ...;  cost += g;
//   x+_a = ((A[a,0]*x0 + A[a,1]*x1) + ...) + B[a,0]*u0 + ... + c_a   (every product rounded: -ffp-contract=off).
// Everything is double.  The pairwise lerp tree is evaluated DEPTH-FIRST: corner c is a leaf, and after it the tree nodes it
// completes (one per trailing 1-bit of c) are folded into a stack of D + 1 partials - the same operations on the same operands
// as the breadth-first loop of k_policy_lookup, so the result is bit-identical to hjb_policy_lookup on the dense values
// u_table[labels[:, p] - base, j], without 2^D x n_u doubles live (D = 6: 64 labels + 7 partials).
// Knots, 1/dx and u_table are staged in LDS when they fit (LDS = true; hjb_rollout_run decides), else read from global memory.
// Labels stay in global memory (nS x n_planes: one plane of a reference-sized grid is L2-resident).  Labels were range-checked by
// hjb_rollout_create, so no read leaves u_table.  Offsets are int64 throughout; stores are plain, trajectory index fastest.
#pragma once
#include "hjbdp_dev.h"
#include "hjbdp_canon.h"

namespace hjb {

struct DRollout {
    int32_t n_u, n_labels, index_base, n_steps;
    int32_t n_knots;                  // sum of n[a]: knots / rdx are concatenated, axis a at koff[a]
    int32_t has_c;
    int32_t n[HJB_MAX_D];
    int32_t koff[HJB_MAX_D];
    int32_t uniform[HJB_MAX_D];       // find_cell's arithmetic first guess (exact either way)
    double x0[HJB_MAX_D], inv_h[HJB_MAX_D];
    int64_t stride[HJB_MAX_D];        // state strides, axis 0 fastest
    int64_t nS;                       // states per plane of the label array
    const double *knots, *rdx;        // [n_knots] each (global)
    const double *u_table;            // [n_labels, n_u] column-major (global)
    const void *labels;               // [nS, n_planes] column-major, TL
    const int32_t *plane_of_step;     // [n_steps]
    double A[HJB_MAX_D * HJB_MAX_D];  // [D, D] column-major
    double B[HJB_MAX_D * HJB_ROLLOUT_MAX_U];   // [D, n_u] column-major
    double c[HJB_MAX_D], q[HJB_MAX_D], r[HJB_ROLLOUT_MAX_U];   // NULL on the host side = zeros (q, r) / no addition (c)
};

// number of trailing 1-bits of c: the tree nodes corner c completes
__device__ __forceinline__ constexpr int trailing_ones(int c) { return (c & 1) ? 1 + trailing_ones(c >> 1) : 0; }

// One step's policy lookup, the ONE definition K16 and K17 (kernels_rollout_attitude.h) share: declares u_[NU_] = the controls at
// x_ on plane plane_of_step[k_] (u_[nu_ .. NU_) = 0).  kn_ / rd_ / ut_: knots, 1/dx and u_table (LDS or global); nl_ = R_.n_labels.
// A macro, not a __device__ function: routed through a function (force-inlined, R by reference or by value) the compiler schedules
// K16 differently and its pos-att case ran 6 % slower; expanded in place, K16's code object is byte for byte the one it was.
// Names it declares in the caller's scope: `base` (int64_t), `tw` (double[D_]) and the output array named by u_; its loop
// variables (a, j, c) and the temporaries kk, cell, L, off, s, v, t1 live inside its own blocks.  It reads the caller's
// find_cell, fma_t and trailing_ones.  One expansion per scope (a step-loop body).
#define HJB_ROLLOUT_LOOKUP(D_, NU_, METHOD_, R_, kn_, rd_, ut_, lab_, k_, x_, nu_, nl_, u_)                                          \
    int64_t base = (int64_t)R_.plane_of_step[k_] * R_.nS;                                                                       \
    double tw[D_];                                                                                                              \
    _Pragma("unroll") for (int a = 0; a < D_; ++a) {                                                                            \
        const double *kk = kn_ + R_.koff[a];                                                                                    \
        int cell = find_cell<double>(kk, R_.n[a], x_[a], R_.uniform[a], R_.x0[a], R_.inv_h[a]);                                 \
        if (METHOD_ == HJB_LOOKUP_NEAREST) {                                                                                    \
            if ((double)(x_[a] - kk[cell]) >= (double)(kk[cell + 1] - x_[a])) ++cell;                                           \
            tw[a] = 0.0;                                                                                                        \
        } else {                                                                                                                \
            tw[a] = (double)((double)(x_[a] - kk[cell]) * rd_[R_.koff[a] + cell]);                                              \
        }                                                                                                                       \
        base += R_.stride[a] * cell;                                                                                            \
    }                                                                                                                           \
    double u_[NU_];                                                                                                             \
    if (METHOD_ == HJB_LOOKUP_NEAREST) {                                                                                        \
        const int64_t L = (int64_t)lab_[base] - R_.index_base;                                                                  \
        _Pragma("unroll") for (int j = 0; j < NU_; ++j) {                                                                       \
            u_[j] = 0.0;                                                                                                        \
            if (j < nu_) u_[j] = ut_[L + nl_ * j];                                                                              \
        }                                                                                                                       \
    } else {                                                                                                                    \
        int32_t L[1 << D_];                                                                                                     \
        _Pragma("unroll") for (int c = 0; c < (1 << D_); ++c) { /* every corner label in flight before the first is used */  \
            int64_t off = base;                                                                                                 \
            _Pragma("unroll") for (int a = 0; a < D_; ++a) if (c & (1 << a)) off += R_.stride[a];                               \
            L[c] = (int32_t)lab_[off];                                                                                          \
        }                                                                                                                       \
        _Pragma("unroll") for (int c = 0; c < (1 << D_); ++c) L[c] -= R_.index_base;                                            \
        _Pragma("unroll") for (int j = 0; j < NU_; ++j) {                                                                       \
            u_[j] = 0.0;                                                                                                        \
            if (j < nu_) {                                                                                                      \
                double s[D_ + 1];                                                                                               \
                _Pragma("unroll") for (int c = 0; c < (1 << D_); ++c) {                                                         \
                    double v = ut_[L[c] + nl_ * j];                                                                             \
                    const int t1 = trailing_ones(c);                                                                            \
                    _Pragma("unroll") for (int a = 0; a < D_; ++a) if (a < t1) v = fma_t<double>(tw[a], (double)(v - s[a]), s[a]); \
                    s[t1] = v;                                                                                                  \
                }                                                                                                               \
                u_[j] = s[D_];                                                                                                  \
            }                                                                                                                   \
        }                                                                                                                       \
    }

// One step's stage cost and affine update, the ONE statement K16, K25 (kernels_rollout_noisy.h) and K28
// (kernels_rollout_campaign.h) expand: declares g_ = ((q0*(x0*x0) + q1*(x1*x1)) + ...) + r0*(u0*u0) + ... and xn_[D_], xn_a =
// ((A[a,0]*x0 + A[a,1]*x1) + ...) + B[a,0]*u0 + ... (+ c_a), every product rounded, in this order: what the bit-exact contracts of
// the three kernels and of hjbdp_greedy.h's two halves (greedy_state_parts, greedy_control) rest on.  Rg_ and Ra_ are EXPRESSIONS
// for the record (a DRollout): Rg_ is evaluated once, for the cost; Ra_ once per row of A and B, inside the row loop - K28 passes
// a reread of its launch record for each (campaign_reread_in_step), K16 and K25 their argument.  A macro for HJB_ROLLOUT_LOOKUP's
// reason; its records are aff_g_ and aff_r_, its loop variables (a, b, j) and acc live inside its own blocks.
#define HJB_ROLLOUT_AFFINE_STEP(D_, NU_, Rg_, Ra_, x_, u_, nu_, g_, xn_)                                                        \
    double g_;                                                                                                                  \
    {                                                                                                                           \
        const auto &aff_g_ = Rg_;                                                                                               \
        g_ = aff_g_.q[0] * (x_[0] * x_[0]);                                                                                     \
        _Pragma("unroll") for (int a = 1; a < D_; ++a) g_ = g_ + aff_g_.q[a] * (x_[a] * x_[a]);                                 \
        _Pragma("unroll") for (int j = 0; j < NU_; ++j) if (j < nu_) g_ = g_ + aff_g_.r[j] * (u_[j] * u_[j]);                   \
    }                                                                                                                           \
    double xn_[D_];                                                                                                             \
    _Pragma("unroll") for (int a = 0; a < D_; ++a) {                                                                            \
        const auto &aff_r_ = Ra_;                                                                                               \
        double acc = aff_r_.A[a] * x_[0];                                                                                       \
        _Pragma("unroll") for (int b = 1; b < D_; ++b) acc = acc + aff_r_.A[a + D_ * b] * x_[b];                                \
        _Pragma("unroll") for (int j = 0; j < NU_; ++j) if (j < nu_) acc = acc + aff_r_.B[a + D_ * j] * u_[j];                  \
        if (aff_r_.has_c) acc = acc + aff_r_.c[a];                                                                              \
        xn_[a] = acc;                                                                                                           \
    }

// One channel's tables for the lookup, the ONE staging every rollout kernel uses, in two steps (t_: a name for the channel; c_: a
// DRollout or a DPaChan; width_: u_table doubles per label).
//   HJB_ROLLOUT_PLACE: the channel's place in LDS, [knots | 1/dx | u_table] from at_ on; HJB_ROLLOUT_PLACE_END(t_) is where the
//     next channel goes.
//   HJB_ROLLOUT_STAGE: LDS_: the block copies the channel to its place and kn_ / rd_ / ut_ point into the copy (the caller issues
//     ONE __syncthreads() after its last channel); otherwise kn_ / rd_ / ut_ are the channel's global pointers.
// Every PLACE of a kernel comes before its first STAGE, and the end of a place is an expression, not a variable: with a channel's
// counts read between two copy loops, or with the end held in a pointer of its own, the compiler allocates the registers of the
// LDS kernels differently.  Macros for HJB_ROLLOUT_LOOKUP's reason: behind a force-inlined function K16's registers move too.
// Names: PLACE declares nk_<t_>, nu_<t_> and lds_<t_> in the CALLER's scope, in the global-memory form of a kernel too (where
// only the discarded branch of STAGE reads them and they cost nothing): leave them there, moving them into the branch is the
// change of order described above.  STAGE's loop variable is stage_e_, inside its own blocks.
#define HJB_ROLLOUT_PLACE(t_, c_, width_, at_)                                                                                 \
    const int nk_##t_ = c_.n_knots, nu_##t_ = c_.n_labels * width_;                                                            \
    double *lds_##t_ = at_;
#define HJB_ROLLOUT_PLACE_END(t_) (lds_##t_ + 2 * nk_##t_ + nu_##t_)
#define HJB_ROLLOUT_STAGE(LDS_, t_, c_, kn_, rd_, ut_)                                                                         \
    if constexpr (LDS_) {                                                                                                      \
        for (int stage_e_ = threadIdx.x; stage_e_ < nk_##t_; stage_e_ += blockDim.x) {                                         \
            lds_##t_[stage_e_] = c_.knots[stage_e_];                                                                           \
            lds_##t_[nk_##t_ + stage_e_] = c_.rdx[stage_e_];                                                                   \
        }                                                                                                                      \
        for (int stage_e_ = threadIdx.x; stage_e_ < nu_##t_; stage_e_ += blockDim.x)                                           \
            lds_##t_[2 * nk_##t_ + stage_e_] = c_.u_table[stage_e_];                                                           \
        kn_ = lds_##t_;                                                                                                        \
        rd_ = lds_##t_ + nk_##t_;                                                                                              \
        ut_ = lds_##t_ + 2 * nk_##t_;                                                                                          \
    } else {                                                                                                                   \
        kn_ = c_.knots;                                                                                                        \
        rd_ = c_.rdx;                                                                                                          \
        ut_ = c_.u_table;                                                                                                      \
    }

// One classical RK4 step of hs_ from x_ into xo_ (W_ doubles each; xo_ may be x_ itself), the ONE definition the rollout kernels
// share.  RHS_(j, y, r) is a macro of the caller's that writes the right-hand side at the state y into r; j = 0..3 is the
// evaluation (k1..k4), for a right-hand side that reads a table node per evaluation (K18).  One fixed operation order:
// (r*hs)/2.0, acc + 2.0*r, (hs*(acc+r))/6.0.  A macro: as a force-inlined function taking a lambda the same operations come out
// with the operands of some commutative instructions swapped - equal results, but not the code objects that were measured.
// Its locals are rk_r_, rk_acc_, rk_xt_ and the loop variable rk_a_, inside its own block: no name of the caller's (x_, hs_, what
// RHS_ reads) may be one of these four.
#define HJB_ROLLOUT_RK4_STEP(W_, x_, xo_, hs_, RHS_)                                                                           \
    {                                                                                                                          \
        double rk_r_[W_], rk_acc_[W_], rk_xt_[W_];                                                                             \
        RHS_(0, x_, rk_r_);                                       /* k1 */                                                     \
        _Pragma("unroll") for (int rk_a_ = 0; rk_a_ < W_; ++rk_a_) {                                                           \
            rk_acc_[rk_a_] = rk_r_[rk_a_];                                                                                     \
            rk_xt_[rk_a_] = x_[rk_a_] + (rk_r_[rk_a_] * hs_) / 2.0;                                                            \
        }                                                                                                                      \
        RHS_(1, rk_xt_, rk_r_);                                   /* k2 */                                                     \
        _Pragma("unroll") for (int rk_a_ = 0; rk_a_ < W_; ++rk_a_) {                                                           \
            rk_acc_[rk_a_] = rk_acc_[rk_a_] + 2.0 * rk_r_[rk_a_];                                                              \
            rk_xt_[rk_a_] = x_[rk_a_] + (rk_r_[rk_a_] * hs_) / 2.0;                                                            \
        }                                                                                                                      \
        RHS_(2, rk_xt_, rk_r_);                                   /* k3 */                                                     \
        _Pragma("unroll") for (int rk_a_ = 0; rk_a_ < W_; ++rk_a_) {                                                           \
            rk_acc_[rk_a_] = rk_acc_[rk_a_] + 2.0 * rk_r_[rk_a_];                                                              \
            rk_xt_[rk_a_] = x_[rk_a_] + rk_r_[rk_a_] * hs_;                                                                    \
        }                                                                                                                      \
        RHS_(3, rk_xt_, rk_r_);                                   /* k4 */                                                     \
        _Pragma("unroll") for (int rk_a_ = 0; rk_a_ < W_; ++rk_a_)                                                             \
            xo_[rk_a_] = x_[rk_a_] + (hs_ * (rk_acc_[rk_a_] + rk_r_[rk_a_])) / 6.0;                                            \
    }

template <int D, typename TL, int METHOD, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout(const DRollout R, int64_t nc, const double *__restrict__ X0, double *__restrict__ Xf, double *__restrict__ cost,
          double *__restrict__ Xp, double *__restrict__ Up) {
    extern __shared__ double smem[];
    const double *kn, *rd, *ut;
    HJB_ROLLOUT_PLACE(p, R, R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, R, kn, rd, ut)
    if constexpr (LDS) __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const TL *__restrict__ lab = static_cast<const TL *>(R.labels);
    const int nu = R.n_u;
    const int64_t nl = R.n_labels;
    double x[D];
#pragma unroll
    for (int a = 0; a < D; ++a) x[a] = X0[a + (int64_t)D * i];
    if (Xp) {
#pragma unroll
        for (int a = 0; a < D; ++a) Xp[i + nc * a] = x[a];
    }
    double J = 0.0;
    for (int k = 0; k < R.n_steps; ++k) {
        HJB_ROLLOUT_LOOKUP(D, HJB_ROLLOUT_MAX_U, METHOD, R, kn, rd, ut, lab, k, x, nu, nl, u)
        HJB_ROLLOUT_AFFINE_STEP(D, HJB_ROLLOUT_MAX_U, R, R, x, u, nu, g, xn)
        J = J + g;
        if (Up) {
#pragma unroll
            for (int j = 0; j < HJB_ROLLOUT_MAX_U; ++j)
                if (j < nu) Up[i + nc * (j + (int64_t)nu * k)] = u[j];
        }
#pragma unroll
        for (int a = 0; a < D; ++a) x[a] = xn[a];
        if (Xp) {
#pragma unroll
            for (int a = 0; a < D; ++a) Xp[i + nc * (a + (int64_t)D * (k + 1))] = x[a];
        }
    }
#pragma unroll
    for (int a = 0; a < D; ++a) Xf[a + (int64_t)D * i] = x[a];
    if (cost) cost[i] = J;
}

// rollout_affine.hip instantiates the 72 kernels (label type x method x LDS x D) and launches the one asked for
hipError_t launch_rollout(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, int64_t nc, size_t lds, hipStream_t st,
                          const double *X0, double *Xf, double *cost, double *Xp, double *Up);

}  // namespace hjb
