// hjbdp_greedy.h - one step of the greedy rollout (K26, kernels_rollout_greedy.h): one-step lookahead on a stored cost-to-go,
//   u_k(x) = argmin_u  g(x, u) + J_{k+1}(f(x, u))   at the state actually visited,
// over the affine model of K16 (x+ = A x + B u + c, g = x'diag(q)x + u'diag(r)u) and a finite control table.  Written once for
// the kernel and for its host twin hjb_rollout_greedy_host (rollout.hip).  No HIP dependency: tests/greedy_harness.cpp compiles
// it as plain C++.  The contract (stated verbatim in include/hjbdp.h), everything in double, every product rounded:
//   state parts  gs = (q0*(x0*x0) + q1*(x1*x1)) + ...;  as_a = (A[a,0]*x0 + A[a,1]*x1) + ...          (once per step)
//   candidate l  u_j = u_table[l, j];  g_l = gs + r0*(u0*u0) + ...;  xn_a = as_a + B[a,0]*u0 + ... (+ c_a)      (K16's g and x+)
//                v_l = the N-linear blend of the value plane at xn: cell = clamp(upper_bound(knots, xn_a) - 1, 0, n - 2) (outside
//                the grid the blend extrapolates; NaN: cell 0), t_a = (xn_a - k[cell]) * rdx[cell], fma lerps axis 0 first,
//                pairwise - hjb_policy_lookup's 'linear' in double on that plane, bit for bit; no plane: v_l = +0.0, nothing read
//                cand_l = g_l + v_l
//   choice       best = cand_0; label l >= 1 replaces iff cand_l < best: the first minimum wins, a NaN candidate never replaces
//   apply        u, g and x+ of the chosen label, formed again by the operations above on the same operands: the same bits.
// The lerp tree is evaluated depth-first as in HJB_ROLLOUT_LOOKUP (kernels_rollout.h): corner c is a leaf, after it the tree nodes
// it completes (one per trailing 1-bit of c) fold into a stack of D + 1 partials - never 2^D values live.
// MODEL is any record with K16's members (DRollout on the device, GreedyModel here): n_u, n_labels, has_c, n, koff, uniform, x0,
// inv_h, stride, A, B, c, q, r.
#pragma once
#include <stdint.h>
#include "../../include/hjbdp.h"

#if defined(__HIPCC__)
#include "hjbdp_dev.h"
#define HJB_GREEDY_FN __host__ __device__ __forceinline__
#else
#define HJB_GREEDY_FN inline
#endif
// every product rounded, whatever the including unit's default: only the explicit fmas contract
#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace hjb {

// K16's model and grid description without the device pointers (the members DRollout has, under the same names)
struct GreedyModel {
    int32_t n_u, n_labels, has_c, n_knots;
    int32_t n[HJB_MAX_D];
    int32_t koff[HJB_MAX_D];
    int32_t uniform[HJB_MAX_D];
    double x0[HJB_MAX_D], inv_h[HJB_MAX_D];
    int64_t stride[HJB_MAX_D];
    int64_t nS;
    double A[HJB_MAX_D * HJB_MAX_D];
    double B[HJB_MAX_D * HJB_ROLLOUT_MAX_U];
    double c[HJB_MAX_D], q[HJB_MAX_D], r[HJB_ROLLOUT_MAX_U];
};

// The grid half of a MODEL and 1/dx, the one place they are formed (hjb_rollout_create calls it on its DRollout): rdx[i] =
// 1 / (k[i+1] - k[i]) (0 at an axis' last knot), the arithmetic first guess of the cell search on axes whose knots are uniform
// to 1.5 steps.  knots: the axes' vectors concatenated; rdx: as many doubles.
template <typename MODEL>
inline void greedy_grid(int D, const int32_t *n, const double *knots, MODEL &M, double *rdx) {
    int64_t s = 1;
    int32_t off = 0;
    for (int a = 0; a < D; ++a) {
        const double *k = knots + off;
        for (int i = 0; i < n[a]; ++i) rdx[off + i] = i + 1 < n[a] ? 1.0 / (k[i + 1] - k[i]) : 0.0;
        const double hstep = (k[n[a] - 1] - k[0]) / (n[a] - 1);
        double dev = 0;
        for (int i = 0; i < n[a]; ++i) {
            const double d = k[i] - (k[0] + i * hstep);
            dev = dev > (d < 0 ? -d : d) ? dev : (d < 0 ? -d : d);
        }
        M.uniform[a] = dev <= 1.5 * hstep ? 1 : 0;
        M.x0[a] = k[0];
        M.inv_h[a] = 1.0 / hstep;
        M.n[a] = n[a];
        M.koff[a] = off;
        M.stride[a] = s;
        s *= n[a];
        off += n[a];
    }
    M.n_knots = off;
    M.nS = s;
}

// clamp(upper_bound(k, q) - 1, 0, n - 2), exact for any strictly increasing knots: find_cell of kernels_generic.h for host and
// device (the first guess of a uniform axis is corrected by the two walks, so both branches end at the same cell)
HJB_GREEDY_FN int greedy_cell(const double *k, int n, double q, int uniform, double x0, double inv_h) {
    int i;
    if (uniform) {
        double f = (q - x0) * inv_h;
        const double hi = (double)(n - 2);
        f = f > 0.0 ? f : 0.0;
        f = f < hi ? f : hi;
        i = (int)f;
        while (i > 0 && q < k[i]) --i;
        while (i < n - 2 && q >= k[i + 1]) ++i;
    } else {
        int lo = 0, hi = n - 1;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (k[mid] <= q) lo = mid; else hi = mid;
        }
        i = lo;
    }
    return i;
}

// The record M read again where it lies (record_reread, hjbdp_dev.h): on the device the model is read through the kernel's argument
// segment with scalar loads (kernels_rollout_greedy.h), and the reads of a loop body are issued in the body.  As plain C++ (the
// harnesses) there is no such segment and nothing to reread.
#if !defined(__HIPCC__)
template <typename T>
inline const T &record_reread(const T &r) { return r; }
#endif

// ... inside the candidate loop, where it is needed: from D = 3 on.  Below that the loop's scalars fit and stay in registers.
template <int D, typename MODEL>
HJB_GREEDY_FN const MODEL &greedy_reread_in_loop(const MODEL &M) {
    if constexpr (D >= 3) return record_reread(M);
    else return M;
}

HJB_GREEDY_FN constexpr int greedy_trailing_ones(int c) { return (c & 1) ? 1 + greedy_trailing_ones(c >> 1) : 0; }

// the state parts of a step: gs and as[D], K16's sums up to the point where the control enters
template <int D, typename MODEL>
HJB_GREEDY_FN void greedy_state_parts(const MODEL &M, const double (&x)[D], double &gs, double (&as)[D]) {
    double g = M.q[0] * (x[0] * x[0]);
#pragma unroll
    for (int a = 1; a < D; ++a) g = g + M.q[a] * (x[a] * x[a]);
    gs = g;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        double acc = M.A[a] * x[0];
#pragma unroll
        for (int b = 1; b < D; ++b) acc = acc + M.A[a + D * b] * x[b];
        as[a] = acc;
    }
}

// label l's control, stage cost (returned) and next state from the state parts; NU = n_u, u[NU ..] = 0
template <int D, int NU, typename MODEL>
HJB_GREEDY_FN double greedy_control(const MODEL &M0, const double *ut, int l, double gs, const double (&as)[D],
                                    double (&u)[HJB_ROLLOUT_MAX_U], double (&xn)[D]) {
    const int64_t nl = M0.n_labels;
#pragma unroll
    for (int j = 0; j < HJB_ROLLOUT_MAX_U; ++j) u[j] = j < NU ? ut[l + nl * j] : 0.0;
    double g = gs;
#pragma unroll
    for (int j = 0; j < NU; ++j) g = g + M0.r[j] * (u[j] * u[j]);
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const MODEL &M = greedy_reread_in_loop<D>(M0);
        double acc = as[a];
#pragma unroll
        for (int j = 0; j < NU; ++j) acc = acc + M.B[a + D * j] * u[j];
        if (M.has_c) acc = acc + M.c[a];
        xn[a] = acc;
    }
    return g;
}

// The N-linear blend of `plane` (nS values of TV, read as doubles) at xn.  The corners are read GRP at a time, every read of a
// group issued before its first value is folded: all 2^D for D <= 4, 16 beyond (D = 6 with 64 reads in flight would hold 128
// registers of values; four groups of 16 hold 32).
template <int D, typename TV, typename MODEL>
HJB_GREEDY_FN double greedy_value(const MODEL &M0, const double *kn, const double *rd, const TV *plane, const double (&xn)[D]) {
    int64_t base = 0;
    double tw[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const MODEL &M = greedy_reread_in_loop<D>(M0);
        const double *kk = kn + M.koff[a];
        const int cell = greedy_cell(kk, M.n[a], xn[a], M.uniform[a], M.x0[a], M.inv_h[a]);
        tw[a] = (double)((double)(xn[a] - kk[cell]) * rd[M.koff[a] + cell]);
        base += M.stride[a] * cell;
    }
    constexpr int GRP = (1 << D) < 16 ? (1 << D) : 16;
    double s[D + 1];
#pragma unroll
    for (int c0 = 0; c0 < (1 << D); c0 += GRP) {
        const MODEL &M = greedy_reread_in_loop<D>(M0);
        double leaf[GRP];
#pragma unroll
        for (int e = 0; e < GRP; ++e) {
            int64_t off = base;
#pragma unroll
            for (int a = 0; a < D; ++a)
                if ((c0 + e) & (1 << a)) off += M.stride[a];
            leaf[e] = (double)plane[off];
        }
#pragma unroll
        for (int e = 0; e < GRP; ++e) {
            double v = leaf[e];
            const int t1 = greedy_trailing_ones(c0 + e);
#pragma unroll
            for (int a = 0; a < D; ++a)
                if (a < t1) v = __builtin_fma(tw[a], (double)(v - s[a]), s[a]);
            s[t1] = v;
        }
    }
    return s[D];
}

// greedy_step at n_u = NU
template <int D, int NU, typename TV, typename MODEL>
HJB_GREEDY_FN void greedy_step_nu(const MODEL &M0, const double *kn, const double *rd, const double *ut, const TV *plane,
                                  double (&x)[D], double (&u)[HJB_ROLLOUT_MAX_U], double &g, int &label, double &best) {
    double gs, as[D];
    greedy_state_parts<D>(record_reread(M0), x, gs, as);
    double bst = 0.0;
    int lb = 0;
    const int nl = M0.n_labels;
    for (int l = 0; l < nl; ++l) {
        double ul[HJB_ROLLOUT_MAX_U], xn[D];
        const double gl = greedy_control<D, NU>(greedy_reread_in_loop<D>(M0), ut, l, gs, as, ul, xn);
        const double v = plane ? greedy_value<D, TV>(greedy_reread_in_loop<D>(M0), kn, rd, plane, xn) : 0.0;
        const double cand = gl + v;
        if (l == 0 || cand < bst) {
            bst = cand;
            lb = l;
        }
    }
    double xn[D];
    g = greedy_control<D, NU>(record_reread(M0), ut, lb, gs, as, u, xn);
#pragma unroll
    for (int a = 0; a < D; ++a) x[a] = xn[a];
    label = lb;
    best = bst;
}

// One step at x: the first minimum over the labels 0 .. n_labels - 1 of g_l + v_l, then the chosen label applied.  plane: the
// value plane of the step, or null for the zero function.  On return x is the next state, u the chosen control (u[n_u ..] = 0),
// g its stage cost, label the chosen label (0-based), best the minimum - the cost-to-go the controller believed.
// The candidate loop is compiled once per n_u (1 .. HJB_ROLLOUT_MAX_U) and picked by a uniform branch: written over
// HJB_ROLLOUT_MAX_U controls with the unused ones masked, as K16 writes its one evaluation per step, every candidate of a
// one-control problem would pay four controls' products.
template <int D, typename TV, typename MODEL>
HJB_GREEDY_FN void greedy_step(const MODEL &M, const double *kn, const double *rd, const double *ut, const TV *plane, double (&x)[D],
                               double (&u)[HJB_ROLLOUT_MAX_U], double &g, int &label, double &best) {
    static_assert(HJB_ROLLOUT_MAX_U == 4, "one case per n_u below");
    switch (M.n_u) {
        case 1: greedy_step_nu<D, 1, TV>(M, kn, rd, ut, plane, x, u, g, label, best); break;
        case 2: greedy_step_nu<D, 2, TV>(M, kn, rd, ut, plane, x, u, g, label, best); break;
        case 3: greedy_step_nu<D, 3, TV>(M, kn, rd, ut, plane, x, u, g, label, best); break;
        default: greedy_step_nu<D, 4, TV>(M, kn, rd, ut, plane, x, u, g, label, best); break;
    }
}

// The host twin's loop: n_traj trajectories, n_steps steps each, with the functions above and nothing else.  values: [nS,
// n_planes] of TV, column-major; plane_of_step[k] = -1: the zero function.  Paths laid out as the kernel's, trajectory index
// fastest; any of cost and the four paths may be null.  L_path holds the 0-based label.
template <int D, typename TV>
inline void greedy_rollout_host(const GreedyModel &M, const double *knots, const double *rdx, const double *u_table, const TV *values,
                                int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj, const double *X0, double *X_final,
                                double *cost, double *X_path, double *U_path, double *L_path, double *V_path) {
    const int nu = M.n_u;
    for (int64_t i = 0; i < n_traj; ++i) {
        double x[D];
        for (int a = 0; a < D; ++a) x[a] = X0[a + (int64_t)D * i];
        if (X_path)
            for (int a = 0; a < D; ++a) X_path[i + n_traj * a] = x[a];
        double J = 0.0;
        for (int k = 0; k < n_steps; ++k) {
            const int32_t p = plane_of_step[k];
            const TV *plane = p < 0 ? nullptr : values + (int64_t)p * M.nS;
            double u[HJB_ROLLOUT_MAX_U], g, best;
            int label;
            greedy_step<D, TV>(M, knots, rdx, u_table, plane, x, u, g, label, best);
            J = J + g;
            if (U_path)
                for (int j = 0; j < nu; ++j) U_path[i + n_traj * (j + (int64_t)nu * k)] = u[j];
            if (L_path) L_path[i + n_traj * k] = (double)label;
            if (V_path) V_path[i + n_traj * k] = best;
            if (X_path)
                for (int a = 0; a < D; ++a) X_path[i + n_traj * (a + (int64_t)D * (k + 1))] = x[a];
        }
        for (int a = 0; a < D; ++a) X_final[a + (int64_t)D * i] = x[a];
        if (cost) cost[i] = J;
    }
}

}  // namespace hjb
