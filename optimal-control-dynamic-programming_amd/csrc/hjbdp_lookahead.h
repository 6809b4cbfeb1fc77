// hjbdp_lookahead.h - one step of the disturbance-aware greedy rollout (K27, kernels_rollout_lookahead.h): K26's one-step lookahead
// (hjbdp_greedy.h) with the disturbed backup's E_w / max_w (K24, hjb_set_disturbance) inside every candidate,
//   u_k(x) = argmin_u  g(x, u) + E_w[ J_{k+1}(f(x, u) + e_w) ]      (HJB_DIST_EXPECT; HJB_DIST_WORST: max_w)
// at the state actually visited, and optionally K25's sampled plant noise (hjbdp_noise.h) after the chosen step.  Written once for
// the kernel and its host twin hjb_rollout_lookahead_host (rollout.hip).  No HIP dependency: tests/lookahead_harness.cpp compiles
// it as plain C++.  The contract (stated verbatim in include/hjbdp.h), everything in double, every product rounded:
//   state parts, candidate l's u, g_l and xn_a: greedy_state_parts and greedy_control of hjbdp_greedy.h, called, not restated;
//   axes outside the lookahead mask (the axes with a lookahead offset that is not +-0): cell and t_a of xn_a once per candidate,
//                shared by the nodes; such an axis is not touched by + 0.0 (K24's rule);
//   node w       in order: q_aw = xn_a + e[a][w] on the masked axes, its cell (greedy_cell) and t = (q - k[c]) * rdx[c];
//                v_w = the N-linear blend, K26's depth-first fma tree in K26's corner groups (look_blend: greedy_value's second half
//                on a located point - the same operations on the same operands);
//   combine      EXPECT: acc = p_0 * v_0 rounded, then acc = fma(p_w, v_w, acc);  WORST: acc = v_0, then acc = v_w > acc ? v_w : acc
//                (the first maximum wins, a NaN never replaces);  no plane: acc = +0.0, nothing read;  cand_l = g_l + acc;
//   choice       K26's: best = cand_0, label l >= 1 replaces iff cand_l < best;  apply: greedy_control again on the same operands;
//   flight       (a noisy plant only) K25's: the drawn node's offsets added on the FLIGHT set's mask - another set than the
//                lookahead's: the lookahead set is what the controller believes, the flight set is the plant.
// The lookahead block is [p (W) | e (n_axes x W)]: row j the j-th masked axis, node index fastest.  It is indexed by the node
// counter only, so on the device it is read through the constant address space: scalar loads into scalar registers.
#pragma once
#include "hjbdp_greedy.h"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace hjb {

// the lookahead node set as the kernel and the twin read it
struct LookSet {
    int32_t mode;                     // HJB_DIST_EXPECT / HJB_DIST_WORST
    int32_t n_nodes;                  // W; 0: no set
    int32_t mask, n_axes;             // the axes with an offset that is not +-0; n_axes = popcount(mask)
    const double *tab;                // [p (W) | e (n_axes x W)]
};

// element i of the lookahead block: i is wave-uniform (the node counter), the block is not written while a kernel runs
HJB_GREEDY_FN double look_read(const double *tab, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) double *cptr;
    return ((cptr)(uintptr_t)tab)[i];
#else
    return tab[i];
#endif
}

// The block of a node set: mask and n_axes into S, [p | e] into tab (W + D * W doubles at most; S.tab is left alone).
// offsets [D, W] column-major; weights null: 1.0 / W each; weights are used as given, not normalised.
inline int look_table(int D, int n_nodes, const double *offsets, const double *weights, LookSet &S, double *tab) {
    int mask = 0, n_axes = 0;
    for (int w = 0; w < n_nodes; ++w)
        for (int a = 0; a < D; ++a)
            if (offsets[a + (int64_t)D * w] != 0.0) mask |= 1 << a;
    for (int w = 0; w < n_nodes; ++w) tab[w] = weights ? weights[w] : 1.0 / n_nodes;
    double *row = tab + n_nodes;
    for (int a = 0; a < D; ++a) {
        if (!((mask >> a) & 1)) continue;
        for (int w = 0; w < n_nodes; ++w) row[w] = offsets[a + (int64_t)D * w];
        row += n_nodes;
        ++n_axes;
    }
    S.n_nodes = n_nodes;
    S.mask = mask;
    S.n_axes = n_axes;
    return n_nodes + n_axes * n_nodes;
}

// M again once per node of the node loop, where that is the form: below D = 3 (look_value)
template <int D, typename MODEL>
HJB_GREEDY_FN const MODEL &greedy_reread_per_node(const MODEL &M) {
    if constexpr (D < 3) return record_reread(M);
    else return M;
}

// greedy_value's first half for one axis: the weight of q on axis a, and its cell's offset in the plane (returned)
template <int D, typename MODEL>
HJB_GREEDY_FN int64_t look_locate(const MODEL &M0, const double *kn, const double *rd, int a, double q, double &t) {
    const MODEL &M = greedy_reread_in_loop<D>(M0);
    const double *kk = kn + M.koff[a];
    const int cell = greedy_cell(kk, M.n[a], q, M.uniform[a], M.x0[a], M.inv_h[a]);
    t = (double)((double)(q - kk[cell]) * rd[M.koff[a] + cell]);
    return M.stride[a] * cell;
}

// greedy_value's second half: the blend of `plane` at the point whose cell starts at `base` with the weights `tw`, in the same
// corner groups (the group size only sets how many gathers are in flight - the fold order and the bits do not depend on it; groups
// of 8 were tried at D = 5 and 6 and need MORE registers, 146 - 218, the compiler then issuing several groups' gathers at once)
template <int D, typename TV, typename MODEL>
HJB_GREEDY_FN double look_blend(const MODEL &M0, const TV *plane, int64_t base, const double (&tw)[D]) {
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
#if defined(__HIP_DEVICE_COMPILE__)
        // D = 5: nothing is scheduled across the end of a group.  Without this the second group's 16 gathers are issued under the
        // first group's folds and the double-plane forms need 130 vector registers; with it every D = 5 form fits 128 (115 - 124).
        // Scheduling only: the operations and their operands are the same.  At D = 6 it changes no count and is left out.
        if constexpr (D == 5) __builtin_amdgcn_sched_barrier(0);
#endif
    }
    return s[D];
}

// E_w / max_w of the plane at xn + e_w over the node set: the candidate's acc
template <int D, typename TV, typename MODEL, typename LOOK>
HJB_GREEDY_FN double look_value(const MODEL &M0, const LOOK &L0, const double *kn, const double *rd, const TV *plane,
                                const double (&xn)[D]) {
    const int mask = L0.mask, W = L0.n_nodes;
    const bool worst = L0.mode == HJB_DIST_WORST;
    double tw[D];
    int64_t shared = 0;                                       // the cells of the axes outside the mask: one offset (sums of int64: exact)
#pragma unroll
    for (int a = 0; a < D; ++a) {
        tw[a] = 0.0;
        if (!(mask & (1 << a))) shared += look_locate<D>(M0, kn, rd, a, xn[a], tw[a]);
    }
    double acc = 0.0;
    const double *tab = L0.tab;
    for (int w = 0; w < W; ++w) {
        const double pw = look_read(tab, w);
        // D < 3: the node's scalars in one batch, held for the node alone; from D = 3 on look_locate and look_blend reread per body
        const MODEL &Mw = greedy_reread_per_node<D>(M0);
        int row = W + w;
        int64_t base = shared;
#pragma unroll
        for (int a = 0; a < D; ++a)
            if (mask & (1 << a)) {
                const double q = xn[a] + look_read(tab, row);
                row += W;
                base += look_locate<D>(Mw, kn, rd, a, q, tw[a]);
            }
        const double v = look_blend<D, TV>(Mw, plane, base, tw);
        if (worst) acc = (w == 0 || v > acc) ? v : acc;
        else acc = w == 0 ? (double)(pw * v) : __builtin_fma(pw, v, acc);
    }
    return acc;
}

// look_step at n_u = NU
template <int D, int NU, typename TV, typename MODEL, typename LOOK>
HJB_GREEDY_FN void look_step_nu(const MODEL &M0, const LOOK &L0, const double *kn, const double *rd, const double *ut, const TV *plane,
                                double (&x)[D], double (&u)[HJB_ROLLOUT_MAX_U], double &g, int &label, double &best) {
    double gs, as[D];
    greedy_state_parts<D>(record_reread(M0), x, gs, as);
    double bst = 0.0;
    int lb = 0;
    const int nl = M0.n_labels;
    for (int l = 0; l < nl; ++l) {
        double ul[HJB_ROLLOUT_MAX_U], xn[D];
        const double gl = greedy_control<D, NU>(greedy_reread_in_loop<D>(M0), ut, l, gs, as, ul, xn);
        const double acc = plane ? look_value<D, TV>(record_reread(M0), record_reread(L0), kn, rd, plane, xn) : 0.0;
        const double cand = gl + acc;
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

// One step at x, greedy_step's interface with the lookahead set beside the model: on return x is the NOMINAL next state of the
// chosen label (the caller adds the plant's noise), u its control, g its stage cost, best the minimum over the candidates.
template <int D, typename TV, typename MODEL, typename LOOK>
HJB_GREEDY_FN void look_step(const MODEL &M, const LOOK &L, const double *kn, const double *rd, const double *ut, const TV *plane,
                             double (&x)[D], double (&u)[HJB_ROLLOUT_MAX_U], double &g, int &label, double &best) {
    static_assert(HJB_ROLLOUT_MAX_U == 4, "one case per n_u below");
    switch (M.n_u) {
        case 1: look_step_nu<D, 1, TV>(M, L, kn, rd, ut, plane, x, u, g, label, best); break;
        case 2: look_step_nu<D, 2, TV>(M, L, kn, rd, ut, plane, x, u, g, label, best); break;
        case 3: look_step_nu<D, 3, TV>(M, L, kn, rd, ut, plane, x, u, g, label, best); break;
        default: look_step_nu<D, 4, TV>(M, L, kn, rd, ut, plane, x, u, g, label, best); break;
    }
}

// The host twin's loop: greedy_rollout_host's with the lookahead set, and, when `nodes` is given, a plant flown under the nodes
// nodes[i + n_traj * k] (what hjb_rollout_noise_draw writes) of the flight offsets fd [D, W_f] column-major, added on the axes of
// fmask alone.
template <int D, typename TV>
inline void lookahead_rollout_host(const GreedyModel &M, const LookSet &L, const double *knots, const double *rdx, const double *u_table,
                                   const TV *values, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj, const double *X0,
                                   const int32_t *nodes, int fmask, const double *fd, double *X_final, double *cost, double *X_path,
                                   double *U_path, double *L_path, double *V_path) {
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
            look_step<D, TV>(M, L, knots, rdx, u_table, plane, x, u, g, label, best);
            J = J + g;
            if (nodes) {
                const int64_t w = nodes[i + n_traj * k];
                for (int a = 0; a < D; ++a)
                    if (fmask & (1 << a)) x[a] = x[a] + fd[a + (int64_t)D * w];
            }
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
