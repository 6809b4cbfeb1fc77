// hjbdp_ctrl_lookahead.h - one step of the lookahead rollout under a CONTROL-DEPENDENT node set (K35,
// kernels_rollout_ctrl_lookahead.h; K36, kernels_rollout_ctrl_lookahead_campaign.h): K27's one-step lookahead (hjbdp_lookahead.h)
// with the control-dependent backup's E_w / max_w (K32, hjb_set_control_disturbance) inside every candidate,
//   u_k(x) = argmin_l  g(x, u_l) + E_w[ J_{k+1}(f(x, u_l) + e_w(l)) ]      (HJB_DIST_EXPECT; HJB_DIST_WORST: max_w)
// at the state actually visited - what flies the value function K32 produces.  Written once for the kernels and the host twin
// hjb_rollout_control_lookahead_host (rollout_ctrl_lookahead_host.hip).  No HIP dependency: tests/ctrl_lookahead_harness.cpp
// compiles it as plain C++.  The contract is K27's (hjbdp_lookahead.h, lines 6-17) with ONE change, the one
// hjb_set_control_disturbance makes to hjb_set_disturbance's contract:
//   node w of the candidate with 0-based label l: q_aw = xn_a + e[a][w][l] on the masked axes;
//   the mask has bit a set iff some (w, l) entry of row a is not +-0;
//   an axis outside the mask is located once per candidate and is not touched by + 0.0.
// Everything else is called, not restated: greedy_state_parts and greedy_control (hjbdp_greedy.h), look_locate, look_blend and
// look_read (hjbdp_lookahead.h), the combine (p_0 v_0 rounded then fma, or the first maximum) and K26's first-minimum choice in
// the statements look_value and look_step_nu have them.  EVERY node is evaluated for EVERY candidate, also for a candidate whose
// offsets are all zero: the bits are the contract's, not a shortcut's (K32's rule).
// The block is [p (W) | for l = 0 .. n_labels-1: e (n_axes x W)]: candidate l's rows are contiguous, n_axes * W doubles from
// W + l * n_axes * W on; within them row j is the j-th masked axis, node index fastest - K27's [p | e] with one e per candidate.
// It is indexed by the node counter and the candidate counter only, both wave-uniform, so on the device it is read through the
// constant address space into scalar registers (look_read), never per lane and never staged in LDS.
// This is a function of its own beside look_value, not a hook in it: hjbdp_lookahead.h is the text it was, and every unit that
// includes it (rollout_lookahead*.hip, rollout_lookahead_campaign*.hip) compiles to the code object it had.
// The flown plant of the host twin is K33's (kernels_rollout_actuator.h, steps 3 - 4) at a GIVEN node: ctrl_look_actuator_host.
#pragma once
#include "hjbdp_lookahead.h"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace hjb {

// the per-control lookahead node set as the kernels and the twin read it
struct CtrlLookSet {
    int32_t mode;                     // HJB_DIST_EXPECT / HJB_DIST_WORST
    int32_t n_nodes;                  // W; 0: no set
    int32_t mask, n_axes;             // the axes with a (w, l) entry that is not +-0; n_axes = popcount(mask)
    int32_t n_controls, reserved_;    // the labels the table was given for (the object's n_labels)
    const double *tab;                // [p (W) | for l: e (n_axes x W)]
};

// The block of a per-control node set: mask and n_axes into S, the block into tab (W + n_controls * D * W doubles at most; S.tab is
// left alone).  offsets [D, W, n_controls] column-major (hjb_set_control_disturbance's argument); weights null: 1.0 / W each;
// weights are used as given, not normalised.  -> the doubles written
inline int64_t ctrl_look_table(int D, int n_nodes, int n_controls, const double *offsets, const double *weights, CtrlLookSet &S,
                               double *tab) {
    int mask = 0, n_axes = 0;
    for (int64_t c = 0; c < (int64_t)n_nodes * n_controls; ++c)
        for (int a = 0; a < D; ++a)
            if (offsets[a + (int64_t)D * c] != 0.0) mask |= 1 << a;
    for (int a = 0; a < D; ++a) n_axes += (mask >> a) & 1;
    for (int w = 0; w < n_nodes; ++w) tab[w] = weights ? weights[w] : 1.0 / n_nodes;
    double *row = tab + n_nodes;
    for (int l = 0; l < n_controls; ++l)
        for (int a = 0; a < D; ++a) {
            if (!((mask >> a) & 1)) continue;
            for (int w = 0; w < n_nodes; ++w) row[w] = offsets[a + (int64_t)D * (w + (int64_t)n_nodes * l)];
            row += n_nodes;
        }
    S.n_nodes = n_nodes;
    S.n_controls = n_controls;
    S.mask = mask;
    S.n_axes = n_axes;
    return (int64_t)n_nodes + (int64_t)n_controls * n_axes * n_nodes;
}

// E_w / max_w of the plane at xn + e_w(l) over candidate l's nodes: look_value with the rows of the candidate.  l is the
// candidate counter: wave-uniform, so the row index stays a scalar.
template <int D, typename TV, typename MODEL, typename LOOK>
HJB_GREEDY_FN double ctrl_look_value(const MODEL &M0, const LOOK &L0, const double *kn, const double *rd, const TV *plane,
                                     const double (&xn)[D], int l) {
    const int mask = L0.mask, W = L0.n_nodes;
    const bool worst = L0.mode == HJB_DIST_WORST;
    const int first = W + l * (L0.n_axes * W);               // candidate l's rows (at most 2^26 entries: an int holds it)
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
        const MODEL &Mw = greedy_reread_per_node<D>(M0);      // look_value's rule: per node below D = 3, per loop body from there on
        int row = first + w;
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

// ctrl_look_step at n_u = NU: look_step_nu with the candidate's own rows
template <int D, int NU, typename TV, typename MODEL, typename LOOK>
HJB_GREEDY_FN void ctrl_look_step_nu(const MODEL &M0, const LOOK &L0, const double *kn, const double *rd, const double *ut,
                                     const TV *plane, double (&x)[D], double (&u)[HJB_ROLLOUT_MAX_U], double &g, int &label, double &best) {
    double gs, as[D];
    greedy_state_parts<D>(record_reread(M0), x, gs, as);
    double bst = 0.0;
    int lb = 0;
    const int nl = M0.n_labels;
    for (int l = 0; l < nl; ++l) {
        double ul[HJB_ROLLOUT_MAX_U], xn[D];
        const double gl = greedy_control<D, NU>(greedy_reread_in_loop<D>(M0), ut, l, gs, as, ul, xn);
        const double acc = plane ? ctrl_look_value<D, TV>(record_reread(M0), record_reread(L0), kn, rd, plane, xn, l) : 0.0;
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

// One step at x, look_step's interface: on return x is the NOMINAL next state of the chosen label (the caller flies the plant on
// it), u its commanded control, g its stage cost, best the minimum over the candidates.
template <int D, typename TV, typename MODEL, typename LOOK>
HJB_GREEDY_FN void ctrl_look_step(const MODEL &M, const LOOK &L, const double *kn, const double *rd, const double *ut, const TV *plane,
                                  double (&x)[D], double (&u)[HJB_ROLLOUT_MAX_U], double &g, int &label, double &best) {
    static_assert(HJB_ROLLOUT_MAX_U == 4, "one case per n_u below");
    switch (M.n_u) {
        case 1: ctrl_look_step_nu<D, 1, TV>(M, L, kn, rd, ut, plane, x, u, g, label, best); break;
        case 2: ctrl_look_step_nu<D, 2, TV>(M, L, kn, rd, ut, plane, x, u, g, label, best); break;
        case 3: ctrl_look_step_nu<D, 3, TV>(M, L, kn, rd, ut, plane, x, u, g, label, best); break;
        default: ctrl_look_step_nu<D, 4, TV>(M, L, kn, rd, ut, plane, x, u, g, label, best); break;
    }
}

// The actuator plant of the host twin, as its arguments give it: eps [n_u, W_f] and base [D, W_f] (or null) column-major, and what
// hjb_rollout_set_actuator_noise and actuator_terms (kernels_rollout_actuator.h) form of them and of B
struct CtrlLookPlant {
    int32_t n_nodes, live, base_mask;
    uint32_t terms;                   // bit j + HJB_ROLLOUT_MAX_U * a: input j is live and B[a,j] is not +-0
    const double *eps, *base;
};

inline void ctrl_look_plant(int D, int nu, int n_nodes, const double *eps, const double *base, const double *B, CtrlLookPlant &P) {
    P.n_nodes = n_nodes;
    P.eps = eps;
    P.base = base;
    P.live = P.base_mask = 0;
    P.terms = 0;
    for (int w = 0; w < n_nodes; ++w) {
        for (int j = 0; j < nu; ++j)
            if (eps[j + (int64_t)nu * w] != 0.0) P.live |= 1 << j;
        for (int a = 0; base && a < D; ++a)
            if (base[a + (int64_t)D * w] != 0.0) P.base_mask |= 1 << a;
    }
    for (int a = 0; a < D; ++a)
        for (int j = 0; j < nu; ++j)
            if (((P.live >> j) & 1) && B[a + D * j] != 0.0) P.terms |= 1u << (j + HJB_ROLLOUT_MAX_U * a);
}

// K33's steps 3 - 4 at the GIVEN node w (HJB_ROLLOUT_ACTUATOR_STEP's arithmetic, kernels_rollout_actuator.h): ue_j = u_j * eps[j][w]
// for the live inputs, then per axis the terms B[a,j] * ue_j for live j ascending with B[a,j] not +-0 and base[a][w] on a base axis,
// summed left to right from the first term; an axis with no term is not touched.  u is consumed, as the macro consumes it.
template <int D>
inline void ctrl_look_actuator_host(const CtrlLookPlant &P, int nu, const double *B, int64_t w, double (&u)[HJB_ROLLOUT_MAX_U],
                                    double (&x)[D]) {
    for (int j = 0; j < nu; ++j)
        if ((P.live >> j) & 1) u[j] = u[j] * P.eps[j + (int64_t)nu * w];
    for (int a = 0; a < D; ++a) {
        double n = -0.0;                                      // -0.0 + t is t, bit for bit: the first term starts the sum
        for (int j = 0; j < nu; ++j)
            if (P.terms & (1u << (j + HJB_ROLLOUT_MAX_U * a))) n = n + B[a + D * j] * u[j];
        if ((P.base_mask >> a) & 1) n = n + P.base[a + (int64_t)D * w];
        x[a] = x[a] + n;                                      // no term: x + -0.0 is x, bit for bit
    }
}

// The host twin's loop: lookahead_rollout_host's with the per-control set and, when `nodes` is given, the actuator plant flown
// under the nodes nodes[i + n_traj * k] (what hjb_rollout_noise_draw writes).  The cost is charged on the commanded u, and U_path
// holds it.
template <int D, typename TV>
inline void ctrl_lookahead_rollout_host(const GreedyModel &M, const CtrlLookSet &L, const double *knots, const double *rdx,
                                        const double *u_table, const TV *values, int32_t n_steps, const int32_t *plane_of_step,
                                        int64_t n_traj, const double *X0, const int32_t *nodes, const CtrlLookPlant &P, double *X_final,
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
            ctrl_look_step<D, TV>(M, L, knots, rdx, u_table, plane, x, u, g, label, best);
            J = J + g;
            if (U_path)
                for (int j = 0; j < nu; ++j) U_path[i + n_traj * (j + (int64_t)nu * k)] = u[j];
            if (nodes) ctrl_look_actuator_host<D>(P, nu, M.B, nodes[i + n_traj * k], u, x);
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
