// kernels_disturb.h - variant 8 (K24): the stage kernel of a handle with a disturbance (hjb_set_disturbance, include/hjbdp.h).
//
//   J_k(x) = min_u  g(x, u) + COMBINE_w F_{k+1}(x_next(x, u) + d_w)      COMBINE = sum_w p_w (.) (HJB_DIST_EXPECT) or max_w (.) (HJB_DIST_WORST)
//
// One thread per owned state, grid-stride, as k_backup_generic: controls are the outer loop (control dim 0 slowest, first minimum
// wins), the W nodes the inner loop.  Per state the control-independent prefixes of the term sums and of the cost are formed once;
// per control the term sums q_a, the stage cost g and - for the axes no node offsets (DDisturb::axes, a launch constant: wave-uniform
// branches) - the cell and weight; per node only the offset axes are located again, q_aw = (TQ)(q_a + d[a][w]), then the 2^D corners
// are gathered (axis-0 neighbours in one load: jstride[0] == 1) and lerped by HJB_LERP_AXES (hjbdp_canon.h, as every other piece here).
//   EXPECT: acc = (T)(p_0 v_0), acc = fma(p_w, v_w, acc) in node order.   WORST: acc = v_0, acc = v_w > acc ? v_w : acc.
//   candidate = (T)(g + acc).  With one node, no offset axis and p_0 = 1 every operation is k_backup_generic's: the same bits.
// The node offsets and weights sit in one small device block behind a kernel-argument pointer and are indexed by the node counter
// only: scalar loads into scalar registers, no per-lane traffic, no LDS.
//   TQ: the type queries are formed, located and weighted in.  HJB_TAB_F64: double - PQ is the handle's float64 shadow of the axes
//   (knots, 1/dx, next-state terms: Handle::dp64), the weight is rounded to float once; the stage-invariant (cell, weight) tables the
//   other kernels read for this typing cannot serve an offset query.  Otherwise TQ = T and PQ = P.
//   HJB_COST_F64: state part of the cost summed once per state in double, each control adds its part and rounds once.
//   FIXED: the fixed-label form (hjb_evaluate*): the thread reads its label, decodes it column-major and forms that ONE candidate -
//   the same operations on the same operands, so the same bits as the candidate the min form compares.  A label out of range: nothing
//   is read, NaN is stored, *bad_label is raised (kernels_evaluate.h's rule).
//   IX: int64_t serves any size; uint32_t is the same kernel where the host found every state index and J offset below 2^31
//   (eval_runs_i32).  The floating-point operations do not depend on it.
// Whole grids only (hjb_set_disturbance refuses slab handles): no halo, no plane window.  No LDS.
#pragma once
#include "hjbdp_dev.h"
#include "hjbdp_canon.h"

namespace hjb {

// the device block of one handle's disturbance, typed as the kernel reads it (the host fills it once per hjb_set_disturbance)
template <typename TQ, typename T>
struct DDisturb {
    int32_t n_nodes;
    int32_t mode;                               // HJB_DIST_EXPECT / HJB_DIST_WORST
    uint32_t axes;                              // bit a: some node offsets axis a
    int32_t pad;
    TQ off[HJB_MAX_D][HJB_DIST_MAX_NODES];      // d[a][w], rounded once to TQ
    T p[HJB_DIST_MAX_NODES];                    // weights, rounded once to T (EXPECT)
};

template <typename TQ, typename IX, int D>
__device__ __forceinline__ TQ dist_term(const DTerm &t, const int (&si)[D], const int (&cj)[HJB_MAX_C]) {
    return as_global<TQ>(t.data)[eval_term_off<IX, false, D>(t, si, cj)];
}

template <typename T, typename TJ, typename TQ, int D, typename IX, bool FIXED>
__global__ void __launch_bounds__(256)
k_backup_disturb(const DParams *__restrict__ P, const DParams *__restrict__ PQ, const DDisturb<TQ, T> *__restrict__ DW,
                 const TJ *__restrict__ Jn, TJ *__restrict__ Jout, void *__restrict__ idx_out,
                 const void *__restrict__ labels, int32_t *__restrict__ bad_label) {
    const int C = P->C;
    const IX n_owned = (IX)P->n_owned;
    const IX nU = (IX)P->nU;
    const int W = DW->n_nodes;
    const bool worst = DW->mode == HJB_DIST_WORST;
    const uint32_t axes = DW->axes;
    const bool c64 = P->cost_f64 != 0;
    const int idx_bytes = P->idx_bytes, index_base = P->index_base;
    IX js[D];
#pragma unroll
    for (int a = 0; a < D; ++a) js[a] = (IX)P->jstride[a];
    HJB_PAIR_OFFSETS(IX, 1 << (D - 1), D, poff, js)
    const IX stride = (IX)gridDim.x * (IX)blockDim.x;
    for (IX ls = (IX)blockIdx.x * (IX)blockDim.x + (IX)threadIdx.x; ls < n_owned; ls += stride) {
        int cj[HJB_MAX_C] = {0, 0, 0};
        IX u_first = 0, u_end = nU;
        if (FIXED) {
            // (the label minus the base in 64 bits: an int32 label of any value stays what it is)
            const int64_t lab64 = (int64_t)ld_label(labels, (int64_t)ls, idx_bytes) - index_base;
            if (lab64 < 0 || lab64 >= (int64_t)nU) {
                *bad_label = 1;
                stj<T, TJ>(Jout, (int64_t)ls, eval_nan<T>());
                continue;
            }
            IX lab = (IX)lab64;                               // column-major label: control dim 0 fastest
            if (C == 1) {
                cj[0] = (int)lab;
            } else {
                cj[0] = (int)(lab % (IX)P->m[0]);
                lab /= (IX)P->m[0];
                if (C == 2) cj[1] = (int)lab;
                else { cj[1] = (int)(lab % (IX)P->m[1]); cj[2] = (int)(lab / (IX)P->m[1]); }
            }
            u_end = 1;                                        // one candidate
        }
        int si[D];
        {
            IX r = ls;
#pragma unroll
            for (int a = 0; a < D - 1; ++a) {
                const IX na = (IX)P->n[a];
                const IX qd = r / na;
                si[a] = (int)(r - qd * na);
                r = qd;
            }
            si[D - 1] = (int)r;
        }
        // control-independent prefixes, once per state (the fixed-label form has one control: everything is formed below)
        TQ qpre[D];
        T gpre = (T)0;
        double gpre64 = 0.0;
        if (!FIXED) {
            const int zc[HJB_MAX_C] = {0, 0, 0};
#pragma unroll
            for (int a = 0; a < D; ++a) {
                const DAxis &ax = PQ->axis[a];
                TQ q = (TQ)0;
                HJB_TERM_SUM(TQ, q, k, 0, ax.n_prefix, dist_term<TQ, IX, D>(ax.t[k], si, zc))
                qpre[a] = q;
            }
            if (c64) {
                HJB_TERM_SUM(double, gpre64, k, 0, P->n_cost_prefix, dist_term<double, IX, D>(P->cost64[k], si, zc))
            } else {
                HJB_TERM_SUM(T, gpre, k, 0, P->n_cost_prefix, dist_term<T, IX, D>(P->cost[k], si, zc))
            }
        }

        T best = (T)0;
        IX best_u = 0;
        for (IX u = u_first; u < u_end; ++u) {
            // per control: the term sums, the cells and weights of the axes no node offsets, the stage cost
            TQ q[D];
            T tw[D];
            IX base_shared = 0;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                const DAxis &ax = PQ->axis[a];
                TQ s = FIXED ? (TQ)0 : qpre[a];
                HJB_TERM_SUM(TQ, s, k, FIXED ? 0 : ax.n_prefix, ax.n_terms, dist_term<TQ, IX, D>(ax.t[k], si, cj))
                q[a] = s;
                if (!(axes & (1u << a))) {
                    const int cell = canon_locate<T, TQ, true>(ax, s, tw[a]);
                    base_shared += a == 0 ? (IX)cell : js[a] * (IX)cell;
                }
            }
            T g;
            if (c64) {
                double g64 = FIXED ? 0.0 : gpre64;
                HJB_TERM_SUM(double, g64, k, FIXED ? 0 : P->n_cost_prefix, P->n_cost, dist_term<double, IX, D>(P->cost64[k], si, cj))
                g = (T)g64;
            } else {
                g = FIXED ? (T)0 : gpre;
                HJB_TERM_SUM(T, g, k, FIXED ? 0 : P->n_cost_prefix, P->n_cost, dist_term<T, IX, D>(P->cost[k], si, cj))
            }
            T acc = (T)0;
            for (int w = 0; w < W; ++w) {
                const T pw = DW->p[w];                           // read first: the scalar load's latency passes under the gathers
                IX base = base_shared;
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    if (axes & (1u << a)) {
                        const int cell = canon_locate<T, TQ, true>(PQ->axis[a], (TQ)(q[a] + DW->off[a][w]), tw[a]);
                        base += a == 0 ? (IX)cell : js[a] * (IX)cell;
                    }
                }
                T v[1 << D];
#pragma unroll
                for (int p = 0; p < (1 << (D - 1)); ++p)         // corners 2p, 2p + 1: the axis-0 neighbours, one load
                    tab_load_pair(Jn, (int64_t)(base + poff[p]), v[2 * p], v[2 * p + 1]);
                HJB_LERP_AXES(T, D, v, a, 0, D, tw[a])
                if (worst) acc = (w == 0) ? v[0] : (v[0] > acc ? v[0] : acc);
                else acc = (w == 0) ? (T)(pw * v[0]) : fma_t<T>(pw, v[0], acc);
            }
            const T tot = (T)(g + acc);
            if (u == u_first || tot < best) {
                best = tot;
                best_u = u;
            }
            if (!FIXED) { HJB_NEXT_CONTROL(C, cj, P->m[1], P->m[2]) }
        }
        stj<T, TJ>(Jout, (int64_t)ls, best);
        if (!FIXED && idx_out) {
            int64_t label;
            const int64_t bu = (int64_t)best_u;
            HJB_LABEL(label, int64_t, int64_t, C, bu, P->m[0], P->m[1], P->m[2])
            st_idx(idx_out, (int64_t)ls, (int32_t)(label + index_base), idx_bytes);
        }
    }
}

}  // namespace hjb
