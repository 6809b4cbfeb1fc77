// kernels_disturb_body.inc - the body of the disturbed stage kernel, the one text k_backup_disturb (K24, kernels_disturb.h) and
// k_backup_ctrldist (K32, kernels_ctrldist.h) are made of.  The includer provides the template parameters T, TJ, TQ, D, IX, FIXED, the
// arguments P, PQ, DW, Jn, Jout, idx_out, labels, bad_label and ONE hook:
//   HJB_DIST_OFFSET(a, w)   node w's offset of axis a, in TQ - read inside the node loop, where the loop counter u (min form) and the
//                           decoded cj[] (fixed-label form, after the label's range check) are in scope.
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
                        const int cell = canon_locate<T, TQ, true>(PQ->axis[a], (TQ)(q[a] + HJB_DIST_OFFSET(a, w)), tw[a]);
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
