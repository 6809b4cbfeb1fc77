// kernels_generic.h - variant 0: the fully general stage kernel.
//
// One thread per owned state; the thread walks every control (control dim 0
// slowest = the reference's cascade min, Solver_attitude.m:400-409), evaluates
// the ordered broadcast-term sums for x_next and g on the fly, finds the cell by
// exact search, gathers the 2^D corners of J_{k+1} straight from global memory
// (L1/L2/MALL resident for every reference-sized grid) and keeps the first
// minimum.  Arithmetic is the canonical order of oracle/hjb_oracle.c, so results
// are bit-identical to the CPU twin.  Any D <= 6, C <= 3, uniform or non-uniform
// knots, slabs with halos, float16 J storage.  The fast kernels (kernels_nested.h,
// kernels_packed*.h, kernels_ctrlsplit.h, kernels_tabled.h) cover the shapes that matter
// for throughput; this one is the safety net and the parity anchor.
#pragma once
#include "hjbdp_dev.h"
#include "hjbdp_canon.h"

namespace hjb {

template <typename T, typename TJ, int D>
__global__ void __launch_bounds__(256)
k_backup_generic(const DParams *__restrict__ P, const TJ *__restrict__ Jn, TJ *__restrict__ Jout,
                 void *__restrict__ idx_out) {
    const int C = P->C;
    const int64_t n_owned = P->n_owned;
    const int64_t nU = P->nU;
    for (int64_t ls = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; ls < n_owned;
         ls += (int64_t)gridDim.x * blockDim.x) {
        int si[D];
        HJB_STATE_INDEX(D, P, ls, si, a, )
        int cj[HJB_MAX_C] = {0, 0, 0};
        T qpre[D];
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const DAxis &ax = P->axis[a];
            T q = (T)0;
            HJB_TERM_SUM(T, q, k, 0, ax.n_prefix, term_value<T, D>(ax.t[k], si, cj))
            qpre[a] = q;
        }
        T gpre = (T)0;
        HJB_TERM_SUM(T, gpre, k, 0, P->n_cost_prefix, term_value<T, D>(P->cost[k], si, cj))

        T best = (T)0;
        int64_t best_u = 0;
        for (int64_t u = 0; u < nU; ++u) {
            T tw[D];
            int64_t base = 0;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                const DAxis &ax = P->axis[a];
                T q = qpre[a];
                HJB_TERM_SUM(T, q, k, ax.n_prefix, ax.n_terms, term_value<T, D>(ax.t[k], si, cj))
                int cell = canon_locate<T, T, false>(ax, q, tw[a]);
                if (a == D - 1) { HJB_PLANE_CLAMP(cell, P->plane0, P->nplanes, *P->status = 1) }
                base += P->jstride[a] * cell;
            }
            T v[1 << D];
#pragma unroll
            for (int c = 0; c < (1 << D); ++c) {
                int64_t off = base;
#pragma unroll
                for (int a = 0; a < D; ++a)
                    if (c & (1 << a)) off += P->jstride[a];
                v[c] = ldj<T, TJ>(Jn, off);
            }
            HJB_LERP_AXES(T, D, v, a, 0, D, tw[a])
            T g = gpre;
            HJB_TERM_SUM(T, g, k, P->n_cost_prefix, P->n_cost, term_value<T, D>(P->cost[k], si, cj))
            T tot = (T)(g + v[0]);
            if (u == 0 || tot < best) {
                best = tot;
                best_u = u;
            }
            HJB_NEXT_CONTROL(C, cj, P->m[1], P->m[2])
        }
        int64_t label;
        HJB_LABEL(label, int64_t, int64_t, C, best_u, P->m[0], P->m[1], P->m[2])
        const int64_t in_plane = ls % P->inner, pl = ls / P->inner;
        stj<T, TJ>(Jout, in_plane + P->inner * (pl + P->halo_lo), best);
        if (idx_out) st_idx(idx_out, ls, (int32_t)(label + P->index_base), P->idx_bytes);
    }
}

// Stage-invariant per-axis (cell, weight) table over the axis' broadcast domain
// (used by variant 2).  One thread per domain entry; same canonical arithmetic as
// the stage kernels (hjbdp_canon.h): ordered term sum, locate.
// dom_size[d] = grid size of dim d if d is in the domain, else 1; entries are laid
// out column-major over the domain dims in increasing dim order.
template <typename T, int D>
__global__ void __launch_bounds__(256)
k_prep_axis_table(const DParams *__restrict__ P, int a, const int32_t *__restrict__ dom_size, int64_t n_entries,
                  int2 *__restrict__ out) {
    const DAxis &ax = P->axis[a];
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n_entries;
         e += (int64_t)gridDim.x * blockDim.x) {
        int si[D];
        int cj[HJB_MAX_C] = {0, 0, 0};
        int64_t r = e;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int sz = dom_size[d];
            si[d] = (int)(r % sz);
            r /= sz;
        }
#pragma unroll
        for (int c = 0; c < HJB_MAX_C; ++c) {
            const int sz = dom_size[D + c];
            cj[c] = (int)(r % sz);
            r /= sz;
        }
        si[D - 1] += P->slab_begin;   // term tables are indexed by GLOBAL grid indices; the domain covers owned planes
        T q = (T)0;
        HJB_TERM_SUM(T, q, k, 0, ax.n_terms, term_value<T, D>(ax.t[k], si, cj))
        const T *kk = static_cast<const T *>(ax.knots);
        int cell;
        float t;
        HJB_LOCATE(T, ax, kk, static_cast<const T *>(ax.rdx), q, cell, t, (float));
        out[e] = make_int2(cell, __float_as_int(t));
    }
}

}  // namespace hjb
