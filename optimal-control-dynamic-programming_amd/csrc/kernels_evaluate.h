// kernels_evaluate.h - the fixed-label stage: J_k(x) = g(x, u_k(x)) + F_{k+1}(x_next(x, u_k(x))) for a GIVEN policy u_k.
//
// One thread per owned state, axis 0 fastest (label loads and J stores coalesce; neighbouring lanes with equal labels land in
// neighbouring cells, so the axis-0 corner pairs mostly coalesce too).  The thread reads its label, decodes it column-major
// (first control dim fastest: the layout the stage kernels WRITE, not their visiting order) and forms exactly the candidate value
// the stage kernels form for that (state, control), from the same statements (hjbdp_canon.h: HJB_TERM_SUM, HJB_LOCATE, HJB_PLANE_CLAMP,
// HJB_LERP_AXES), tot = (T)(g + v[0]).  Bit-identical to the value the backup kernels compare.
//   TABLED: cells and weights come from the handle's stage-invariant (cell, t) tables (kernels_tabled.h; HJB_TAB_F64 handles always:
//   their tables are built in double, the weight rounded once); otherwise the terms are summed and located on the fly.
//   HJB_COST_F64: state part and control part of the cost summed in double, one rounding (k_backup_tabled).
// A label outside [index_base, index_base + nU): nothing is read for that state, NaN is stored, *bad_label is set; every other
// state is unaffected.  A query that leaves the slab raises DParams::status and is clamped, as in the stage kernels.  No LDS.
//   IX: the type the state index, the J offsets and the table offsets are formed in.  int64_t serves any size.  uint32_t is the same
//   kernel where every one of them fits 31 bits (the host decides: launch_evaluate): per state the work is index arithmetic - taking
//   the state index apart, decoding the label, the table and corner offsets - around 2^(D-1) pair loads and 2^D - 1 fmas, and 64-bit
//   division and multiplication cost several times their 32-bit forms on this machine (the 64-bit form's timing: DESIGN.md section 4).
//   The 32-bit form also divides by multiplication (EvalDiv: hjbdp_walk.h magic_div, formed by the host per launch) and reads its
//   terms at 32-bit offsets (hjb_create keeps every term below 2^31 elements).  Both forms skip the multiplies of a term's or a
//   table's zero strides (wave-uniform branches: most terms vary along one or two of the D + C dims).
//   M24 (32-bit form only): every stride, index and quotient the kernel multiplies is below 2^24 (the host checked each one:
//   launch_evaluate), so the index products are the full-rate 24-bit multiply instead of the quarter-rate 32-bit one.
//   The floating-point operations, their operands and their order depend on neither: same bits (tested against each other).
#pragma once
#include <type_traits>
#include "hjbdp_dev.h"
#include "hjbdp_walk.h"          // xcd_share
#include "hjbdp_canon.h"
#include "kernels_tabled.h"      // TabEntry, DTabled

namespace hjb {

// the divisors of one launch, by value: n[a] = axis a's size (a < D - 1: what the state index is taken apart by), m[c] = control dim c's
struct EvalDiv {
    MagicDiv n[HJB_MAX_D];
    MagicDiv m[2];
};

// q = r / k.d, rem = r - q * k.d
template <typename IX, bool M24>
__device__ __forceinline__ IX eval_divmod(IX r, const MagicDiv &k, int &rem) {
    IX q;
    if constexpr (std::is_same<IX, uint32_t>::value) q = magic_quot(r, k);
    else q = r / (IX)k.d;
    rem = (int)(r - eval_mul<IX, M24>(q, (IX)k.d));
    return q;
}

template <typename T, typename TJ, int D, bool TABLED, typename IX, bool M24>
__global__ void __launch_bounds__(256)
k_evaluate(const DParams *__restrict__ P, const DTabled *__restrict__ TB, const TJ *__restrict__ Jn,
           const void *__restrict__ labels, TJ *__restrict__ Jout, int32_t *__restrict__ bad_label, const EvalDiv dv) {
    const IX n_owned = (IX)P->n_owned;
    const IX nU = (IX)P->nU;
    const int C = P->C;
    const int plane0 = P->plane0, nplanes = P->nplanes;
    const int idx_bytes = P->idx_bytes, index_base = P->index_base;
    const bool c64 = P->cost_f64 != 0;
    const IX out0 = (IX)P->inner * (IX)P->halo_lo;          // owned state ls sits at ls + inner * halo_lo of a haloed J buffer
    IX js[D];
#pragma unroll
    for (int a = 0; a < D; ++a) js[a] = (IX)P->jstride[a];
    HJB_PAIR_OFFSETS(IX, 1 << (D - 1), D, poff, js)
    const IX stride = (IX)gridDim.x * (IX)blockDim.x;
    for (IX ls = (IX)xcd_share(blockIdx.x, gridDim.x) * (IX)blockDim.x + (IX)threadIdx.x; ls < n_owned; ls += stride) {
        // (the label minus the base in 64 bits: an int32 label of any value stays what it is)
        const int64_t lab64 = (int64_t)ld_label(labels, (int64_t)ls, idx_bytes) - index_base;
        if (lab64 < 0 || lab64 >= (int64_t)nU) {
            *bad_label = 1;
            stj<T, TJ>(Jout, (int64_t)(ls + out0), eval_nan<T>());
            continue;
        }
        int si[D];          // global indices (term tables)
        int sl[D];          // local index along the last axis (axis tables cover owned planes)
        {
            IX r = ls;
#pragma unroll
            for (int a = 0; a < D - 1; ++a) {
                r = eval_divmod<IX, M24>(r, dv.n[a], si[a]);
                sl[a] = si[a];
            }
            sl[D - 1] = (int)r;                              // (r < n[D-1]: ls < n_owned)
            si[D - 1] = (int)r + P->slab_begin;
        }
        // column-major label: control dim 0 fastest
        int cj[HJB_MAX_C] = {0, 0, 0};
        {
            const IX lab = (IX)lab64;
            if (C == 1) {
                cj[0] = (int)lab;
            } else {
                const IX r1 = eval_divmod<IX, M24>(lab, dv.m[0], cj[0]);
                if (C == 2) cj[1] = (int)r1;
                else cj[2] = (int)eval_divmod<IX, M24>(r1, dv.m[1], cj[1]);
            }
        }
        T tw[D];
        IX base = 0;
        bool left = false;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            int cell;
            if (TABLED) {
                const DTabled::Axis &A = TB->ax[a];
                IX off = 0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const int st = A.sstride[d];
                    if (st != 0) off += eval_mul<IX, M24>((IX)st, (IX)sl[d]);
                }
#pragma unroll
                for (int c = 0; c < HJB_MAX_C; ++c) {
                    const int st = A.cstride[c];
                    if (st != 0) off += eval_mul<IX, M24>((IX)st, (IX)cj[c]);
                }
                cell = as_global<TabEntry<T>>(A.tab)[off].cell;
                tw[a] = as_global<TabEntry<T>>(A.tab)[off].t;
            } else {
                const DAxis &ax = P->axis[a];
                T q = (T)0;
                HJB_TERM_SUM(T, q, k, 0, ax.n_terms, as_global<T>(ax.t[k].data)[eval_term_off<IX, M24, D>(ax.t[k], si, cj)])
                const T *kk = static_cast<const T *>(ax.knots);
                HJB_LOCATE(T, ax, kk, static_cast<const T *>(ax.rdx), q, cell, tw[a], (T));
            }
            if (a == D - 1) { HJB_PLANE_CLAMP(cell, plane0, nplanes, left = true) }
            base += a == 0 ? (IX)cell : eval_mul<IX, M24>(js[a], (IX)cell);      // (axis 0 is contiguous in every J layout: jstride[0] == 1)
        }
        if (left) *P->status = 1;
        T v[1 << D];
#pragma unroll
        for (int p = 0; p < (1 << (D - 1)); ++p)             // corners 2p, 2p + 1: the axis-0 neighbours, one load (jstride[0] == 1)
            tab_load_pair(Jn, (int64_t)(base + poff[p]), v[2 * p], v[2 * p + 1]);
        HJB_LERP_AXES(T, D, v, a, 0, D, tw[a])
        T g = (T)0;
        if (c64) {                               // state part, then control part, in double: ONE rounding to the arithmetic type
            double g64 = 0.0;
            HJB_TERM_SUM(double, g64, k, 0, P->n_cost, as_global<double>(P->cost64[k].data)[eval_term_off<IX, M24, D>(P->cost64[k], si, cj)])
            g = (T)g64;
        } else {
            HJB_TERM_SUM(T, g, k, 0, P->n_cost, as_global<T>(P->cost[k].data)[eval_term_off<IX, M24, D>(P->cost[k], si, cj)])
        }
        stj<T, TJ>(Jout, (int64_t)(ls + out0), (T)(g + v[0]));
    }
}

}  // namespace hjb
