// hjbdp_canon.h - the canonical backup arithmetic of DESIGN.md section 2, stated ONCE for the plain stage kernels.
//
// Every piece below is what oracle/hjb_oracle.c does, operation for operation; a kernel that uses a piece uses THIS
// statement of it.  Most pieces are macros, not functions: a macro leaves a kernel's code object byte-identical to the
// hand-written copy it replaced, a force-inlined function mostly does not ("tried and dropped";
// tools/listing_ab.py is the check).  A macro's arguments are expanded in the order the copies evaluated them; names
// ending in `_` are the macros' own.  The hand-scheduled hot paths (kernels_colsweep*, kernels_colcoop.h, kernels_uniwin.h,
// kernels_packed*.h, kernels_prep_mfma.h) keep their own text.
#pragma once
#include "hjbdp_dev.h"

namespace hjb {

template <typename T> __device__ __forceinline__ T fma_t(T a, T b, T c);
template <> __device__ __forceinline__ float fma_t<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <> __device__ __forceinline__ double fma_t<double>(double a, double b, double c) { return __builtin_fma(a, b, c); }

// clamp(upper_bound(k, q) - 1, 0, n-2), exact for any strictly increasing knots.
template <typename T>
__device__ __forceinline__ int find_cell(const T *__restrict__ k, int n, T q, int uniform, T x0, T inv_h) {
    int i;
    if (uniform) {
        T f = (q - x0) * inv_h;
        T hi = (T)(n - 2);
        f = f > (T)0 ? f : (T)0;
        f = f < hi ? f : hi;
        i = (int)f;
        while (i > 0 && q < k[i]) --i;
        while (i < n - 2 && q >= k[i + 1]) ++i;
    } else {
        int lo = 0, hi = n - 1;
        while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (k[mid] <= q) lo = mid; else hi = mid;
        }
        i = lo;
    }
    return i;
}

template <typename T, int D>
__device__ __forceinline__ T term_value(const DTerm &t, const int (&si)[D], const int (&cj)[HJB_MAX_C]) {
    int64_t off = 0;
#pragma unroll
    for (int a = 0; a < D; ++a) off += (int64_t)t.stride[a] * si[a];
#pragma unroll
    for (int c = 0; c < HJB_MAX_C; ++c) off += (int64_t)t.stride[D + c] * cj[c];
    return static_cast<const T *>(t.data)[off];
}

// ---- what the fixed-label and disturbance stages (kernels_evaluate.h, kernels_disturb.h) read their terms and corners with ---
// a * b of two index quantities (M24: both below 2^24, the product below 2^32)
template <typename IX, bool M24>
__device__ __forceinline__ IX eval_mul(IX a, IX b) {
    if constexpr (M24) return (IX)__umul24((unsigned)a, (unsigned)b);
    else return a * b;
}

// element offset of a term at (state, control); zero strides (the dims the term is broadcast along) cost a scalar compare
template <typename IX, bool M24, int D>
__device__ __forceinline__ IX eval_term_off(const DTerm &t, const int (&si)[D], const int (&cj)[HJB_MAX_C]) {
    IX off = 0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const int st = t.stride[a];
        if (st != 0) off += eval_mul<IX, M24>((IX)st, (IX)si[a]);
    }
#pragma unroll
    for (int c = 0; c < HJB_MAX_C; ++c) {
        const int st = t.stride[D + c];
        if (st != 0) off += eval_mul<IX, M24>((IX)st, (IX)cj[c]);
    }
    return off;
}

template <typename T> __device__ __forceinline__ T eval_nan();
template <> __device__ __forceinline__ float eval_nan<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double eval_nan<double>() { return __builtin_nan(""); }

// ---- the ordered term sum: the first term is taken as it is, every later one added and rounded to TT --------------------
#define HJB_TERM_ADD(TT, q, first, x) q = (first) ? x : (TT)(q + x)
// ... over terms k in [lo, hi); the last argument is the k-th term's value (an expression in k; it may hold commas)
#define HJB_TERM_SUM(TT, q, k, lo, hi, ...)         \
    for (int k = (lo); k < (hi); ++k) {             \
        const TT x_ = (__VA_ARGS__);                \
        HJB_TERM_ADD(TT, q, k == 0, x_);            \
    }

// ---- locate: cell = find_cell(knots, q), weight = (q - k[cell]) * rdx[cell], each operation rounded to TQ ----------------
#define HJB_WEIGHT(TQ, q, kc, rc) (TQ)((TQ)((q) - (kc)) * (rc))
// `kk`: the axis' knots (a pointer variable); `rdx`: its reciprocal spacings (an expression: it is evaluated after the search);
// the weight lands in `tw`, converted by WCAST (the weight's storage type)
#define HJB_LOCATE(TQ, ax, kk, rdx, q, cell, tw, WCAST)                                         \
    cell = find_cell<TQ>(kk, ax.n, q, ax.uniform, (TQ)ax.x0, (TQ)ax.inv_h);                     \
    tw = WCAST(HJB_WEIGHT(TQ, q, kk[cell], (rdx)[cell]))

// ---- the last axis' cell inside the plane window [plane0, plane0 + nplanes): a query that leaves it is clamped, `left` runs --
#define HJB_PLANE_CLAMP(cell, plane0, nplanes, left)                    \
    cell -= plane0;                                                     \
    if (cell < 0 || cell + 1 >= nplanes) {                              \
        left;                                                           \
        cell = cell < 0 ? 0 : nplanes - 2;                              \
    }

// ... as a function, where a kernel's listing allows one.  GLOBAL: the axis is read through the global address space (both pointers
// are made before the search there, as k_backup_disturb's own function made them)
template <typename T, typename TQ, bool GLOBAL>
__device__ __forceinline__ int canon_locate(const DAxis &ax, TQ q, T &tw) {
    int cell;
    if constexpr (GLOBAL) {
        const TQ *kk = (const TQ *)as_global<TQ>(ax.knots), *rdx = (const TQ *)as_global<TQ>(ax.rdx);
        HJB_LOCATE(TQ, ax, kk, rdx, q, cell, tw, (T));
    } else {
        const TQ *kk = static_cast<const TQ *>(ax.knots);
        HJB_LOCATE(TQ, ax, kk, static_cast<const TQ *>(ax.rdx), q, cell, tw, (T));
    }
    return cell;
}

// ---- the lerp cascade, axis 0 first: one axis folds 2n values into n with weight w; axes [lo, hi) of D fold with w(a) ------
#define HJB_LERP_AXIS(T, v, n, w)                                                               \
    _Pragma("unroll") for (int j_ = 0; j_ < (n); ++j_)                                          \
        v[j_] = fma_t<T>(w, (T)(v[2 * j_ + 1] - v[2 * j_]), v[2 * j_])
#define HJB_LERP_AXES(T, D, v, a, lo, hi, w)                                                    \
    _Pragma("unroll") for (int a = (lo); a < (hi); ++a) {                                       \
        HJB_LERP_AXIS(T, v, 1 << (D - 1 - a), w);                                               \
    }

// The two axis-0 neighbours of a corner in ONE load: axis 0 is contiguous in every J layout of this library (DParams::jstride[0] == 1),
// so corners 2c and 2c + 1 sit side by side - an 8-byte (float32), 4-byte (binary16) or 16-byte (float64) load at element alignment.
typedef float tab_f2u __attribute__((ext_vector_type(2), aligned(4)));
typedef _Float16 tab_h2u __attribute__((ext_vector_type(2), aligned(2)));
typedef double tab_d2u __attribute__((ext_vector_type(2), aligned(8)));
__device__ __forceinline__ void tab_load_pair(const float *__restrict__ Jn, int64_t off, float &a, float &b) {
    const tab_f2u p = *reinterpret_cast<const tab_f2u *>(Jn + off);
    a = p.x; b = p.y;
}
__device__ __forceinline__ void tab_load_pair(const _Float16 *__restrict__ Jn, int64_t off, float &a, float &b) {
    const tab_h2u p = *reinterpret_cast<const tab_h2u *>(Jn + off);
    a = (float)p.x; b = (float)p.y;
}
__device__ __forceinline__ void tab_load_pair(const double *__restrict__ Jn, int64_t off, double &a, double &b) {
    const tab_d2u p = *reinterpret_cast<const tab_d2u *>(Jn + off);
    a = p.x; b = p.y;
}

// ---- element offset of corner pair p inside a cell (axes 1 .. D-1; the pair itself is axis 0's two neighbours) -------------
#define HJB_PAIR_OFFSETS(IX, NP, D, poff, js)                           \
    IX poff[NP];                                                        \
    _Pragma("unroll") for (int p_ = 0; p_ < (NP); ++p_) {               \
        IX o_ = 0;                                                      \
        _Pragma("unroll") for (int a_ = 1; a_ < D; ++a_)                \
            if (p_ & (1 << (a_ - 1))) o_ += js[a_];                     \
        poff[p_] = o_;                                                  \
    }

// ---- owned-state index ls -> per-axis indices si[] (axis 0 fastest; the last one global: term tables are indexed by GLOBAL
// grid indices); `also` runs per axis before the slab offset is added -------------------------------------------------------
#define HJB_STATE_INDEX(D, P, ls, si, a, also)                          \
    {                                                                   \
        int64_t r_ = ls;                                                \
        _Pragma("unroll") for (int a = 0; a < D; ++a) {                 \
            int na_ = P->n[a];                                          \
            si[a] = (int)(r_ % na_);                                    \
            also;                                                       \
            r_ /= na_;                                                  \
        }                                                               \
        si[D - 1] += P->slab_begin;                                     \
    }

// ---- next control in visiting order: last control dim fastest, dim 0 slowest ----------------------------------------------
#define HJB_NEXT_CONTROL(C, cj, m1, m2)                                 \
    if (C == 1) {                                                       \
        ++cj[0];                                                        \
    } else if (C == 2) {                                                \
        if (++cj[1] == m1) { cj[1] = 0; ++cj[0]; }                      \
    } else {                                                            \
        if (++cj[2] == m2) {                                            \
            cj[2] = 0;                                                  \
            if (++cj[1] == m1) { cj[1] = 0; ++cj[0]; }                  \
        }                                                               \
    }

// ---- the column-major label (control dim 0 fastest) of per-dim control indices; WT: the type the products are formed in -----
#define HJB_LABEL_2(WT, j0, j1, m0) j0 + (WT)m0 * j1
#define HJB_LABEL_3(WT, j0, j1, j2, m0, m1) j0 + (WT)m0 * (j1 + (WT)m1 * j2)
// ... of visiting index u (dim 0 slowest); JT: the type the index is taken apart in
#define HJB_LABEL(label, JT, WT, C, u, m0, m1, m2)                      \
    if (C == 1) {                                                       \
        label = u;                                                      \
    } else if (C == 2) {                                                \
        const JT j1 = u % m1, j0 = u / m1;                              \
        label = HJB_LABEL_2(WT, j0, j1, m0);                            \
    } else {                                                            \
        const JT j2 = u % m2;                                           \
        const JT rr = u / m2;                                           \
        const JT j1 = rr % m1, j0 = rr / m1;                            \
        label = HJB_LABEL_3(WT, j0, j1, j2, m0, m1);                    \
    }
// ... from the nested kernels' pair (outer visiting index uo, innermost control j)
#define HJB_LABEL_NESTED(label, WT, C, uo, j, m0, m1)                   \
    if (C == 1) {                                                       \
        label = j;                                                      \
    } else if (C == 2) {                                                \
        label = HJB_LABEL_2(WT, uo, j, m0);                             \
    } else {                                                            \
        const int j1 = uo % m1, j0 = uo / m1;                           \
        label = HJB_LABEL_3(WT, j0, j1, j, m0, m1);                     \
    }

}  // namespace hjb
