// kernels_rollout_lookahead.h - K27: the disturbance-aware greedy closed loop (hjb_rollout_run_lookahead).  K26's loop
// (kernels_rollout_greedy.h) with the disturbed backup's E_w / max_w (K24, kernels_disturb.h) inside every candidate, flown on a
// nominal plant or under K25's sampled noise (kernels_rollout_noisy.h):
//   u_k(x) = argmin_l  g(x, u_l) + E_w[ J_{k+1}(A x + B u_l + c + e_w) ]    (or max_w),   then  x+ = A x + B u + c (+ d_w', drawn)
//
// One thread per trajectory, all steps in one launch, everything in double, as K16.  Per step k (hjbdp_lookahead.h, the ONE
// statement of the arithmetic, shared with the host twin hjb_rollout_lookahead_host):
//   1. p = plane_of_step[k] (-1: the zero function), the state parts, and per label the candidate's g_l and xn: K26's;
//   2. per candidate: the cell and weight of every axis OUTSIDE the lookahead mask once; per node w, in order, those of the masked
//      axes at xn_a + e[a][w], the N-linear blend (K26's tree in K26's corner groups) and the combine (p_0 v_0 then fma / first max);
//   3. the first minimum of g_l + acc, the chosen label applied: cost += g, x = xn;
//   4. FLY only: K25's steps 2-3 on the object's flight set (HJB_ROLLOUT_NOISE_STEP) - a Philox block when (k & 3) == 0, w' =
//      noise_node, x_a += d[a][w'] on the flight mask alone;
//   5. paths as K26, and the drawn node per step when N.Wp is given.
// The two node blocks:
//   lookahead  [p (W) | e (n_axes x W)] (L.tab), indexed by the node counter only: read through the constant address space into
//              scalar registers (look_read), never per lane, never staged in LDS;
//   flight     K25's [T (W_f - 1) | d (W_f x n_axes_f)] (N.tab), read per lane at the lane's own node; in the LDS form it is staged
//              behind the channel's [knots | 1/dx | u_table], and the host takes the LDS form when the sum fits 32 KiB.
// The argument record is read where it lies, in the argument segment, through record_reread (K26's reason: held in scalar
// registers across three nested loops it would be spilled): per step, per candidate and, inside the node loop, once per node at
// D = 1 and 2 (held across the candidate loop, or across one candidate's nodes, D = 2 spills 5 - 72 scalars) and per loop body
// from D = 3 on, as K26.
#pragma once
#include "hjbdp_dev.h"
#include "hjbdp_lookahead.h"
#include "hjbdp_noise.h"
#include "kernels_rollout_greedy.h"
#include "kernels_rollout_noisy.h"
#include "rollout_dispatch.h"

namespace hjb {

// what the kernel reads: K26's record, the lookahead set and (FLY) the flight set, as one argument
struct DLook {
    DGreedy G;
    LookSet L;                        // L.tab on the device
    DNoise N;                         // FLY: the object's noise set, seed and first stream; N.Wp [nc, n_steps] or null
};

template <int D, typename TV, bool LDS, bool FLY>
__global__ void __launch_bounds__(256)
k_rollout_lookahead(const DLook A) {
    extern __shared__ double smem[];
    const double *kn, *rd, *ut, *nt = nullptr;
    HJB_ROLLOUT_PLACE(p, A.G.R, A.G.R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, A.G.R, kn, rd, ut)
    if constexpr (FLY) {
        HJB_ROLLOUT_STAGE_NOISE(LDS, p, A.N, nt)
    }
    if constexpr (LDS) __syncthreads();
    typedef __attribute__((address_space(4))) DLook KLook;
    const KLook &A0 = *(const KLook *)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= A0.G.nc) return;
    double x[D];
    {
        const KLook &Ak = record_reread(A0);
        const int64_t nc = Ak.G.nc;
#pragma unroll
        for (int a = 0; a < D; ++a) x[a] = Ak.G.X0[a + (int64_t)D * i];
        if (Ak.G.Xp) {
#pragma unroll
            for (int a = 0; a < D; ++a) Ak.G.Xp[i + nc * a] = x[a];
        }
    }
    uint32_t rw[4] = {0u, 0u, 0u, 0u};
    double J = 0.0;
    for (int k = 0; k < record_reread(A0).G.R.n_steps; ++k) {
        double u[HJB_ROLLOUT_MAX_U], g, best;
        int label;
        {
            const KLook &Ak = record_reread(A0);
            const int32_t p = Ak.G.R.plane_of_step[k];
            const TV *plane = p < 0 ? nullptr : static_cast<const TV *>(Ak.G.values) + (int64_t)p * Ak.G.R.nS;
            look_step<D, TV>(A0.G.R, A0.L, kn, rd, ut, plane, x, u, g, label, best);
        }
        J = J + g;
        int w = 0;
        if constexpr (FLY) {
            const KLook &Ak = record_reread(A0);
            HJB_ROLLOUT_NOISE_STEP(D, Ak.N.seed, Ak.N.first + (uint64_t)i, k, rw, nt, nt + (Ak.N.n_nodes - 1), Ak.N.n_nodes,
                                   Ak.N.mask, x, w)
        }
        const KLook &Ak = record_reread(A0);
        const int nu = Ak.G.R.n_u;
        const int64_t nc = Ak.G.nc;
        if (Ak.G.Up) {
#pragma unroll
            for (int j = 0; j < HJB_ROLLOUT_MAX_U; ++j)
                if (j < nu) Ak.G.Up[i + nc * (j + (int64_t)nu * k)] = u[j];
        }
        if (Ak.G.Lp) Ak.G.Lp[i + nc * k] = (double)(label + Ak.G.R.index_base);
        if (Ak.G.Vp) Ak.G.Vp[i + nc * k] = best;
        if constexpr (FLY) {
            if (Ak.N.Wp) Ak.N.Wp[i + nc * k] = (double)w;
        }
        if (Ak.G.Xp) {
#pragma unroll
            for (int a = 0; a < D; ++a) Ak.G.Xp[i + nc * (a + (int64_t)D * (k + 1))] = x[a];
        }
    }
    const KLook &Ak = record_reread(A0);
#pragma unroll
    for (int a = 0; a < D; ++a) Ak.G.Xf[a + (int64_t)D * i] = x[a];
    if (Ak.G.cost) Ak.G.cost[i] = J;
}

// the 24 instantiations of one FLY (D x value type x LDS) and the launch of the one asked for: instantiated by
// rollout_lookahead.hip (FLY = false) and rollout_lookahead_fly.hip (FLY = true) alone
template <bool FLY>
hipError_t launch_rollout_lookahead_form(int val_bytes, bool lds_on, int D, const DLook &A, size_t lds, hipStream_t st) {
    const dim3 b(256), g((unsigned)((A.G.nc + 255) / 256));
    with_bool(val_bytes == 4, [&](auto f) {
        with_bool(lds_on, [&](auto l) {
            with_dim(D, [&](auto d) {
                using TV = std::conditional_t<decltype(f)::value, float, double>;
                constexpr bool LDS = decltype(l)::value;
                hipLaunchKernelGGL((k_rollout_lookahead<decltype(d)::value, TV, LDS, FLY>), g, b, LDS ? lds : 0, st, A);
            });
        });
    });
    return hipGetLastError();
}

// val_bytes: 4 or 8; lds: the bytes of the channel's tables, and of the flight block behind them when fly
hipError_t launch_rollout_lookahead(int val_bytes, bool lds_on, int D, const DLook &A, size_t lds, hipStream_t st);
hipError_t launch_rollout_lookahead_fly(int val_bytes, bool lds_on, int D, const DLook &A, size_t lds, hipStream_t st);

}  // namespace hjb
