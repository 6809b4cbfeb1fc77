// kernels_rollout_ctrl_lookahead.h - K35: the lookahead closed loop under a CONTROL-DEPENDENT node set
// (hjb_rollout_run_control_lookahead).  K27's loop (kernels_rollout_lookahead.h) with the control-dependent backup's E_w / max_w
// (K32, kernels_ctrldist.h) inside every candidate, flown on a nominal plant or on K33's actuator plant
// (kernels_rollout_actuator.h):
//   u_k(x) = argmin_l  g(x, u_l) + E_w[ J_{k+1}(A x + B u_l + c + e_w(l)) ]    (or max_w),
//   then  x+ = A x + B u + c   (FLY: x+ = A x + B (u (1 + eps_w')) + c + base_w', w' drawn)
// - what flies the value function K32 produces, as K27 flies K24's.
//
// One thread per trajectory, all steps in one launch, everything in double, as K27.  Per step k (hjbdp_ctrl_lookahead.h, the ONE
// statement of the arithmetic, shared with the host twin hjb_rollout_control_lookahead_host):
//   1. p = plane_of_step[k] (-1: the zero function), the state parts, and per label the candidate's g_l and xn: K26's;
//   2. per candidate l: the cell and weight of every axis OUTSIDE the mask once; per node w, in order, those of the masked axes at
//      xn_a + e[a][w][l], the N-linear blend and the combine: K27's, on candidate l's own rows;
//   3. the first minimum of g_l + acc, the chosen label applied: cost += g (on the COMMANDED u), x = xn;
//   4. U_path stored here: step 5 consumes u;
//   5. FLY only: K33's drawn-node step on the object's ACTUATOR set (HJB_ROLLOUT_ACTUATOR_STEP) - a Philox block when (k & 3) == 0,
//      w' = noise_node, ue_j = u_j eps[j][w'], x_a += the terms of axis a; the term mask is the launch's (actuator_terms);
//   6. the other paths as K27, and the drawn node per step when N.Wp is given.
// The two node blocks:
//   lookahead  [p (W) | for l: e (n_axes x W)] (L.tab), indexed by the node counter and the candidate counter only, both
//              wave-uniform: read through the constant address space into scalar registers (look_read), never per lane, never
//              staged in LDS;
//   actuator   K33's [T (W_f - 1) | eps rows | base rows] (N.tab), read per lane at the lane's own node; in the LDS form it is
//              staged behind the channel's [knots | 1/dx | u_table], and the host takes the LDS form when the sum fits 32 KiB.
// The two sets are independent: the lookahead table is what the controller believes, the actuator set is the plant.
// The argument record is reread where it lies (record_reread) per step, per candidate and per node, as K27 does and for K27's
// reason; the global form takes the actuator block from the record in the step, so no pointer to it is held across the
// candidate loop (K29's form).
#pragma once
#include "hjbdp_dev.h"
#include "hjbdp_ctrl_lookahead.h"
#include "hjbdp_noise.h"
#include "kernels_rollout_greedy.h"
#include "kernels_rollout_actuator.h"
#include "rollout_dispatch.h"

namespace hjb {

// what the kernel reads: K26's record, the per-control lookahead set and (FLY) the actuator set, as one argument
struct DCtrlLook {
    DGreedy G;
    CtrlLookSet L;                    // L.tab on the device
    DActuator N;                      // FLY: the object's actuator set, the call's seed, first stream and term mask; N.Wp or null
};

template <int D, typename TV, bool LDS, bool FLY>
__global__ void __launch_bounds__(256)
k_rollout_ctrl_lookahead(const DCtrlLook A) {
    extern __shared__ double smem[];
    const double *kn, *rd, *ut, *nt = nullptr;
    HJB_ROLLOUT_PLACE(p, A.G.R, A.G.R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, A.G.R, kn, rd, ut)
    if constexpr (FLY) {
        HJB_ROLLOUT_STAGE_NOISE(LDS, p, A.N, nt)
    }
    if constexpr (LDS) __syncthreads();
    typedef __attribute__((address_space(4))) DCtrlLook KLook;
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
            ctrl_look_step<D, TV>(A0.G.R, A0.L, kn, rd, ut, plane, x, u, g, label, best);
        }
        J = J + g;
        {
            const KLook &Au = record_reread(A0);              // the commanded u: the actuator step consumes it
            const int nu = Au.G.R.n_u;
            const int64_t nc = Au.G.nc;
            if (Au.G.Up) {
#pragma unroll
                for (int j = 0; j < HJB_ROLLOUT_MAX_U; ++j)
                    if (j < nu) Au.G.Up[i + nc * (j + (int64_t)nu * k)] = u[j];
            }
        }
        int w = 0;
        if constexpr (FLY) {
            const KLook &An = record_reread(A0);              // the actuator set; the global form takes the block from here
            const int n_nodes = An.N.n_nodes;
            const double *blk = LDS ? nt : An.N.tab;
            HJB_ROLLOUT_ACTUATOR_STEP(D, HJB_ROLLOUT_MAX_U, An.N.seed, An.N.first + (uint64_t)i, k, rw, blk, blk + (n_nodes - 1), n_nodes,
                                      An.N.live, An.N.base_mask, An.N.terms, record_reread(A0).G.R, u, x, w)
        }
        const KLook &Ak = record_reread(A0);
        const int64_t nc = Ak.G.nc;
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
// rollout_ctrl_lookahead.hip (FLY = false) and rollout_ctrl_lookahead_fly.hip (FLY = true) alone
template <bool FLY>
hipError_t launch_rollout_ctrl_lookahead_form(int val_bytes, bool lds_on, int D, const DCtrlLook &A, size_t lds, hipStream_t st) {
    const dim3 b(256), g((unsigned)((A.G.nc + 255) / 256));
    with_bool(val_bytes == 4, [&](auto f) {
        with_bool(lds_on, [&](auto l) {
            with_dim(D, [&](auto d) {
                using TV = std::conditional_t<decltype(f)::value, float, double>;
                constexpr bool LDS = decltype(l)::value;
                hipLaunchKernelGGL((k_rollout_ctrl_lookahead<decltype(d)::value, TV, LDS, FLY>), g, b, LDS ? lds : 0, st, A);
            });
        });
    });
    return hipGetLastError();
}

// val_bytes: 4 or 8; lds: the bytes of the channel's tables, and of the actuator block behind them when flown
hipError_t launch_rollout_ctrl_lookahead(int val_bytes, bool lds_on, int D, const DCtrlLook &A, size_t lds, hipStream_t st);
hipError_t launch_rollout_ctrl_lookahead_fly(int val_bytes, bool lds_on, int D, const DCtrlLook &A, size_t lds, hipStream_t st);

}  // namespace hjb
