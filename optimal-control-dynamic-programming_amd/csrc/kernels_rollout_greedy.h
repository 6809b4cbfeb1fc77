// kernels_rollout_greedy.h - K26: the greedy closed loop (hjb_rollout_run_greedy).  K16's affine model (kernels_rollout.h) flown
// by one-step lookahead on a stored cost-to-go instead of stored labels:
//   u_k(x) = argmin_l  g(x, u_l) + J_{k+1}(A x + B u_l + c)   over the rows u_l of the object's u_table, at the state visited.
//
// One thread per trajectory, all steps in one launch, everything in double, as K16.  Per step k (hjbdp_greedy.h, the ONE
// statement of the arithmetic, shared with the host twin hjb_rollout_greedy_host):
//   1. p = plane_of_step[k]: a plane of the object's values [nS, n_planes] (TV = float or double, widened exactly on read), or
//      -1 for the zero function (v = +0.0 for every candidate, nothing read); wave-uniform, k is the loop counter;
//   2. the state parts gs and as_a once, outside the candidate loop;
//   3. per label l in order: g_l and xn (K16's g and x+), v_l = the N-linear blend of plane p at xn (exact cell search clamped
//      to [0, n - 2], t = (xn - k[c]) * rdx[c], depth-first pairwise fma tree: hjb_policy_lookup 'linear' in double, bit for bit),
//      cand_l = g_l + v_l; the first minimum wins, a NaN candidate never replaces;
//   4. the chosen label applied: cost += g, x = xn (formed again from the same operands: the same bits);
//   5. paths as K16, and per step the chosen label + index_base (as a double, G.Lp) and the minimum itself (G.Vp).
// Knots, 1/dx and u_table are staged in LDS when they fit (LDS = true: K16's staging and K16's rule); value planes stay in global
// memory: one plane of a reference-sized grid is L2-resident and the lanes of a wave gather from different cells.  The corners of
// a candidate are read in groups (all 2^D up to D = 4, 16 at a time beyond), so no instantiation holds 2^D values and none has a
// private segment.  Offsets are int64 throughout; stores are plain, trajectory index fastest.
#pragma once
#include "hjbdp_dev.h"
#include "hjbdp_greedy.h"
#include "kernels_rollout.h"

namespace hjb {

// what the kernel reads beside the policy object's record: one argument, so that its layout is C++'s
struct DGreedy {
    DRollout R;
    const void *values;               // [nS, n_planes] column-major, TV (global); null when every plane of the run is -1
    int64_t nc;                       // trajectories of the launch
    const double *X0;                 // [D, nc]
    double *Xf, *cost, *Xp, *Up;      // as K16's
    double *Lp, *Vp;                  // [nc, n_steps] chosen label + index_base / the minimum, trajectory fastest, or null
};

// The kernel reads its argument where it lies, in the argument segment, through record_reread (hjbdp_dev.h): the model per
// step and, from D = 3 on, per loop body of the candidate loop; the output pointers where a step stores.  Held in scalar
// registers across the candidate loop, as a by-value argument is, the record and the loop's own scalars exceed the register file
// from D = 2 on and the compiler spills them (to lanes of a vector register; at D = 5 and 6 it also reserved a private segment).
// G itself is only used for the staging.
template <int D, typename TV, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_greedy(const DGreedy G) {
    extern __shared__ double smem[];
    const double *kn, *rd, *ut;
    HJB_ROLLOUT_PLACE(p, G.R, G.R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, G.R, kn, rd, ut)
    if constexpr (LDS) __syncthreads();
    typedef __attribute__((address_space(4))) DGreedy KGreedy;
    const KGreedy &G0 = *(const KGreedy *)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= G0.nc) return;
    double x[D];
    {
        const KGreedy &Gk = record_reread(G0);
        const int64_t nc = Gk.nc;
#pragma unroll
        for (int a = 0; a < D; ++a) x[a] = Gk.X0[a + (int64_t)D * i];
        if (Gk.Xp) {
#pragma unroll
            for (int a = 0; a < D; ++a) Gk.Xp[i + nc * a] = x[a];
        }
    }
    double J = 0.0;
    for (int k = 0; k < record_reread(G0).R.n_steps; ++k) {
        double u[HJB_ROLLOUT_MAX_U], g, best;
        int label;
        {
            const KGreedy &Gk = record_reread(G0);
            const int32_t p = Gk.R.plane_of_step[k];
            const TV *plane = p < 0 ? nullptr : static_cast<const TV *>(Gk.values) + (int64_t)p * Gk.R.nS;
            greedy_step<D, TV>(G0.R, kn, rd, ut, plane, x, u, g, label, best);
        }
        J = J + g;
        const KGreedy &Gk = record_reread(G0);
        const int nu = Gk.R.n_u;
        const int64_t nc = Gk.nc;
        if (Gk.Up) {
#pragma unroll
            for (int j = 0; j < HJB_ROLLOUT_MAX_U; ++j)
                if (j < nu) Gk.Up[i + nc * (j + (int64_t)nu * k)] = u[j];
        }
        if (Gk.Lp) Gk.Lp[i + nc * k] = (double)(label + Gk.R.index_base);
        if (Gk.Vp) Gk.Vp[i + nc * k] = best;
        if (Gk.Xp) {
#pragma unroll
            for (int a = 0; a < D; ++a) Gk.Xp[i + nc * (a + (int64_t)D * (k + 1))] = x[a];
        }
    }
    const KGreedy &Gk = record_reread(G0);
#pragma unroll
    for (int a = 0; a < D; ++a) Gk.Xf[a + (int64_t)D * i] = x[a];
    if (Gk.cost) Gk.cost[i] = J;
}

// rollout_greedy.hip instantiates the 24 kernels (D x value type x LDS) and launches the one asked for; val_bytes: 4 or 8
hipError_t launch_rollout_greedy(int val_bytes, bool lds_on, int D, const DGreedy &G, size_t lds, hipStream_t st);

}  // namespace hjb
