// kernels_rollout_noisy.h - K25: K16's affine closed loop (kernels_rollout.h) under sampled additive process noise
// (hjb_rollout_run_noisy): x+ = A x + B u + c + d_w, the node w of a finite set (d_w, p_w) drawn per trajectory and step from a
// counter-based stream (hjbdp_noise.h) - the model class of the disturbed backup (K24, kernels_disturb.h), so a policy designed
// and priced under a node set can be flown under the same set.
//
// One thread per trajectory, all steps in one launch, everything in double, as K16.  Per step k:
//   1. lookup, g, J += g and the affine update acc_a: K16's operations in K16's order (HJB_ROLLOUT_LOOKUP and the same loops);
//   2. the word of step k: a Philox call when (k & 3) == 0 (a wave-uniform branch: k is the loop counter), one word per step;
//      w = the number of thresholds T[0 .. W-2] that are <= (double)word (noise_node: a binary search, <= 7 dependent reads);
//   3. x+_a = acc_a + d[a][w] for every axis a of the offset mask N.mask (the axes with an offset that is not +-0; a launch
//      constant behind wave-uniform branches, as K24's dist_axes); an axis outside the mask is not touched, not even by + 0.0;
//   4. paths as K16, and the drawn node per step (as a double) when N.Wp is given.
// The node data is one block of doubles in device memory: [T (W - 1) | d (W x n_axes, node index fastest: row j = the j-th masked
// axis)].  Node index fastest because the read is per lane at its own w: lanes of a 32-lane half that drew different nodes hit
// different 8-byte slots of the 256-byte bank row for W <= 32 (equal nodes broadcast), and at most ceil(W / 32) of them share a
// slot beyond that; with the axes fastest an even n_axes would put nodes w and w + 16 on one slot.  In the LDS form the block is
// staged behind the channel's [knots | 1/dx | u_table]; the host takes the LDS form when the sum fits 32 KiB.
// The stream of trajectory i of the launch is N.first + i: the host adds the chunk's offset, so streams count through the call.
#pragma once
#include "hjbdp_dev.h"
#include "hjbdp_noise.h"
#include "kernels_rollout.h"

namespace hjb {

struct DNoise {
    uint64_t seed, first;             // first: first_stream + the chunk's offset in the call
    int32_t n_nodes, mask, n_axes;    // n_axes = popcount(mask)
    int32_t n_tab;                    // (n_nodes - 1) + n_nodes * n_axes: the doubles at tab
    const double *tab;                // [T | d] (global)
    double *Wp;                       // [nc, n_steps] drawn nodes, trajectory fastest, or null
};

template <int D, typename TL, int METHOD, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_noisy(const DRollout R, const DNoise N, int64_t nc, const double *__restrict__ X0, double *__restrict__ Xf,
                double *__restrict__ cost, double *__restrict__ Xp, double *__restrict__ Up) {
    extern __shared__ double smem[];
    const double *kn, *rd, *ut, *nt;
    HJB_ROLLOUT_PLACE(p, R, R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, R, kn, rd, ut)
    if constexpr (LDS) {
        double *lds_n = HJB_ROLLOUT_PLACE_END(p);
        for (int e = threadIdx.x; e < N.n_tab; e += blockDim.x) lds_n[e] = N.tab[e];
        nt = lds_n;
        __syncthreads();
    } else {
        nt = N.tab;
    }
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const TL *__restrict__ lab = static_cast<const TL *>(R.labels);
    const int nu = R.n_u;
    const int64_t nl = R.n_labels;
    const int n_thr = N.n_nodes - 1;
    const double *off = nt + n_thr;
    const uint64_t s = N.first + (uint64_t)i;
    uint32_t rw[4] = {0u, 0u, 0u, 0u};
    double x[D];
#pragma unroll
    for (int a = 0; a < D; ++a) x[a] = X0[a + (int64_t)D * i];
    if (Xp) {
#pragma unroll
        for (int a = 0; a < D; ++a) Xp[i + nc * a] = x[a];
    }
    double J = 0.0;
    for (int k = 0; k < R.n_steps; ++k) {
        HJB_ROLLOUT_LOOKUP(D, HJB_ROLLOUT_MAX_U, METHOD, R, kn, rd, ut, lab, k, x, nu, nl, u)
        double g = R.q[0] * (x[0] * x[0]);
#pragma unroll
        for (int a = 1; a < D; ++a) g = g + R.q[a] * (x[a] * x[a]);
#pragma unroll
        for (int j = 0; j < HJB_ROLLOUT_MAX_U; ++j)
            if (j < nu) g = g + R.r[j] * (u[j] * u[j]);
        J = J + g;
        double xn[D];
#pragma unroll
        for (int a = 0; a < D; ++a) {
            double acc = R.A[a] * x[0];
#pragma unroll
            for (int b = 1; b < D; ++b) acc = acc + R.A[a + D * b] * x[b];
#pragma unroll
            for (int j = 0; j < HJB_ROLLOUT_MAX_U; ++j)
                if (j < nu) acc = acc + R.B[a + D * j] * u[j];
            if (R.has_c) acc = acc + R.c[a];
            xn[a] = acc;
        }
        if ((k & 3) == 0) noise_block(N.seed, s, (uint32_t)k >> 2, rw);
        const int w = noise_node(nt, n_thr, noise_next_word(rw));
        {
            const double *row = off + w;                  // the next masked axis' offsets, at this lane's node
#pragma unroll
            for (int a = 0; a < D; ++a)
                if (N.mask & (1 << a)) {
                    xn[a] = xn[a] + row[0];
                    row += N.n_nodes;
                }
        }
        if (Up) {
#pragma unroll
            for (int j = 0; j < HJB_ROLLOUT_MAX_U; ++j)
                if (j < nu) Up[i + nc * (j + (int64_t)nu * k)] = u[j];
        }
        if (N.Wp) N.Wp[i + nc * k] = (double)w;
#pragma unroll
        for (int a = 0; a < D; ++a) x[a] = xn[a];
        if (Xp) {
#pragma unroll
            for (int a = 0; a < D; ++a) Xp[i + nc * (a + (int64_t)D * (k + 1))] = x[a];
        }
    }
#pragma unroll
    for (int a = 0; a < D; ++a) Xf[a + (int64_t)D * i] = x[a];
    if (cost) cost[i] = J;
}

// rollout_noisy.hip instantiates the 72 kernels (label type x method x LDS x D, as K16) and launches the one asked for; lds: the
// bytes of the channel's tables and the node block together
hipError_t launch_rollout_noisy(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, const DNoise &N, int64_t nc,
                                size_t lds, hipStream_t st, const double *X0, double *Xf, double *cost, double *Xp, double *Up);

}  // namespace hjb
