// kernels_rollout_noisy.h - K25: K16's affine closed loop (kernels_rollout.h) under sampled additive process noise
// (hjb_rollout_run_noisy): x+ = A x + B u + c + d_w, the node w of a finite set (d_w, p_w) drawn per trajectory and step from a
// counter-based stream (hjbdp_noise.h) - the model class of the disturbed backup (K24, kernels_disturb.h), so a policy designed
// and priced under a node set can be flown under the same set.
//
// One thread per trajectory, all steps in one launch, everything in double, as K16.  Per step k:
//   1. lookup, g, J += g and the affine update acc_a: K16's own statements (HJB_ROLLOUT_LOOKUP, HJB_ROLLOUT_AFFINE_STEP);
//   2. the word of step k: a Philox call when (k & 3) == 0 (a wave-uniform branch: k is the loop counter), one word per step;
//      w = the number of thresholds T[0 .. W-2] that are <= (double)word (noise_node: a binary search, <= 7 dependent reads);
//   3. x+_a = acc_a + d[a][w] for every axis a of the offset mask N.mask (the axes with an offset that is not +-0; a launch
//      constant behind wave-uniform branches, as K24's dist_axes); an axis outside the mask is not touched, not even by + 0.0;
//   4. paths as K16, and the drawn node per step (as a double) when N.Wp is given.
// Steps 2 and 3 are HJB_ROLLOUT_NOISE_STEP below, the one statement K27 - K29 fly under too.
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

// The node block's staging, the ONE every kernel that flies under noise expands (K25, K27 FLY, K28, K29), after the channel's
// HJB_ROLLOUT_STAGE: LDS_: the block copies N_.tab to HJB_ROLLOUT_PLACE_END(t_), behind channel t_'s tables, and nt_ points at
// the copy (the caller issues the __syncthreads(), as after HJB_ROLLOUT_STAGE); otherwise nt_ = N_.tab.  A macro because
// HJB_ROLLOUT_PLACE_END is one; its locals lds_n and e live inside its own block.
#define HJB_ROLLOUT_STAGE_NOISE(LDS_, t_, N_, nt_)                                                                              \
    if constexpr (LDS_) {                                                                                                       \
        double *lds_n = HJB_ROLLOUT_PLACE_END(t_);                                                                              \
        for (int e = threadIdx.x; e < N_.n_tab; e += blockDim.x) lds_n[e] = N_.tab[e];                                          \
        nt_ = lds_n;                                                                                                            \
    } else {                                                                                                                    \
        nt_ = N_.tab;                                                                                                           \
    }

// Steps 2 and 3, the ONE drawn-node step of K25, K27 (FLY), K28 and K29: w_ (an int of the caller's) = the node of step k_ of the
// stream - noise_step_node's two statements (hjbdp_noise.h, the host twins' loop) - then x_[a] += d[a][w_] on the axes of mask_,
// at this lane's node.  x_ is K25's and K28's xn, K27's and K29's x.  nt_ is the block [T | d] and d_ its offsets, nt_ +
// (n_nodes_ - 1); like seed_, stream_, n_nodes_ and mask_ they are EXPRESSIONS, evaluated where they stand below, so a kernel
// that reads them from its launch record reads them in the step (K27 - K29; K29's global form takes the block itself from
// there), and K25 passes the d it forms before the step loop.  Not calls of noise_step_node, and d_ not formed here: with
// either, the kernels' scalar loads and registers move.  `row`, `a`, noise_thr_ and noise_t_ live inside its own block.
#define HJB_ROLLOUT_NOISE_STEP(D_, seed_, stream_, k_, rw_, nt_, d_, n_nodes_, mask_, x_, w_)                                   \
    if ((k_ & 3) == 0) noise_block(seed_, stream_, (uint32_t)k_ >> 2, rw_);                                                     \
    {                                                                                                                           \
        const int noise_thr_ = (n_nodes_) - 1;                                                                                  \
        const double *noise_t_ = nt_;                                                                                           \
        w_ = noise_node(noise_t_, noise_thr_, noise_next_word(rw_));                                                            \
        const double *row = (d_) + w_;                        /* the next masked axis' offsets, at this lane's node */          \
        _Pragma("unroll") for (int a = 0; a < D_; ++a)                                                                          \
            if ((mask_) & (1 << a)) {                                                                                           \
                x_[a] = x_[a] + row[0];                                                                                         \
                row += n_nodes_;                                                                                                \
            }                                                                                                                   \
    }

template <int D, typename TL, int METHOD, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_noisy(const DRollout R, const DNoise N, int64_t nc, const double *__restrict__ X0, double *__restrict__ Xf,
                double *__restrict__ cost, double *__restrict__ Xp, double *__restrict__ Up) {
    extern __shared__ double smem[];
    const double *kn, *rd, *ut, *nt;
    HJB_ROLLOUT_PLACE(p, R, R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, R, kn, rd, ut)
    HJB_ROLLOUT_STAGE_NOISE(LDS, p, N, nt)
    if constexpr (LDS) __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const TL *__restrict__ lab = static_cast<const TL *>(R.labels);
    const int nu = R.n_u;
    const int64_t nl = R.n_labels;
    const double *off = nt + (N.n_nodes - 1);
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
        HJB_ROLLOUT_AFFINE_STEP(D, HJB_ROLLOUT_MAX_U, R, R, x, u, nu, g, xn)
        J = J + g;
        int w;
        HJB_ROLLOUT_NOISE_STEP(D, N.seed, s, k, rw, nt, off, N.n_nodes, N.mask, xn, w)
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
