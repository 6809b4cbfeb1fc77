// kernels_rollout_actuator.h - K33: K25's noisy closed loop (kernels_rollout_noisy.h) under ACTUATOR noise
// (hjb_rollout_run_actuator): x+ = A x + B (u (1 + eps_w)) + c (+ base_w), the node w of a finite set (eps_w, base_w, p_w) drawn per
// trajectory and step from K25's stream by K25's sampler - the model class of the control-dependent backup (K32,
// kernels_ctrldist.h), so a policy designed and priced under hjbdp.actuator_nodes can be flown under the same set.
//
// One thread per trajectory, all steps in one launch, everything in double, as K25.  Per step k:
//   1. lookup, g (on the COMMANDED u, as K32's candidate has it), J += g and the affine update acc_a: K16's own statements;
//   2. the word of step k and the node w: K25's two statements (noise_block when (k & 3) == 0, noise_node);
//   3. ue_j = u_j * eps[j][w] for every LIVE input j (an input with some eps that is not +-0): one rounded product per step;
//   4. the noise terms of axis a, in this order: B[a,j] * ue_j (the product rounded) for live j ascending with B[a,j] not +-0,
//      then base[a][w] if a is a base axis (a row of base with an entry that is not +-0).  No term: x+_a = acc_a, the axis is not
//      touched.  Otherwise n_a = the first term, n_a = n_a + term left to right, x+_a = acc_a + n_a.
//   5. paths as K25: U_path the commanded u, W_path the drawn node.
// Steps 2 - 4 are HJB_ROLLOUT_ACTUATOR_STEP below, the one statement K33 and K34 (kernels_rollout_actuator_campaign.h) fly under.
// Which terms exist is a launch constant behind wave-uniform branches: the live mask and the base mask come with the node set,
// B[a,j] != 0 from the model in effect at the run - the host forms the term mask (DActuator::terms) at every launch, so the
// kernel tests bits of one scalar where it would compare D x n_u doubles.
// The node data is one block of doubles in device memory: [T (W - 1) | eps rows of the live inputs | base rows of the base axes],
// every row node index fastest for kernels_rollout_noisy.h's bank reason: the read is per lane at its own w, and the 8-byte slots
// of one 256-byte row do not collide for W <= 32.  In the LDS form the block is staged behind the channel's tables
// (HJB_ROLLOUT_STAGE_NOISE: the record's n_tab and tab are DNoise's); the host takes the LDS form when the sum fits 32 KiB.
#pragma once
#include "hjbdp_dev.h"
#include "hjbdp_noise.h"
#include "kernels_rollout.h"
#include "kernels_rollout_noisy.h"
#include "kernels_rollout_campaign.h"

namespace hjb {

struct DActuator {
    uint64_t seed, first;             // first: first_stream + the chunk's offset in the call (the campaign: the call's)
    int32_t n_nodes, live, base_mask; // live: bit j = input j has an eps that is not +-0; base_mask: bit a = axis a has a base
    int32_t n_tab;                    // (n_nodes - 1) + n_nodes * (popcount(live) + popcount(base_mask)): the doubles at tab
    uint32_t terms, reserved_;        // bit j + HJB_ROLLOUT_MAX_U * a = input j is live and B[a,j] is not +-0 (actuator_terms, per launch)
    const double *tab;                // [T | eps rows | base rows] (global)
    double *Wp;                       // [nc, n_steps] drawn nodes, trajectory fastest, or null
};

// Steps 2 - 4, the ONE drawn-node step of K33 and K34: w_ (an int of the caller's) = the node of step k_ of the stream - K25's two
// statements - then x_[a] += n_a on the axes that have a term, at this lane's node.  x_ is the affine update's xn, u_ the
// commanded controls.  nt_ is the block [T | eps | base] and e_ its eps rows, nt_ + (n_nodes_ - 1); like seed_, stream_,
// n_nodes_, live_, bmask_ and terms_ (DActuator's masks) they are EXPRESSIONS, evaluated where they stand below; Rb_ is an
// expression for the record that holds B (a DRollout), evaluated once per axis, as HJB_ROLLOUT_AFFINE_STEP's Ra_.  `row`, `a`,
// `j`, act_n_, act_r_, noise_thr_ and noise_t_ live inside its own block.  "n_a = the first term" and "an axis with no term is
// not touched" are met without a flag: the sum starts at -0.0, and -0.0 + t = t and x + -0.0 = x hold bit for bit for every
// t and x (both signs of zero included), so no select stands between the terms.  The step CONSUMES u_: a live
// input's u_[j] becomes ue_j where it stands (no second array: with one, an instantiation kept a private segment that no
// instruction touched, and the campaign held u and ue together), so a kernel that stores the commanded u_ does so before the step.
#define HJB_ROLLOUT_ACTUATOR_STEP(D_, NU_, seed_, stream_, k_, rw_, nt_, e_, n_nodes_, live_, bmask_, terms_, Rb_, u_, x_, w_)  \
    if ((k_ & 3) == 0) noise_block(seed_, stream_, (uint32_t)k_ >> 2, rw_);                                                     \
    {                                                                                                                           \
        const int noise_thr_ = (n_nodes_) - 1;                                                                                  \
        const double *noise_t_ = nt_;                                                                                           \
        w_ = noise_node(noise_t_, noise_thr_, noise_next_word(rw_));                                                            \
        const double *row = (e_) + w_;                        /* the next row of the block, at this lane's node */              \
        _Pragma("unroll") for (int j = 0; j < NU_; ++j)                                                                         \
            if ((live_) & (1 << j)) {                                                                                           \
                u_[j] = u_[j] * row[0];                           /* ue_j, formed once, read by every axis */                   \
                row += n_nodes_;                                                                                                \
            }                                                                                                                   \
        _Pragma("unroll") for (int a = 0; a < D_; ++a) {                                                                        \
            const auto &act_r_ = Rb_;                                                                                           \
            double act_n_ = -0.0;                             /* -0.0 + t is t, bit for bit: the first term starts the sum */   \
            _Pragma("unroll") for (int j = 0; j < NU_; ++j)                                                                     \
                if ((terms_) & (1u << (j + NU_ * a))) act_n_ = act_n_ + act_r_.B[a + D_ * j] * u_[j];                           \
            if ((bmask_) & (1 << a)) {                                                                                          \
                act_n_ = act_n_ + row[0];                                                                                       \
                row += n_nodes_;                                                                                                \
            }                                                                                                                   \
            x_[a] = x_[a] + act_n_;                           /* no term: x + -0.0 is x, bit for bit - the axis is as it was */ \
        }                                                                                                                       \
    }

// what the kernel reads: one argument, so that its layout is C++'s and the record can be reread where it lies (record_reread,
// hjbdp_dev.h: K26's reason - K25, which takes its records by value, spills up to 458 scalars to vector lanes; here the
// by-value form also left one instantiation with a private segment)
struct DActuatorArgs {
    DRollout R;
    DActuator N;
    int64_t nc;
    const double *X0;                 // [D, nc]
    double *Xf, *cost, *Xp, *Up;      // as k_rollout_noisy's
};

template <int D, typename TL, int METHOD, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_actuator(const DActuatorArgs K) {
    extern __shared__ double smem[];
    const double *kn, *rd, *ut, *nt;
    HJB_ROLLOUT_PLACE(p, K.R, K.R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, K.R, kn, rd, ut)
    HJB_ROLLOUT_STAGE_NOISE(LDS, p, K.N, nt)
    if constexpr (LDS) __syncthreads();
    typedef __attribute__((address_space(4))) DActuatorArgs KArgs;
    const KArgs &K0 = *(const KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t nc = record_reread(K0).nc;
    if (i >= nc) return;
    double x[D];
    uint64_t s;
    {
        const KArgs &Kk = record_reread(K0);
        s = Kk.N.first + (uint64_t)i;
#pragma unroll
        for (int a = 0; a < D; ++a) x[a] = Kk.X0[a + (int64_t)D * i];
        if (Kk.Xp) {
#pragma unroll
            for (int a = 0; a < D; ++a) Kk.Xp[i + nc * a] = x[a];
        }
    }
    uint32_t rw[4] = {0u, 0u, 0u, 0u};
    double J = 0.0;
    for (int k = 0; k < record_reread(K0).R.n_steps; ++k) {
        const KArgs &Kl = record_reread(K0);                  // the lookup's part of the record
        const TL *__restrict__ lab = static_cast<const TL *>(Kl.R.labels);
        const int nu = Kl.R.n_u;
        const int64_t nl = Kl.R.n_labels;
        HJB_ROLLOUT_LOOKUP(D, HJB_ROLLOUT_MAX_U, METHOD, Kl.R, kn, rd, ut, lab, k, x, nu, nl, u)
        // the record again for the cost, and again for each row of A and of B (K28's rule: from D = 3 on)
        HJB_ROLLOUT_AFFINE_STEP(D, HJB_ROLLOUT_MAX_U, campaign_reread_in_step<D>(K0, Kl).R, campaign_reread_in_step<D>(K0, Kl).R, x, u, nu,
                                g, xn)
        J = J + g;
        const KArgs &Kn = campaign_reread_in_step<D>(K0, Kl); // the node set and the paths
        if (Kn.Up) {
#pragma unroll
            for (int j = 0; j < HJB_ROLLOUT_MAX_U; ++j)
                if (j < nu) Kn.Up[i + nc * (j + (int64_t)nu * k)] = u[j];
        }
        const int n_nodes = Kn.N.n_nodes;
        int w;
        HJB_ROLLOUT_ACTUATOR_STEP(D, HJB_ROLLOUT_MAX_U, Kn.N.seed, s, k, rw, nt, nt + (n_nodes - 1), n_nodes, Kn.N.live, Kn.N.base_mask,
                                  Kn.N.terms, campaign_reread_in_step<D>(K0, Kl).R, u, xn, w)
        if (Kn.N.Wp) Kn.N.Wp[i + nc * k] = (double)w;
#pragma unroll
        for (int a = 0; a < D; ++a) x[a] = xn[a];
        if (Kn.Xp) {
#pragma unroll
            for (int a = 0; a < D; ++a) Kn.Xp[i + nc * (a + (int64_t)D * (k + 1))] = x[a];
        }
    }
    const KArgs &Kk = record_reread(K0);
#pragma unroll
    for (int a = 0; a < D; ++a) Kk.Xf[a + (int64_t)D * i] = x[a];
    if (Kk.cost) Kk.cost[i] = J;
}

// The term mask of a launch: which products B[a,j] * ue_j exist, from the node set's live inputs and the model's B (host)
inline uint32_t actuator_terms(int D, int nu, int live, const double *B) {
    uint32_t terms = 0;
    for (int a = 0; a < D; ++a)
        for (int j = 0; j < nu; ++j)
            if (((live >> j) & 1) && B[a + D * j] != 0.0) terms |= 1u << (j + HJB_ROLLOUT_MAX_U * a);
    return terms;
}

// rollout_actuator.hip instantiates the 72 kernels (label type x method x LDS x D, as K25) and launches the one asked for; lds: the
// bytes of the channel's tables and the node block together
hipError_t launch_rollout_actuator(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, const DActuator &N, int64_t nc,
                                   size_t lds, hipStream_t st, const double *X0, double *Xf, double *cost, double *Xp, double *Up);

}  // namespace hjb
