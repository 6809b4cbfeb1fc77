// hjbdp_noise.h - the random stream and the node sampler of the noisy rollouts (K25, kernels_rollout_noisy.h), shared by the kernel
// and its host twins hjb_rollout_noise_table / hjb_rollout_noise_draw (rollout.hip).  No HIP dependency: tests/noise_harness.cpp
// compiles it as plain C++.  The contract (stated verbatim in include/hjbdp.h):
//   generator   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers
//               0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds;
//   addressing  counter-based, no state between calls: the stream of a trajectory is s = first_stream + i (uint64; i its index in
//               the CALL, not in the chunk); step k reads word k & 3 of
//               Philox(counter = (lo32 s, hi32 s, k >> 2, 0), key = (lo32 seed, hi32 seed)) - one Philox call per four steps;
//   thresholds  W - 1 doubles T[w] = floor(2^32 * (S_w / S_{W-1})), S_w = p_0 + .. + p_w summed left to right in double (null
//               weights: p_w = 1.0 each); the drawn node is the number of w in [0, W-2] with T[w] <= (double)word.
// Doubles keep T = 2^32 representable, so a trailing zero-weight node is never drawn; a zero-weight node anywhere has
// T[w] == T[w-1] (or T[0] == 0) and is never drawn either; W = 1 draws node 0.  Probabilities resolve to 2^-32: a node of weight
// below 2^-32 of the total may never be drawn, and every node's frequency is its weight rounded to a multiple of 2^-32.
// The multiplies are 32 x 32 -> 64 (quarter rate): 40 per four steps next to a step of several hundred vector instructions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HJB_NOISE_FN __host__ __device__ __forceinline__
#else
#define HJB_NOISE_FN inline
#endif

namespace hjb {

// Philox4x32-10 in place: c = the counter on entry, the four output words on return.
// The rounds stay a loop of ten trips (unroll 1): unrolled into the step loop of K25, the register allocation of the D = 3
// global-memory 'linear' kernels reserves a private segment (a spill slot no instruction touches); the loop costs nothing measurable
HJB_NOISE_FN void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll 1
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1;
        c[3] = (uint32_t)p0;
        c[0] = n0;
        c[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// the four words steps 4 * block .. 4 * block + 3 of stream s read
HJB_NOISE_FN void noise_block(uint64_t seed, uint64_t s, uint32_t block, uint32_t (&r)[4]) {
    r[0] = (uint32_t)s;
    r[1] = (uint32_t)(s >> 32);
    r[2] = block;
    r[3] = 0u;
    philox4x32_10(r, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// The word of the step at hand and the shift that brings the next step's to the front: a kernel that calls noise_block when
// (k & 3) == 0 and this once per step reads word k & 3 at step k, without indexing registers by k.
HJB_NOISE_FN uint32_t noise_next_word(uint32_t (&r)[4]) {
    const uint32_t w = r[0];
    r[0] = r[1];
    r[1] = r[2];
    r[2] = r[3];
    return w;
}

// The drawn node: the number of w in [0, n_thr) with T[w] <= (double)word, n_thr = W - 1.  T is non-decreasing (cumulative sums of
// non-negative weights), so the count is where a binary search ends: at most 7 dependent reads for W <= 128, none for W = 1.
HJB_NOISE_FN int noise_node(const double *T, int n_thr, uint32_t word) {
    const double x = (double)word;
    int step = 1;
    while (2 * step <= n_thr) step *= 2;
    int lo = 0;
    for (; step > 0; step >>= 1)
        if (lo + step <= n_thr && T[lo + step - 1] <= x) lo += step;
    return lo;
}

// The node of step k of a stream, the ONE loop body of the host twins (hjb_rollout_noise_draw, hjb_rollout_lookahead_campaign_host):
// called for k = 0, 1, 2, ... in order with one r per stream, it makes a Philox call when (k & 3) == 0 and takes one word per
// step.  The kernels' step (HJB_ROLLOUT_NOISE_STEP, kernels_rollout_noisy.h) is these two statements expanded in place, with its
// arguments read inside the branch: as a call of this function, every noisy kernel's code object changed.
HJB_NOISE_FN int noise_step_node(uint64_t seed, uint64_t s, int k, uint32_t (&r)[4], const double *T, int n_thr) {
    if ((k & 3) == 0) noise_block(seed, s, (uint32_t)k >> 2, r);
    return noise_node(T, n_thr, noise_next_word(r));
}

// The thresholds of n_nodes weights (null: 1.0 each) into T[0 .. n_nodes - 2].  Returns the weights' sum S_{W-1}; the caller has
// checked that every weight is finite and non-negative and refuses a sum of 0.
inline double noise_table(int n_nodes, const double *weights, double *T) {
    double total = 0.0;
    for (int w = 0; w < n_nodes; ++w) total = total + (weights ? weights[w] : 1.0);
    double S = 0.0;
    for (int w = 0; w + 1 < n_nodes; ++w) {
        S = S + (weights ? weights[w] : 1.0);
        const double t = 4294967296.0 * (S / total);
        T[w] = (double)(uint64_t)t;                  // floor: 0 <= t <= 2^32
    }
    return total;
}

}  // namespace hjb
