// rollout_campaign.hip - K28's 72 instantiations (kernels_rollout_campaign.h: label type x method x LDS x D, the set K25 has) and
// the fold kernel in a unit of their own, behind launch_rollout_campaign (called by hjb_rollout_run_campaign in
// rollout_campaign_host.hip).
#include "kernels_rollout_campaign.h"
#include "rollout_dispatch.h"

namespace hjb {

// n_fold threads: thread j folds the partials of start s0 + j that lie in this launch into stats[:, s0 + j]
__global__ void __launch_bounds__(256)
k_campaign_fold(int64_t n_blocks, int64_t block0, int64_t B, int64_t s0, int64_t n_fold, const double *__restrict__ partials,
                double *__restrict__ stats) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n_fold) return;
    const int64_t s = s0 + j;
    int64_t b = s * B > block0 ? s * B : block0;
    const int64_t b_end = (s + 1) * B < block0 + n_blocks ? (s + 1) * B : block0 + n_blocks;
    const double *p = partials + 8 * (b - block0);
    double *out = stats + 8 * s;
    const double *from = out;                                 // a start continued from an earlier launch
    if (b == s * B) {                                         // its first block: acc = p_0
        from = p;
        p += 8;
        ++b;
    }
    CampVals acc = {from[0], from[1], from[2], from[3], from[7]};
    double n_exceed = from[4], n_left = from[5], n_settled = from[6];
    // unrolled so that the loads of eight blocks are in flight together: the fold itself is serial by contract, and with few starts
    // and many blocks each (8 starts x 2048 blocks) a load's latency per block is what the kernel would otherwise wait for
#pragma unroll 8
    for (; b < b_end; ++b, p += 8) {
        const CampVals o = {p[0], p[1], p[2], p[3], p[7]};
        acc = campaign_op(acc, o);
        n_exceed = n_exceed + p[4];                           // integers below 2^53: exact
        n_left = n_left + p[5];
        n_settled = n_settled + p[6];
    }
    out[0] = acc.sum;
    out[1] = acc.sumsq;
    out[2] = acc.mn;
    out[3] = acc.mx;
    out[4] = n_exceed;
    out[5] = n_left;
    out[6] = n_settled;
    out[7] = acc.sum_settled;
}

hipError_t launch_rollout_campaign(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, const DNoise &N,
                                   const DCampaign &Cp, size_t lds, hipStream_t st, const double *X0, double *stats) {
    const int64_t lanes = Cp.n_blocks * Cp.G;
    const dim3 b(256), g((unsigned)((lanes + 255) / 256));
    const DCampaignArgs K{R, N, Cp, X0};
    with_label_type(idx_bytes, [&](auto tl) {
        with_int<HJB_LOOKUP_NEAREST, HJB_LOOKUP_LINEAR>(method, [&](auto m) {
            with_bool(lds_on, [&](auto l) {
                with_dim(D, [&](auto d) {
                    using TL = typename decltype(tl)::type;
                    constexpr bool LDS = decltype(l)::value;
                    hipLaunchKernelGGL((k_rollout_campaign<decltype(d)::value, TL, decltype(m)::value, LDS>), g, b, LDS ? lds : 0, st, K);
                });
            });
        });
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_campaign_fold(Cp, st, stats);
}

hipError_t launch_campaign_fold(const DCampaign &Cp, hipStream_t st, double *stats) {
    // the starts this launch touches: block0 / B .. (block0 + n_blocks - 1) / B
    const int64_t s0 = Cp.block0 / Cp.B, n_fold = (Cp.block0 + Cp.n_blocks - 1) / Cp.B - s0 + 1;
    hipLaunchKernelGGL(k_campaign_fold, dim3((unsigned)((n_fold + 255) / 256)), dim3(256), 0, st, Cp.n_blocks, Cp.block0, Cp.B, s0, n_fold,
                       (const double *)Cp.partials, stats);
    return hipGetLastError();
}

}  // namespace hjb
