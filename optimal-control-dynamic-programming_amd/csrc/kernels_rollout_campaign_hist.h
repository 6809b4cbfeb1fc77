// kernels_rollout_campaign_hist.h - K30: K28's campaign (kernels_rollout_campaign.h) with a per-start histogram of the costs beside
// the eight statistics (hjb_rollout_run_campaign_hist; the bin rule: campaign_bin, hjbdp_campaign.h).  k_rollout_campaign_hist is
// K28's flight (kernels_rollout_campaign_body.inc, the same text) and K28's block partial, unchanged - the statistics are the
// plain call's bits - plus, between the two, the count of every live lane's cost into hist [n_bins + 2, n_starts] int64 on the
// device, zeroed once per call on the call's stream and accumulated across launches.  Padding slots and lanes past the launch's
// last block count nothing.  No array has a dimension of n_starts * M.
//
// The counts are integers and integer addition commutes, so they are accumulated with atomics (hjbdp_campaign.h says why that
// breaks no rule and how far the licence goes).  The form is decided once, on the host (campaign_hist_form, below):
//   wave form (G == 64: a wave is exactly one block of one start, a workgroup four consecutive blocks)  a private histogram per
//       wave in LDS, 4 x (n_bins + 2) uint32 behind the tables, zeroed by the workgroup, counted with 32-bit LDS atomics - a
//       workgroup adds at most 256, nothing overflows - and after a barrier flushed by bin: thread j adds bin j of the waves of
//       one start together first, then makes one 64-bit global atomic add per start of the workgroup and non-zero sum.  With few
//       starts and many samples every workgroup would otherwise hit the same n_bins + 2 global counters 256 times;
//   direct form (G < 64: a start has at most 32 samples)  one 64-bit global atomic add per live lane: nothing contends.
// The count comes after the step loop, from the slot value v.mn (= c in a live lane, before the tree): nothing of it is live
// across the flight.
#pragma once
#include "kernels_rollout_campaign.h"

namespace hjb {

struct DCampHist {
    const double *range;              // [3, n_starts] (global): lo, hi and scale of every start
    unsigned long long *hist;         // [n_bins + 2, n_starts] (global), int64 counts
    int32_t n_bins;
    int32_t wave_form;                // 1: a private histogram per wave in LDS (G == 64); 0: direct global atomics
    int32_t lds_off;                  // wave form: bytes from the start of the dynamic LDS to the wave histograms (a multiple of 8)
    int32_t reserved_;
};

constexpr int kCampHistWaves = 4;     // waves of a campaign kernel's workgroup (256 lanes)

// The ONE place the accumulation form and its LDS are decided (host): wave form iff G == 64; its bytes count with the tables'
// bytes `lds_tables` against `lds_max` where the tables' placement is decided.  Returns the launch's dynamic LDS bytes.
inline size_t campaign_hist_form(int G, int n_bins, bool lds_option, size_t lds_tables, size_t lds_max, bool *lds_on, DCampHist *H) {
    H->n_bins = n_bins;
    H->wave_form = G == kCampaignMaxGroup ? 1 : 0;
    const size_t hb = H->wave_form ? (size_t)kCampHistWaves * (size_t)(n_bins + 2) * sizeof(uint32_t) : 0;
    *lds_on = lds_option && lds_tables + hb <= lds_max;
    H->lds_off = (int32_t)(*lds_on ? lds_tables : 0);
    return (*lds_on ? lds_tables : 0) + hb;
}

// The count of one lane's cost c (read only where live), by every lane of the workgroup: C the launch's DCampaign, s the lane's
// start.  The wave form's barriers are uniform: H.wave_form is the launch's.
template <typename HIST, typename CAMP>
__device__ __forceinline__ void campaign_hist_count(const HIST &H, const CAMP &C, double *smem, bool live, double c, int64_t s) {
    const int nb2 = H.n_bins + 2;
    int bin = 0;
    if (live) {
        const double *r = H.range + 3 * s;
        bin = campaign_bin(c, r[0], r[1], r[2], H.n_bins);
    }
    if (H.wave_form) {
        uint32_t *wh = (uint32_t *)((char *)smem + H.lds_off);
        for (int j = threadIdx.x; j < kCampHistWaves * nb2; j += 256) wh[j] = 0u;
        __syncthreads();
        if (live) atomicAdd(&wh[(int)(threadIdx.x >> 6) * nb2 + bin], 1u);
        __syncthreads();
        // wave w of the workgroup is block 4 * blockIdx.x + w of the launch; consecutive blocks of one start merge first
        const int64_t lb0 = (int64_t)blockIdx.x * kCampHistWaves;
        for (int j = threadIdx.x; j < nb2; j += 256) {
            unsigned long long run = 0ull;
            int64_t s_run = 0;
            for (int w = 0; w < kCampHistWaves && lb0 + w < C.n_blocks; ++w) {
                const int64_t sw = (C.block0 + lb0 + w) / C.B;
                if (sw != s_run) {
                    if (run) atomicAdd(H.hist + (j + (int64_t)nb2 * s_run), run);
                    run = 0ull;
                    s_run = sw;
                }
                run += wh[w * nb2 + j];
            }
            if (run) atomicAdd(H.hist + (j + (int64_t)nb2 * s_run), run);
        }
    } else if (live) {
        atomicAdd(H.hist + (bin + (int64_t)nb2 * s), 1ull);
    }
}

// what the kernel reads: K28's record first, where K28's flight rereads it, then the histogram's
struct DCampaignHistArgs {
    DCampaignArgs A;
    DCampHist H;
};

template <int D, typename TL, int METHOD, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_campaign_hist(const DCampaignHistArgs KH) {
    const DCampaignArgs &K = KH.A;
#include "kernels_rollout_campaign_body.inc"
    // every lane of the wave from here on: the count of the lane's cost (v.mn = c in a live lane), then K28's block partial
    {
        typedef __attribute__((address_space(4))) DCampaignHistArgs KHArgs;
        const KHArgs &KH0 = *(const KHArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        campaign_hist_count(record_reread(KH0).H, record_reread(K0).C, smem, live, v.mn, s);
    }
    HJB_CAMPAIGN_BLOCK_PARTIAL(v, f_exceed, f_left, f_settled, G, slot, lb, record_reread(K0).C)
}

// rollout_campaign_hist.hip instantiates the 72 kernels (K28's set) and launches the one asked for, then K28's fold; lds: the
// launch's dynamic LDS bytes (campaign_hist_form)
hipError_t launch_rollout_campaign_hist(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, const DNoise &N,
                                        const DCampaign &Cp, const DCampHist &H, size_t lds, hipStream_t st, const double *X0,
                                        double *stats);

}  // namespace hjb
