// rollout_campaign_host.hip - hjb_rollout_run_campaign and hjb_rollout_campaign_reduce (include/hjbdp.h): the host side of the
// noisy campaigns (K28, kernels_rollout_campaign.h / rollout_campaign.hip).  The run function makes hjb_rollout_run_noisy's
// refusals (rollout_host.h: check_run, check_traj) and its own before any device work, uploads X0 and the thresholds once per call
// (upload), and walks the call's block list in launches of at most option "chunk" lanes.  run_chunks is not used: its record and
// its transfers are per trajectory, which is what a campaign does away with.  What a call holds on the device is
// [D + 1 + 8, n_starts] doubles and 8 doubles per block of a launch; nothing has a dimension of n_starts * n_samples.
// The host reduce runs hjbdp_campaign.h's functions in a plain loop, with no device.  No kernel is instantiated in this unit.
#include "rollout_host.h"
#include "kernels_rollout_campaign.h"

using namespace hjbhost;

namespace hjbhost {

// What the campaigns' entry points refuse of their sizes, in `who`'s name: n_samples < 1, n_starts * n_samples overflowing
int check_campaign_sizes(Rollout *ro, const char *who, int64_t n_starts, int64_t n_samples) {
    if (n_samples < 1) return rfail(ro, HJB_E_INVALID, "%s: n_samples=%lld < 1", who, (long long)n_samples);
    if (n_starts > 0 && n_samples > INT64_MAX / n_starts)
        return rfail(ro, HJB_E_INVALID, "%s: n_starts * n_samples overflows (%lld x %lld)", who, (long long)n_starts, (long long)n_samples);
    return HJB_OK;
}

// ... and of its bounds: a NaN threshold, a NaN or negative tol (n_starts >= 0 and D are the caller's)
int check_campaign_bounds(Rollout *ro, const char *who, int D, int64_t n_starts, const double *threshold, const double *tol) {
    for (int64_t s = 0; threshold && s < n_starts; ++s)
        if (threshold[s] != threshold[s]) return rfail(ro, HJB_E_INVALID, "%s: threshold[%lld] is NaN", who, (long long)s);
    for (int a = 0; tol && a < D; ++a)
        if (!(tol[a] >= 0)) return rfail(ro, HJB_E_INVALID, "%s: tol[%d] = %g is NaN or negative", who, a, tol[a]);
    return HJB_OK;
}

// ... and of its streams, with the sizes first: what a run function refuses before it needs an object
int check_campaign_streams(Rollout *ro, const char *who, int64_t n_starts, int64_t n_samples, int64_t first_stream) {
    if (first_stream < 0) return rfail(ro, HJB_E_INVALID, "%s: first_stream=%lld < 0", who, (long long)first_stream);
    if (const int bad = check_campaign_sizes(ro, who, n_starts, n_samples)) return bad;
    if (n_starts > 0 && first_stream > INT64_MAX - n_starts * n_samples)
        return rfail(ro, HJB_E_INVALID, "%s: first_stream + n_starts * n_samples overflows (%lld + %lld)", who, (long long)first_stream,
                     (long long)(n_starts * n_samples));
    return HJB_OK;
}

// The device side of a campaign call whose arguments have been checked (n_starts >= 1): X0, the thresholds and the planes of the
// steps uploaded once, the block list walked in launches of at most option "chunk" lanes - `launch` starts the controller's kernel
// and the fold on the launch's stream - and stats downloaded.  Under ro->mu.
int run_campaign_launches(Rollout *ro, const char *who, int32_t n_steps, const int32_t *plane_of_step, int64_t n_starts, int64_t n_samples,
                          const double *X0, uint64_t seed, int64_t first_stream, const double *threshold, const double *tol, double *stats,
                          double *device_ms, const std::function<hipError_t(const CampaignLaunch &)> &launch, const CampaignHistCall *hist) {
    const int D = ro->D;
    DCampaign Cp{};
    Cp.M = n_samples;
    Cp.G = campaign_group(n_samples, &Cp.log2G);
    Cp.B = (n_samples + Cp.G - 1) / Cp.G;
    Cp.has_tol = tol ? 1 : 0;
    for (int a = 0; a < D; ++a) {
        Cp.lo[a] = ro->grid_lo[a];
        Cp.hi[a] = ro->grid_hi[a];
        Cp.tol[a] = tol ? tol[a] : 0.0;
    }
    const int64_t n_blocks = n_starts * Cp.B;                 // <= n_starts * n_samples
    const int64_t nb_max = std::min(n_blocks, std::max<int64_t>(ro->chunk / Cp.G, 1));

    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(ro->device) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipSetDevice failed");
    const size_t xb = (size_t)n_starts * D * sizeof(double), sb = (size_t)n_starts * HJB_CAMPAIGN_NSTAT * sizeof(double);
    const size_t tb = threshold ? (size_t)n_starts * sizeof(double) : 0, pb = (size_t)nb_max * HJB_CAMPAIGN_NSTAT * sizeof(double);
    const size_t kb = (size_t)std::max(n_steps, 1) * sizeof(int32_t);
    // the histogram's [lo | hi | scale] and its counts (K30): nothing without one
    const size_t rb = hist ? (size_t)n_starts * 3 * sizeof(double) : 0, hb = hist ? (size_t)n_starts * (hist->n_bins + 2) * sizeof(int64_t) : 0;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipMemGetInfo failed");
    if (xb + sb + tb + pb + kb + rb + hb + ((size_t)64 << 20) > fr)
        return rfail(ro, HJB_E_NOMEM, "%s: %lld starts and launches of %lld blocks need %zu bytes, %zu free (lower option \"chunk\")", who,
                     (long long)n_starts, (long long)nb_max, xb + sb + tb + pb + kb + rb + hb, fr);
    DevData dd(ro->device);                                   // freed on every way out
    const void *dX0 = nullptr, *dthr = nullptr, *dplane = nullptr;
    int st = upload(ro, dd, X0, xb, &dX0);
    if (!st && threshold) st = upload(ro, dd, threshold, tb, &dthr);
    if (!st) st = upload(ro, dd, plane_of_step, n_steps > 0 ? kb : 0, &dplane);
    const void *drange = nullptr;
    if (!st && hist) {                                        // [3, n_starts]: lo, hi and the scale, formed once, here
        std::vector<double> range((size_t)n_starts * 3);
        for (int64_t s = 0; s < n_starts; ++s) {
            range[3 * s] = hist->lo[s];
            range[3 * s + 1] = hist->hi[s];
            range[3 * s + 2] = campaign_hist_scale(hist->lo[s], hist->hi[s], hist->n_bins);
        }
        st = upload(ro, dd, range.data(), rb, &drange);
    }
    if (st) return st;
    double *dstats = nullptr, *dpart = nullptr, *dhist = nullptr;     // stats, partials: written by the kernels before they are read
    for (auto buf : {std::make_pair(&dstats, sb), std::make_pair(&dpart, pb), std::make_pair(&dhist, hb)}) {
        if (!buf.second) continue;
        void *d = nullptr;
        if (hipMalloc(&d, buf.second) != hipSuccess) return rfail(ro, HJB_E_NOMEM, "%s: hipMalloc of %zu bytes failed", who, buf.second);
        dd.allocs.push_back(d);
        *buf.first = (double *)d;
    }
    Cp.threshold = (const double *)dthr;
    Cp.partials = dpart;
    DNoise N = ro->N;
    N.seed = seed;
    N.first = (uint64_t)first_stream;                         // the call's: a lane adds s * M + m, whatever the launch
    N.Wp = nullptr;
    DRollout R = ro->R;
    R.plane_of_step = (const int32_t *)dplane;
    R.n_steps = n_steps;
    // the LDS rule of hjb_rollout_run_noisy: the channel's tables and the node block together
    const size_t lds = (size_t)(2 * (int64_t)R.n_knots + (int64_t)R.n_labels * R.n_u + N.n_tab) * sizeof(double);
    bool lds_on = ro->lds && lds <= kLdsMax;
    size_t lds_launch = lds;
    DCampHist H{};
    if (hist) {                                               // the accumulation form and its LDS bytes, with the tables' placement
        lds_launch = campaign_hist_form(Cp.G, hist->n_bins, ro->lds, lds, kLdsMax, &lds_on, &H);
        H.range = (const double *)drange;
        H.hist = (unsigned long long *)dhist;
    }
    hipStream_t stream = ro->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    double ms_total = 0;
    if (e == hipSuccess && hist) e = hipMemsetAsync(dhist, 0, hb, stream);    // once per call; the launches accumulate
    for (int64_t b0 = 0; e == hipSuccess && b0 < n_blocks; b0 += nb_max) {    // a start's blocks may straddle two launches
        Cp.block0 = b0;
        Cp.n_blocks = std::min(nb_max, n_blocks - b0);
        (void)hipEventRecord(e0, stream);
        e = launch(CampaignLaunch{R, N, Cp, lds_launch, lds_on, stream, (const double *)dX0, dstats, H});
        if (e != hipSuccess) break;
        (void)hipEventRecord(e1, stream);
        e = hipStreamSynchronize(stream);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        ms_total += ms;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(stats, dstats, sb, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && hist) e = hipMemcpyAsync(hist->hist, dhist, hb, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream);
        return rfail(ro, HJB_E_DEVICE, "%s: %s", who, hipGetErrorString(e));
    }
    if (device_ms) *device_ms = ms_total;
    return HJB_OK;
}

}  // namespace hjbhost

extern "C" {

int32_t hjb_rollout_run_campaign(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_starts,
                                 int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream, const double *threshold,
                                 const double *tol, double *stats, double *device_ms) {
    Rollout *ro = (Rollout *)rollout;
    const char *const who = "hjb_rollout_run_campaign";
    // every refusal before any device work, the outputs untouched; the ones that need no object first
    if (const int bad = check_campaign_streams(ro, who, n_starts, n_samples, first_stream)) return bad;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    const int bad_arg = check_run(ro, kModelAffine, method, n_steps, plane_of_step, n_starts);
    if (bad_arg) return bad_arg;
    if (ro->N.n_nodes < 1) return rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_noise", who);
    if (n_starts == 0) {
        if (device_ms) *device_ms = 0.0;
        return HJB_OK;
    }
    const int D = ro->D;
    if (!stats) return rfail(ro, HJB_E_INVALID, "%s: null stats", who);
    const int bad_traj = check_traj(ro, "rollout", D, "D", n_steps, n_starts, X0, stats);
    if (bad_traj) return bad_traj;
    if (const int bad = check_campaign_bounds(ro, who, D, n_starts, threshold, tol)) return bad;
    if (device_ms) *device_ms = 0.0;

    return run_campaign_launches(ro, who, n_steps, plane_of_step, n_starts, n_samples, X0, seed, first_stream, threshold, tol, stats, device_ms,
                                 [&](const CampaignLaunch &c) {
                                     return launch_rollout_campaign(ro->idx_bytes, method, c.lds_on, ro->D, c.R, c.N, c.C, c.lds, c.st, c.X0, c.stats);
                                 });
}

int32_t hjb_rollout_campaign_reduce(int64_t n_starts, int64_t n_samples, int32_t D, const double *cost, const double *X_final,
                                    const uint8_t *left, const double *threshold, const double *tol, double *stats) {
    const char *const who = "hjb_rollout_campaign_reduce";
    if (n_starts < 0) return rfail(nullptr, HJB_E_INVALID, "%s: n_starts=%lld < 0", who, (long long)n_starts);
    if (D < 1 || D > HJB_MAX_D) return rfail(nullptr, HJB_E_INVALID, "%s: D=%d not in 1..%d", who, D, HJB_MAX_D);
    if (const int bad = check_campaign_sizes(nullptr, who, n_starts, n_samples)) return bad;
    if (const int bad = check_campaign_bounds(nullptr, who, D, n_starts, threshold, tol)) return bad;
    if (n_starts == 0) return HJB_OK;
    if (n_starts * n_samples > INT64_MAX / (8 * D)) return rfail(nullptr, HJB_E_INVALID, "%s: size overflow (n_starts x n_samples x D)", who);
    if (!cost || !stats) return rfail(nullptr, HJB_E_INVALID, "%s: null cost / stats", who);
    if (tol && !X_final) return rfail(nullptr, HJB_E_INVALID, "%s: tol given without X_final", who);
    for (int64_t s = 0; s < n_starts; ++s) {
        const int64_t i = s * n_samples;
        campaign_reduce_start(n_samples, D, cost + i, X_final ? X_final + (int64_t)D * i : nullptr, left ? left + i : nullptr,
                              threshold != nullptr, threshold ? threshold[s] : 0.0, tol, stats + HJB_CAMPAIGN_NSTAT * s);
    }
    return HJB_OK;
}

}  // extern "C"
