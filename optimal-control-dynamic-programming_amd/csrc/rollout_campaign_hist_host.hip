// rollout_campaign_hist_host.hip - hjb_rollout_run_campaign_hist, hjb_rollout_run_lookahead_campaign_hist and
// hjb_rollout_campaign_hist_reduce (include/hjbdp.h): the host side of the campaign histograms (K30,
// kernels_rollout_campaign_hist.h / kernels_rollout_lookahead_campaign_hist.h).  The run functions make the plain campaign's
// refusals in the plain campaign's order and the histogram's own (check_campaign_hist) before any device work, then K28's device
// side (run_campaign_launches) with the histogram and K30's launch.  The host reduce bins a cost array with hjbdp_campaign.h's
// campaign_bin in a plain loop, with no device.  No kernel is instantiated in this unit.
#include "rollout_host.h"
#include "kernels_rollout_lookahead_campaign_hist.h"

using namespace hjbhost;

namespace hjbhost {

int check_campaign_hist(Rollout *ro, const char *who, int64_t n_starts, const CampaignHistCall &h) {
    if (h.n_bins < 1 || h.n_bins > HJB_CAMPAIGN_MAX_BINS)
        return rfail(ro, HJB_E_INVALID, "%s: n_bins=%d not in 1..%d", who, h.n_bins, HJB_CAMPAIGN_MAX_BINS);
    if (n_starts <= 0) return HJB_OK;
    if (!h.lo || !h.hi || !h.hist) return rfail(ro, HJB_E_INVALID, "%s: null lo / hi / hist", who);
    for (int64_t s = 0; s < n_starts; ++s) {
        if (!all_finite(h.lo + s, 1) || !all_finite(h.hi + s, 1))
            return rfail(ro, HJB_E_INVALID, "%s: lo[%lld] = %g or hi[%lld] = %g is not finite", who, (long long)s, h.lo[s], (long long)s, h.hi[s]);
        if (!(h.lo[s] < h.hi[s]))
            return rfail(ro, HJB_E_INVALID, "%s: lo[%lld] = %g is not below hi[%lld] = %g", who, (long long)s, h.lo[s], (long long)s, h.hi[s]);
        if (!campaign_hist_range_ok(h.lo[s], h.hi[s], h.n_bins))
            return rfail(ro, HJB_E_INVALID, "%s: the scale n_bins / (hi[%lld] - lo[%lld]) = %d / %g is not finite", who, (long long)s, (long long)s,
                         h.n_bins, h.hi[s] - h.lo[s]);
    }
    return HJB_OK;
}

}  // namespace hjbhost

static_assert(HJB_CAMPAIGN_MAX_BINS == hjb::kCampaignMaxBins, "the header's bound is the contract's");

extern "C" {

int32_t hjb_rollout_run_campaign_hist(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_starts,
                                      int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream, const double *threshold,
                                      const double *tol, const double *lo, const double *hi, int32_t n_bins, double *stats, int64_t *hist,
                                      double *device_ms) {
    Rollout *ro = (Rollout *)rollout;
    const char *const who = "hjb_rollout_run_campaign_hist";
    const CampaignHistCall h{lo, hi, n_bins, hist};
    // every refusal before any device work, the outputs untouched; the ones that need no object first
    if (const int bad = check_campaign_streams(ro, who, n_starts, n_samples, first_stream)) return bad;
    if (n_bins < 1 || n_bins > HJB_CAMPAIGN_MAX_BINS) return check_campaign_hist(ro, who, 0, h);
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    if (const int bad = check_run(ro, kModelAffine, method, n_steps, plane_of_step, n_starts)) return bad;
    if (ro->N.n_nodes < 1) return rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_noise", who);
    if (n_starts == 0) {
        if (device_ms) *device_ms = 0.0;
        return HJB_OK;
    }
    const int D = ro->D;
    if (!stats) return rfail(ro, HJB_E_INVALID, "%s: null stats", who);
    if (const int bad = check_traj(ro, "rollout", D, "D", n_steps, n_starts, X0, stats)) return bad;
    if (const int bad = check_campaign_bounds(ro, who, D, n_starts, threshold, tol)) return bad;
    if (const int bad = check_campaign_hist(ro, who, n_starts, h)) return bad;
    if (device_ms) *device_ms = 0.0;
    return run_campaign_launches(
        ro, who, n_steps, plane_of_step, n_starts, n_samples, X0, seed, first_stream, threshold, tol, stats, device_ms,
        [&](const CampaignLaunch &c) {
            return launch_rollout_campaign_hist(ro->idx_bytes, method, c.lds_on, ro->D, c.R, c.N, c.C, c.H, c.lds, c.st, c.X0, c.stats);
        },
        &h);
}

int32_t hjb_rollout_run_lookahead_campaign_hist(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_starts,
                                                int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream,
                                                const double *threshold, const double *tol, const double *lo, const double *hi,
                                                int32_t n_bins, double *stats, int64_t *hist, double *device_ms) {
    Rollout *ro = (Rollout *)rollout;
    const char *const who = "hjb_rollout_run_lookahead_campaign_hist";
    const CampaignHistCall h{lo, hi, n_bins, hist};
    if (const int bad = check_campaign_streams(ro, who, n_starts, n_samples, first_stream)) return bad;
    if (n_bins < 1 || n_bins > HJB_CAMPAIGN_MAX_BINS) return check_campaign_hist(ro, who, 0, h);
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    if (const int bad = check_lookahead_run(ro, who, 1, n_steps, value_plane_of_step, n_starts)) return bad;
    if (n_starts == 0) {
        if (device_ms) *device_ms = 0.0;
        return HJB_OK;
    }
    const int D = ro->D;
    if (!stats) return rfail(ro, HJB_E_INVALID, "%s: null stats", who);
    if (const int bad = check_traj(ro, "rollout", D, "D", n_steps, n_starts, X0, stats)) return bad;
    if (const int bad = check_campaign_bounds(ro, who, D, n_starts, threshold, tol)) return bad;
    if (const int bad = check_campaign_hist(ro, who, n_starts, h)) return bad;
    if (device_ms) *device_ms = 0.0;
    return run_campaign_launches(
        ro, who, n_steps, value_plane_of_step, n_starts, n_samples, X0, seed, first_stream, threshold, tol, stats, device_ms,
        [&](const CampaignLaunch &c) {
            const DLookCampaignHistArgs K{{c.R, ro->dvalues, ro->L, c.N, c.C, c.X0}, c.H};
            return launch_rollout_lookahead_campaign_hist(ro->val_bytes, c.lds_on, D, K, c.lds, c.st, c.stats);
        },
        &h);
}

int32_t hjb_rollout_campaign_hist_reduce(int64_t n_starts, int64_t n_samples, const double *cost, const double *lo, const double *hi,
                                         int32_t n_bins, int64_t *hist) {
    const char *const who = "hjb_rollout_campaign_hist_reduce";
    if (n_starts < 0) return rfail(nullptr, HJB_E_INVALID, "%s: n_starts=%lld < 0", who, (long long)n_starts);
    if (const int bad = check_campaign_sizes(nullptr, who, n_starts, n_samples)) return bad;
    const CampaignHistCall h{lo, hi, n_bins, hist};
    if (const int bad = check_campaign_hist(nullptr, who, n_starts, h)) return bad;
    if (n_starts == 0) return HJB_OK;
    if (n_starts * n_samples > INT64_MAX / 8) return rfail(nullptr, HJB_E_INVALID, "%s: size overflow (n_starts x n_samples)", who);
    if (!cost) return rfail(nullptr, HJB_E_INVALID, "%s: null cost", who);
    for (int64_t s = 0; s < n_starts; ++s)
        campaign_hist_start(n_samples, cost + s * n_samples, lo[s], hi[s], n_bins, hist + (int64_t)(n_bins + 2) * s);
    return HJB_OK;
}

}  // extern "C"
