// rollout_campaign_hist_host.hip - hjb_rollout_run_campaign_hist, hjb_rollout_run_lookahead_campaign_hist and
// hjb_rollout_campaign_hist_reduce (include/hjbdp.h): the host side of the campaign histograms (K30,
// kernels_rollout_campaign_hist.h / kernels_rollout_lookahead_campaign_hist.h).  The run functions make the plain campaign's
// refusals in the plain campaign's order and the histogram's own (check_campaign_hist) before any device work - the campaigns' one
// entry frame (run_campaign_call, rollout_campaign_host.hip) with n_bins refused before an object is needed - then the campaigns'
// one device loop (run_campaign_launches) with the histogram in the plan and K30's launch.  The host reduce bins a cost array
// with hjbdp_campaign.h's campaign_bin in a plain loop, with no device.  No kernel is instantiated in this unit.
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

// what a histogram call refuses before it needs an object: n_bins out of range, in check_campaign_hist's text
static int check_n_bins(Rollout *ro, const char *who, const CampaignHistCall &h) {
    return h.n_bins < 1 || h.n_bins > HJB_CAMPAIGN_MAX_BINS ? check_campaign_hist(ro, who, 0, h) : HJB_OK;
}

int32_t hjb_rollout_run_campaign_hist(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_starts,
                                      int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream, const double *threshold,
                                      const double *tol, const double *lo, const double *hi, int32_t n_bins, double *stats, int64_t *hist,
                                      double *device_ms) {
    const CampaignCall call{"hjb_rollout_run_campaign_hist", n_steps, n_starts, n_samples, X0, seed, first_stream, threshold, tol, device_ms};
    const CampaignHistCall h{lo, hi, n_bins, hist};
    CampaignPlan plan;
    plan.stats[0] = stats;
    plan.planes[0] = plane_of_step;
    plan.hist = &h;
    return run_campaign_call(
        rollout, call, plan, [&](Rollout *ro) { return check_n_bins(ro, call.who, h); },
        [&](Rollout *ro) {
            if (const int bad = check_run(ro, kModelAffine, method, n_steps, plane_of_step, n_starts)) return bad;
            return ro->N.n_nodes < 1 ? rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_noise", call.who) : HJB_OK;
        },
        [&](const CampaignLaunch &c) {
            const Rollout *ro = (const Rollout *)rollout;
            return launch_rollout_campaign_hist(ro->idx_bytes, method, c.lds_on, ro->D, c.R[0], c.N, c.C[0], c.H, c.lds, c.st, c.X0, c.stats[0]);
        });
}

int32_t hjb_rollout_run_lookahead_campaign_hist(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_starts,
                                                int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream,
                                                const double *threshold, const double *tol, const double *lo, const double *hi,
                                                int32_t n_bins, double *stats, int64_t *hist, double *device_ms) {
    const CampaignCall call{"hjb_rollout_run_lookahead_campaign_hist", n_steps, n_starts, n_samples, X0, seed, first_stream, threshold, tol,
                            device_ms};
    const CampaignHistCall h{lo, hi, n_bins, hist};
    CampaignPlan plan;
    plan.stats[0] = stats;
    plan.planes[0] = value_plane_of_step;
    plan.hist = &h;
    return run_campaign_call(
        rollout, call, plan, [&](Rollout *ro) { return check_n_bins(ro, call.who, h); },
        [&](Rollout *ro) { return check_lookahead_run(ro, call.who, 1, n_steps, value_plane_of_step, n_starts); },
        [&](const CampaignLaunch &c) {
            const Rollout *ro = (const Rollout *)rollout;
            const DLookCampaignHistArgs K{{c.R[0], ro->dvalues, ro->L, c.N, c.C[0], c.X0}, c.H};
            return launch_rollout_lookahead_campaign_hist(ro->val_bytes, c.lds_on, ro->D, K, c.lds, c.st, c.stats[0]);
        });
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
