// rollout_campaign_host.hip - hjb_rollout_run_campaign and hjb_rollout_campaign_reduce (include/hjbdp.h): the host side of the
// noisy campaigns (K28, kernels_rollout_campaign.h / rollout_campaign.hip).  The run function makes hjb_rollout_run_noisy's
// refusals (rollout_host.h: check_run, check_traj) and its own before any device work.  This unit also holds what all five
// campaign run functions (K28 - K31) share: their entry frame (run_campaign_call: the refusals, in one order) and their device
// loop (run_campaign_launches, driven by a CampaignPlan), which uploads X0, the thresholds and the planes once per call (upload)
// and walks the call's block list in launches of at most option "chunk" lanes.  run_chunks is not used: its record and
// its transfers are per trajectory, which is what a campaign does away with.  What a plain call holds on the device is
// [D + 1 + 8, n_starts] doubles and 8 doubles per block of a launch; nothing has a dimension of n_starts * n_samples.
// hjb_rollout_run_actuator_campaign (K34, kernels_rollout_actuator_campaign.h / rollout_actuator_campaign.hip) is the same frame
// and loop on the actuator set's plant (CampaignPlan::actuator).
// The host reduce runs hjbdp_campaign.h's functions in a plain loop, with no device.  No kernel is instantiated in this unit.
#include "rollout_host.h"
#include "kernels_rollout_campaign.h"
#include "kernels_rollout_actuator_campaign.h"

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

// The device side of a campaign call whose arguments have been checked (n_starts >= 1; rollout_host.h).  Under ro->mu.
int run_campaign_launches(Rollout *ro, const CampaignCall &call, const CampaignPlan &plan,
                          const std::function<hipError_t(const CampaignLaunch &)> &launch) {
    const char *const who = call.who;
    const int D = ro->D, n_rec = plan.n_records;
    const int64_t n_starts = call.n_starts;
    const CampaignHistCall *hist = plan.hist;
    const CampaignGeometry g = campaign_geometry(n_starts, call.n_samples, D, call.n_steps, ro->chunk, n_rec, plan.n_plane_lists,
                                                 call.threshold != nullptr, hist ? hist->n_bins : 0, plan.pair_scratch, plan.greedy);
    DCampaign Cp{};
    Cp.M = call.n_samples;
    Cp.G = g.G;
    Cp.log2G = g.log2G;
    Cp.B = g.B;
    Cp.has_tol = call.tol ? 1 : 0;
    for (int a = 0; a < D; ++a) {
        Cp.lo[a] = ro->grid_lo[a];
        Cp.hi[a] = ro->grid_hi[a];
        Cp.tol[a] = call.tol ? call.tol[a] : 0.0;
    }

    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(ro->device) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipSetDevice failed");
    const size_t xb = (size_t)n_starts * D * sizeof(double), sb = (size_t)n_starts * HJB_CAMPAIGN_NSTAT * sizeof(double);
    const size_t tb = call.threshold ? (size_t)n_starts * sizeof(double) : 0, pb = (size_t)g.nb_max * HJB_CAMPAIGN_NSTAT * sizeof(double);
    const size_t kb = (size_t)std::max(call.n_steps, 1) * sizeof(int32_t);
    // the histogram's [lo | hi | scale] and its counts (K30): nothing without one
    const size_t rb = hist ? (size_t)n_starts * 3 * sizeof(double) : 0, hb = hist ? (size_t)n_starts * (hist->n_bins + 2) * sizeof(int64_t) : 0;
    // the pair scratch (K31): one double and one byte per lane of a launch, never n_starts * M
    const size_t cb = plan.pair_scratch ? (size_t)g.lanes_max * sizeof(double) : 0, fb = plan.pair_scratch ? (size_t)g.lanes_max : 0;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipMemGetInfo failed");
    if ((size_t)g.need + ((size_t)64 << 20) > fr) {
        if (plan.pair_scratch)
            return rfail(ro, HJB_E_NOMEM, "%s: %lld starts and launches of %lld blocks need %zu bytes (three records, three partial arrays and "
                         "%zu bytes of pair scratch), %zu free (lower option \"chunk\")", who, (long long)n_starts, (long long)g.nb_max,
                         (size_t)g.need, cb + fb, fr);
        return rfail(ro, HJB_E_NOMEM, "%s: %lld starts and launches of %lld blocks need %zu bytes, %zu free (lower option \"chunk\")", who,
                     (long long)n_starts, (long long)g.nb_max, (size_t)g.need, fr);
    }
    DevData dd(ro->device);                                   // freed on every way out
    const void *dX0 = nullptr, *dthr = nullptr, *dplane[2] = {nullptr, nullptr}, *drange = nullptr, *dgtab = nullptr;
    int st = upload(ro, dd, call.X0, xb, &dX0);
    if (!st && call.threshold) st = upload(ro, dd, call.threshold, tb, &dthr);
    for (int i = 0; !st && i < plan.n_plane_lists; ++i) st = upload(ro, dd, plan.planes[i], call.n_steps > 0 ? kb : 0, &dplane[i]);
    if (!st && hist) {                                        // [3, n_starts]: lo, hi and the scale, formed once, here
        std::vector<double> range((size_t)n_starts * 3);
        for (int64_t s = 0; s < n_starts; ++s) {
            range[3 * s] = hist->lo[s];
            range[3 * s + 1] = hist->hi[s];
            range[3 * s + 2] = campaign_hist_scale(hist->lo[s], hist->hi[s], hist->n_bins);
        }
        st = upload(ro, dd, range.data(), rb, &drange);
    }
    CampaignLaunch c{};
    // HJB_PAIR_GREEDY's set: one zero node of weight 1, mode expect, formed by look_table as hjb_rollout_set_lookahead forms the
    // object's own - which is neither read nor changed
    c.Lg.mode = HJB_DIST_EXPECT;
    if (!st && plan.greedy) {
        const double zeros[HJB_MAX_D] = {}, one = 1.0;
        double tab[1 + HJB_MAX_D];
        const int n_tab = look_table(D, 1, zeros, &one, c.Lg, tab);
        st = upload(ro, dd, tab, (size_t)n_tab * sizeof(double), &dgtab);
        c.Lg.tab = (const double *)dgtab;
    }
    // the records, their partials, the counts and the scratch: all written by the kernels before they are read
    double *dpart[3] = {}, *dhist = nullptr;
    const auto scratch = [&](auto *&out, size_t bytes) -> int {
        void *d = nullptr;
        if (!bytes) return HJB_OK;
        if (hipMalloc(&d, bytes) != hipSuccess) return rfail(ro, HJB_E_NOMEM, "%s: hipMalloc of %zu bytes failed", who, bytes);
        dd.allocs.push_back(d);
        out = static_cast<std::remove_reference_t<decltype(out)>>(d);
        return HJB_OK;
    };
    for (int r = 0; !st && r < n_rec; ++r) st = scratch(c.stats[r], sb);
    for (int r = 0; !st && r < n_rec; ++r) st = scratch(dpart[r], pb);
    if (!st) st = scratch(dhist, hb);
    if (!st) st = scratch(c.pair_cost, cb);
    if (!st) st = scratch(c.pair_left, fb);
    if (st) return st;
    Cp.threshold = (const double *)dthr;
    c.N = ro->N;
    c.N.seed = call.seed;
    c.N.first = (uint64_t)call.first_stream;                  // the call's: a lane adds s * M + m, whatever the launch
    c.N.Wp = nullptr;
    for (int i = 0; i < plan.n_plane_lists; ++i) {
        c.R[i] = ro->R;
        c.R[i].plane_of_step = (const int32_t *)dplane[i];
        c.R[i].n_steps = call.n_steps;
    }
    for (int r = 0; r < n_rec; ++r) {                         // one geometry; each record its own partials
        c.C[r] = Cp;
        c.C[r].partials = dpart[r];
    }
    c.Na = ro->Act;                                           // read by an actuator call alone (K34)
    c.Na.seed = call.seed;
    c.Na.first = (uint64_t)call.first_stream;
    c.Na.Wp = nullptr;
    c.Na.terms = actuator_terms(D, ro->R.n_u, c.Na.live, ro->R.B);  // B of the model in effect at this run
    const size_t lds = c.lds = plan.actuator ? actuator_lds(ro, &c.lds_on) : noisy_lds(ro, &c.lds_on);
    if (hist) {                                               // the accumulation form and its LDS bytes, with the tables' placement
        c.lds = campaign_hist_form(Cp.G, hist->n_bins, ro->lds, lds, kLdsMax, &c.lds_on, &c.H);
        c.H.range = (const double *)drange;
        c.H.hist = (unsigned long long *)dhist;
    }
    c.X0 = (const double *)dX0;
    hipStream_t stream = c.st = ro->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    double ms_total = 0;
    if (e == hipSuccess && hist) e = hipMemsetAsync(dhist, 0, hb, stream);    // once per call; the launches accumulate
    for (int64_t b0 = 0; e == hipSuccess && b0 < g.n_blocks; b0 += g.nb_max) {    // a start's blocks may straddle two launches
        for (int r = 0; r < n_rec; ++r) {
            c.C[r].block0 = b0;
            c.C[r].n_blocks = std::min(g.nb_max, g.n_blocks - b0);
        }
        (void)hipEventRecord(e0, stream);
        e = launch(c);
        if (e != hipSuccess) break;
        (void)hipEventRecord(e1, stream);
        e = hipStreamSynchronize(stream);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        ms_total += ms;
    }
    for (int r = 0; e == hipSuccess && r < n_rec; ++r) e = hipMemcpyAsync(plan.stats[r], c.stats[r], sb, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && hist) e = hipMemcpyAsync(hist->hist, dhist, hb, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream);
        return rfail(ro, HJB_E_DEVICE, "%s: %s", who, hipGetErrorString(e));
    }
    if (call.device_ms) *call.device_ms = ms_total;
    return HJB_OK;
}

// The frame of the five run functions (rollout_host.h): every refusal before any device work, the outputs untouched; the ones that
// need no object first
int run_campaign_call(void *rollout, const CampaignCall &call, const CampaignPlan &plan, const std::function<int(Rollout *)> &no_object,
                      const std::function<int(Rollout *)> &controller, const std::function<hipError_t(const CampaignLaunch &)> &launch) {
    Rollout *ro = (Rollout *)rollout;
    const char *const who = call.who;
    if (const int bad = check_campaign_streams(ro, who, call.n_starts, call.n_samples, call.first_stream)) return bad;
    if (no_object)
        if (const int bad = no_object(ro)) return bad;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    if (const int bad = controller(ro)) return bad;
    if (call.n_starts == 0) {
        if (call.device_ms) *call.device_ms = 0.0;
        return HJB_OK;
    }
    for (int r = 0; r < plan.n_records; ++r)
        if (!plan.stats[r]) return rfail(ro, HJB_E_INVALID, plan.n_records == 1 ? "%s: null stats" : "%s: null stats_a / stats_b / stats_d", who);
    if (const int bad = check_traj(ro, "rollout", ro->D, "D", call.n_steps, call.n_starts, call.X0, plan.stats[0])) return bad;
    if (const int bad = check_campaign_bounds(ro, who, ro->D, call.n_starts, call.threshold, call.tol)) return bad;
    if (plan.hist)
        if (const int bad = check_campaign_hist(ro, who, call.n_starts, *plan.hist)) return bad;
    if (call.device_ms) *call.device_ms = 0.0;
    return run_campaign_launches(ro, call, plan, launch);
}

}  // namespace hjbhost

extern "C" {

int32_t hjb_rollout_run_campaign(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_starts,
                                 int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream, const double *threshold,
                                 const double *tol, double *stats, double *device_ms) {
    const CampaignCall call{"hjb_rollout_run_campaign", n_steps, n_starts, n_samples, X0, seed, first_stream, threshold, tol, device_ms};
    CampaignPlan plan;
    plan.stats[0] = stats;
    plan.planes[0] = plane_of_step;
    return run_campaign_call(
        rollout, call, plan, nullptr,
        [&](Rollout *ro) {
            if (const int bad = check_run(ro, kModelAffine, method, n_steps, plane_of_step, n_starts)) return bad;
            return ro->N.n_nodes < 1 ? rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_noise", call.who) : HJB_OK;
        },
        [&](const CampaignLaunch &c) {
            const Rollout *ro = (const Rollout *)rollout;
            return launch_rollout_campaign(ro->idx_bytes, method, c.lds_on, ro->D, c.R[0], c.N, c.C[0], c.lds, c.st, c.X0, c.stats[0]);
        });
}

// K34: hjb_rollout_run_campaign's frame and loop on the actuator set's plant (kernels_rollout_actuator_campaign.h)
int32_t hjb_rollout_run_actuator_campaign(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_starts,
                                          int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream, const double *threshold,
                                          const double *tol, double *stats, double *device_ms) {
    const CampaignCall call{"hjb_rollout_run_actuator_campaign", n_steps, n_starts, n_samples, X0, seed, first_stream, threshold, tol, device_ms};
    CampaignPlan plan;
    plan.stats[0] = stats;
    plan.planes[0] = plane_of_step;
    plan.actuator = true;
    return run_campaign_call(
        rollout, call, plan, nullptr,
        [&](Rollout *ro) {
            if (const int bad = check_run(ro, kModelAffine, method, n_steps, plane_of_step, n_starts)) return bad;
            return ro->Act.n_nodes < 1 ? rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_actuator_noise", call.who) : HJB_OK;
        },
        [&](const CampaignLaunch &c) {
            const Rollout *ro = (const Rollout *)rollout;
            return launch_rollout_actuator_campaign(ro->idx_bytes, method, c.lds_on, ro->D, c.R[0], c.Na, c.C[0], c.lds, c.st, c.X0, c.stats[0]);
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
