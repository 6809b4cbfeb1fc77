// rollout_campaign_pair_host.hip - hjb_rollout_run_campaign_pair and hjb_rollout_campaign_pair_reduce (include/hjbdp.h): the host
// side of the paired campaigns (K31, kernels_rollout_campaign_pair.h / kernels_rollout_lookahead_campaign_pair.h).  The run function
// makes the plain campaigns' refusals for each side, named "A:" / "B:", and its own before any device work, then walks the call's
// block list as run_campaign_launches does (rollout_campaign_host.hip: a sibling, so that the plain and the histogram calls keep
// their loop and their device-memory bound): per launch A's flight kernel, B's flight kernel and K28's fold three times, all on
// the object's stream, synchronised once.  What a call holds on the device is [D + 1 + 24, n_starts] doubles, 24 doubles per block
// of a launch and the pair scratch, one double and one byte per lane of a launch; nothing has a dimension of n_starts * n_samples.
// The host reduce runs hjbdp_campaign.h's campaign_pair_start in a plain loop, with no device.  No kernel is instantiated here.
#include "rollout_host.h"
#include "kernels_rollout_lookahead_campaign_pair.h"

using namespace hjbhost;

static_assert(HJB_CAMPAIGN_PAIR_NSTAT == HJB_CAMPAIGN_NSTAT, "the difference record is K28's record of d");

namespace {

struct PairSide {
    const char *name;                 // "A" / "B"
    int32_t kind, method;
    const int32_t *planes;
};

// What the plain campaign of the side's kind refuses of the object and the planes, with the side named in front of its text
int check_pair_side(Rollout *ro, const char *who, const PairSide &sd, int32_t n_steps, int64_t n_starts) {
    int bad;
    if (sd.kind == HJB_PAIR_LABELS) {
        bad = check_run(ro, kModelAffine, sd.method, n_steps, sd.planes, n_starts);
        if (!bad && ro->N.n_nodes < 1) bad = rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_noise", who);
    } else {
        bad = check_lookahead_run(ro, who, 1, n_steps, sd.planes, n_starts, sd.kind == HJB_PAIR_LOOKAHEAD);
    }
    if (!bad) return HJB_OK;
    const std::string text = ro->err;
    return rfail(ro, bad, "%s: %s", sd.name, text.c_str());
}

// The device side of a pair call whose arguments have been checked (n_starts >= 1).  Under ro->mu.
int run_campaign_pair_launches(Rollout *ro, const char *who, const PairSide &sa, const PairSide &sb, int32_t n_steps, int64_t n_starts,
                               int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream, const double *threshold,
                               const double *tol, double *const stats[3], double *device_ms) {
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
    const int64_t lanes_max = nb_max * Cp.G;                  // the pair scratch: the lanes of a launch, never n_starts * M

    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(ro->device) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipSetDevice failed");
    const size_t xb = (size_t)n_starts * D * sizeof(double), sb1 = (size_t)n_starts * HJB_CAMPAIGN_NSTAT * sizeof(double);
    const size_t tb = threshold ? (size_t)n_starts * sizeof(double) : 0, pb1 = (size_t)nb_max * HJB_CAMPAIGN_NSTAT * sizeof(double);
    const size_t kb = (size_t)std::max(n_steps, 1) * sizeof(int32_t);
    const size_t cb = (size_t)lanes_max * sizeof(double), fb = (size_t)lanes_max;
    const bool greedy = sa.kind == HJB_PAIR_GREEDY || sb.kind == HJB_PAIR_GREEDY;
    const size_t gb = greedy ? 16 : 0;
    const size_t need = xb + 3 * sb1 + tb + 3 * pb1 + 2 * kb + cb + fb + gb;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipMemGetInfo failed");
    if (need + ((size_t)64 << 20) > fr)
        return rfail(ro, HJB_E_NOMEM, "%s: %lld starts and launches of %lld blocks need %zu bytes (three records, three partial arrays and "
                     "%zu bytes of pair scratch), %zu free (lower option \"chunk\")", who, (long long)n_starts, (long long)nb_max, need,
                     cb + fb, fr);
    DevData dd(ro->device);                                   // freed on every way out
    const void *dX0 = nullptr, *dthr = nullptr, *dplane[2] = {nullptr, nullptr}, *dgtab = nullptr;
    int st = upload(ro, dd, X0, xb, &dX0);
    if (!st && threshold) st = upload(ro, dd, threshold, tb, &dthr);
    if (!st) st = upload(ro, dd, sa.planes, n_steps > 0 ? kb : 0, &dplane[0]);
    if (!st) st = upload(ro, dd, sb.planes, n_steps > 0 ? kb : 0, &dplane[1]);
    // HJB_PAIR_GREEDY's set: one zero node of weight 1, mode expect, formed by look_table as hjb_rollout_set_lookahead forms the
    // object's own - which is neither read nor changed
    LookSet Lg{};
    Lg.mode = HJB_DIST_EXPECT;
    if (!st && greedy) {
        const double zeros[HJB_MAX_D] = {}, one = 1.0;
        double tab[1 + HJB_MAX_D];
        const int n_tab = look_table(D, 1, zeros, &one, Lg, tab);
        st = upload(ro, dd, tab, (size_t)n_tab * sizeof(double), &dgtab);
        Lg.tab = (const double *)dgtab;
    }
    if (st) return st;
    double *dstats[3] = {}, *dpart[3] = {}, *dcost = nullptr;
    uint8_t *dleft = nullptr;
    void *got[8] = {};
    const size_t want[8] = {sb1, sb1, sb1, pb1, pb1, pb1, cb, fb};
    for (int i = 0; i < 8; ++i) {                             // all written by the kernels before they are read
        if (hipMalloc(&got[i], want[i]) != hipSuccess) return rfail(ro, HJB_E_NOMEM, "%s: hipMalloc of %zu bytes failed", who, want[i]);
        dd.allocs.push_back(got[i]);
    }
    for (int i = 0; i < 3; ++i) {
        dstats[i] = (double *)got[i];
        dpart[i] = (double *)got[3 + i];
    }
    dcost = (double *)got[6];
    dleft = (uint8_t *)got[7];
    Cp.threshold = (const double *)dthr;
    DNoise N = ro->N;
    N.seed = seed;
    N.first = (uint64_t)first_stream;                         // the call's: a lane adds s * M + m, whatever the launch
    N.Wp = nullptr;
    DRollout R[2] = {ro->R, ro->R};
    for (int i = 0; i < 2; ++i) {
        R[i].plane_of_step = (const int32_t *)dplane[i];
        R[i].n_steps = n_steps;
    }
    // the LDS rule each plain kernel has, which is one rule: the channel's tables and the node block together
    const size_t lds = (size_t)(2 * (int64_t)ro->R.n_knots + (int64_t)ro->R.n_labels * ro->R.n_u + N.n_tab) * sizeof(double);
    const bool lds_on = ro->lds && lds <= kLdsMax;
    hipStream_t stream = ro->stream;
    auto fly = [&](const PairSide &sd, const DRollout &Rs, const DCampaign &C, const DCampPair &P) -> hipError_t {
        if (sd.kind == HJB_PAIR_LABELS)
            return launch_rollout_campaign_pair(ro->idx_bytes, sd.method, lds_on, D, Rs, N, C, P, lds, stream, (const double *)dX0);
        const DLookCampaignPairArgs K{{Rs, ro->dvalues, sd.kind == HJB_PAIR_LOOKAHEAD ? ro->L : Lg, N, C, (const double *)dX0}, P};
        return launch_rollout_lookahead_campaign_pair(ro->val_bytes, lds_on, D, K, lds, stream);
    };
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    double ms_total = 0;
    for (int64_t b0 = 0; e == hipSuccess && b0 < n_blocks; b0 += nb_max) {    // a start's blocks may straddle two launches
        Cp.block0 = b0;
        Cp.n_blocks = std::min(nb_max, n_blocks - b0);
        DCampaign C[3] = {Cp, Cp, Cp};                        // one geometry; each record its own partials
        for (int i = 0; i < 3; ++i) C[i].partials = dpart[i];
        (void)hipEventRecord(e0, stream);
        // A flies and leaves its costs and flags in the scratch; B flies, reads them at the same lanes and reduces d as well
        e = fly(sa, R[0], C[0], DCampPair{dcost, dleft, nullptr, 1, 0});
        if (e == hipSuccess) e = fly(sb, R[1], C[1], DCampPair{dcost, dleft, dpart[2], 0, 1});
        for (int i = 0; e == hipSuccess && i < 3; ++i) e = launch_campaign_fold(C[i], stream, dstats[i]);
        if (e != hipSuccess) break;
        (void)hipEventRecord(e1, stream);
        e = hipStreamSynchronize(stream);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        ms_total += ms;
    }
    for (int i = 0; e == hipSuccess && i < 3; ++i) e = hipMemcpyAsync(stats[i], dstats[i], sb1, hipMemcpyDeviceToHost, stream);
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

}  // namespace

extern "C" {

int32_t hjb_rollout_run_campaign_pair(void *rollout, int32_t kind_a, int32_t method_a, const int32_t *planes_a, int32_t kind_b,
                                      int32_t method_b, const int32_t *planes_b, int32_t n_steps, int64_t n_starts, int64_t n_samples,
                                      const double *X0, uint64_t seed, int64_t first_stream, const double *threshold, const double *tol,
                                      double *stats_a, double *stats_b, double *stats_d, double *device_ms) {
    Rollout *ro = (Rollout *)rollout;
    const char *const who = "hjb_rollout_run_campaign_pair";
    // every refusal before any device work, the outputs untouched; the ones that need no object first
    if (const int bad = check_campaign_streams(ro, who, n_starts, n_samples, first_stream)) return bad;
    if (kind_a < HJB_PAIR_LABELS || kind_a > HJB_PAIR_GREEDY) return rfail(ro, HJB_E_INVALID, "%s: A: kind %d not in 0..2", who, kind_a);
    if (kind_b < HJB_PAIR_LABELS || kind_b > HJB_PAIR_GREEDY) return rfail(ro, HJB_E_INVALID, "%s: B: kind %d not in 0..2", who, kind_b);
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    const PairSide sa{"A", kind_a, method_a, planes_a}, sb{"B", kind_b, method_b, planes_b};
    if (const int bad = check_pair_side(ro, who, sa, n_steps, n_starts)) return bad;
    if (const int bad = check_pair_side(ro, who, sb, n_steps, n_starts)) return bad;
    if (n_starts == 0) {
        if (device_ms) *device_ms = 0.0;
        return HJB_OK;
    }
    const int D = ro->D;
    if (!stats_a || !stats_b || !stats_d) return rfail(ro, HJB_E_INVALID, "%s: null stats_a / stats_b / stats_d", who);
    if (const int bad = check_traj(ro, "rollout", D, "D", n_steps, n_starts, X0, stats_a)) return bad;
    if (const int bad = check_campaign_bounds(ro, who, D, n_starts, threshold, tol)) return bad;
    if (device_ms) *device_ms = 0.0;
    double *const stats[3] = {stats_a, stats_b, stats_d};
    return run_campaign_pair_launches(ro, who, sa, sb, n_steps, n_starts, n_samples, X0, seed, first_stream, threshold, tol, stats, device_ms);
}

int32_t hjb_rollout_campaign_pair_reduce(int64_t n_starts, int64_t n_samples, const double *cost_a, const double *cost_b,
                                         const uint8_t *left_a, const uint8_t *left_b, double *stats_d) {
    const char *const who = "hjb_rollout_campaign_pair_reduce";
    if (n_starts < 0) return rfail(nullptr, HJB_E_INVALID, "%s: n_starts=%lld < 0", who, (long long)n_starts);
    if (const int bad = check_campaign_sizes(nullptr, who, n_starts, n_samples)) return bad;
    if (n_starts == 0) return HJB_OK;
    if (n_starts * n_samples > INT64_MAX / 8) return rfail(nullptr, HJB_E_INVALID, "%s: size overflow (n_starts x n_samples)", who);
    if (!cost_a || !cost_b || !stats_d) return rfail(nullptr, HJB_E_INVALID, "%s: null cost_a / cost_b / stats_d", who);
    for (int64_t s = 0; s < n_starts; ++s) {
        const int64_t i = s * n_samples;
        campaign_pair_start(n_samples, cost_a + i, cost_b + i, left_a ? left_a + i : nullptr, left_b ? left_b + i : nullptr,
                            stats_d + HJB_CAMPAIGN_PAIR_NSTAT * s);
    }
    return HJB_OK;
}

}  // extern "C"
