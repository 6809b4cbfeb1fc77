// rollout_campaign_pair_host.hip - hjb_rollout_run_campaign_pair and hjb_rollout_campaign_pair_reduce (include/hjbdp.h): the host
// side of the paired campaigns (K31, kernels_rollout_campaign_pair.h / kernels_rollout_lookahead_campaign_pair.h).  The run function
// makes the plain campaigns' refusals for each side, named "A:" / "B:", and its own before any device work - the campaigns' one
// entry frame (run_campaign_call, rollout_campaign_host.hip), with the kinds refused before an object is needed - then walks the
// call's block list in the campaigns' one device loop (run_campaign_launches), whose plan asks for three records, two plane lists,
// the pair scratch and, for a greedy side, the one-node lookahead table: per launch A's flight kernel, B's flight kernel and K28's
// fold three times, all on the object's stream, synchronised once.  What a call holds on the device is [D + 1 + 24, n_starts]
// doubles, 24 doubles per block of a launch and the pair scratch, one double and one byte per lane of a launch; nothing has a
// dimension of n_starts * n_samples.
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

}  // namespace

extern "C" {

int32_t hjb_rollout_run_campaign_pair(void *rollout, int32_t kind_a, int32_t method_a, const int32_t *planes_a, int32_t kind_b,
                                      int32_t method_b, const int32_t *planes_b, int32_t n_steps, int64_t n_starts, int64_t n_samples,
                                      const double *X0, uint64_t seed, int64_t first_stream, const double *threshold, const double *tol,
                                      double *stats_a, double *stats_b, double *stats_d, double *device_ms) {
    const CampaignCall call{"hjb_rollout_run_campaign_pair", n_steps, n_starts, n_samples, X0, seed, first_stream, threshold, tol, device_ms};
    const char *const who = call.who;
    const PairSide sa{"A", kind_a, method_a, planes_a}, sb{"B", kind_b, method_b, planes_b};
    CampaignPlan plan;
    plan.n_records = 3;                                       // A's, B's and d's
    plan.stats[0] = stats_a, plan.stats[1] = stats_b, plan.stats[2] = stats_d;
    plan.n_plane_lists = 2;
    plan.planes[0] = planes_a, plan.planes[1] = planes_b;
    plan.pair_scratch = true;
    plan.greedy = kind_a == HJB_PAIR_GREEDY || kind_b == HJB_PAIR_GREEDY;
    return run_campaign_call(
        rollout, call, plan,
        [&](Rollout *ro) {
            for (const PairSide *sd : {&sa, &sb})
                if (sd->kind < HJB_PAIR_LABELS || sd->kind > HJB_PAIR_GREEDY)
                    return rfail(ro, HJB_E_INVALID, "%s: %s: kind %d not in 0..2", who, sd->name, sd->kind);
            return (int)HJB_OK;
        },
        [&](Rollout *ro) {
            const int bad = check_pair_side(ro, who, sa, n_steps, n_starts);
            return bad ? bad : check_pair_side(ro, who, sb, n_steps, n_starts);
        },
        // per launch: A flies and leaves its costs and flags in the scratch; B flies, reads them at the same lanes and reduces d as
        // well; K28's fold, once per record - all on the object's stream
        [&](const CampaignLaunch &c) {
            const Rollout *ro = (const Rollout *)rollout;
            auto fly = [&](const PairSide &sd, const DRollout &Rs, const DCampaign &C, const DCampPair &P) -> hipError_t {
                if (sd.kind == HJB_PAIR_LABELS)
                    return launch_rollout_campaign_pair(ro->idx_bytes, sd.method, c.lds_on, ro->D, Rs, c.N, C, P, c.lds, c.st, c.X0);
                const DLookCampaignPairArgs K{{Rs, ro->dvalues, sd.kind == HJB_PAIR_LOOKAHEAD ? ro->L : c.Lg, c.N, C, c.X0}, P};
                return launch_rollout_lookahead_campaign_pair(ro->val_bytes, c.lds_on, ro->D, K, c.lds, c.st);
            };
            hipError_t e = fly(sa, c.R[0], c.C[0], DCampPair{c.pair_cost, c.pair_left, nullptr, 1, 0});
            if (e == hipSuccess) e = fly(sb, c.R[1], c.C[1], DCampPair{c.pair_cost, c.pair_left, c.C[2].partials, 0, 1});
            for (int i = 0; e == hipSuccess && i < 3; ++i) e = launch_campaign_fold(c.C[i], c.st, c.stats[i]);
            return e;
        });
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
