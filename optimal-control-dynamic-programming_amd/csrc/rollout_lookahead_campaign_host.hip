// rollout_lookahead_campaign_host.hip - hjb_rollout_run_lookahead_campaign and hjb_rollout_lookahead_campaign_host
// (include/hjbdp.h): the host side of the lookahead campaigns (K29, kernels_rollout_lookahead_campaign.h /
// rollout_lookahead_campaign.hip).  The run function makes hjb_rollout_run_lookahead's refusals with fly_noise = 1
// (check_lookahead_run) and K28's of the sizes, the streams and the bounds (check_campaign_*) before any device work - the
// campaigns' one entry frame (run_campaign_call, rollout_campaign_host.hip) - then their one device loop (run_campaign_launches)
// with K29's launch.  The host twin flies one start's samples at a time with
// lookahead_rollout_host (hjbdp_lookahead.h) under the nodes hjbdp_noise.h draws, and reduces them with hjbdp_campaign.h.
// No kernel is instantiated in this unit.
#include "rollout_host.h"
#include "kernels_rollout_lookahead_campaign.h"
#include "rollout_dispatch.h"

using namespace hjbhost;

extern "C" {

int32_t hjb_rollout_run_lookahead_campaign(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_starts,
                                           int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream,
                                           const double *threshold, const double *tol, double *stats, double *device_ms) {
    const CampaignCall call{"hjb_rollout_run_lookahead_campaign", n_steps, n_starts, n_samples, X0, seed, first_stream, threshold, tol, device_ms};
    CampaignPlan plan;
    plan.stats[0] = stats;
    plan.planes[0] = value_plane_of_step;
    return run_campaign_call(
        rollout, call, plan, nullptr,
        [&](Rollout *ro) { return check_lookahead_run(ro, call.who, 1, n_steps, value_plane_of_step, n_starts); },
        [&](const CampaignLaunch &c) {
            const Rollout *ro = (const Rollout *)rollout;
            const DLookCampaignArgs K{c.R[0], ro->dvalues, ro->L, c.N, c.C[0], c.X0};
            return launch_rollout_lookahead_campaign(ro->val_bytes, c.lds_on, ro->D, K, c.lds, c.st, c.stats[0]);
        });
}

int32_t hjb_rollout_lookahead_campaign_host(int32_t D, const int32_t *n, const double *knots, int32_t n_labels, int32_t n_u,
                                            const double *u_table, const double *A, const double *B, const double *c, const double *q,
                                            const double *r, int32_t dtype, int32_t n_value_planes, const void *values, int32_t n_steps,
                                            const int32_t *value_plane_of_step, int32_t mode, int32_t n_nodes, const double *offsets,
                                            const double *weights, int32_t n_flight_nodes, const double *flight_offsets,
                                            const double *flight_weights, int64_t n_starts, int64_t n_samples, const double *X0,
                                            uint64_t seed, int64_t first_stream, const double *threshold, const double *tol, double *stats) {
    const char *const who = "hjb_rollout_lookahead_campaign_host";
    if (const int bad = check_campaign_streams(nullptr, who, n_starts, n_samples, first_stream)) return bad;
    const AffineHostArgs a{D, n, knots, n_labels, n_u, u_table, A, B, c, q, r, dtype, n_value_planes, values, n_steps, value_plane_of_step};
    if (const int bad = look_host_args(who, a, n_starts, mode, n_nodes, offsets, weights)) return bad;
    if (n_flight_nodes < 1 || n_flight_nodes > HJB_DIST_MAX_NODES)
        return rfail(nullptr, HJB_E_INVALID, "%s: n_flight_nodes=%d not in 1..%d", who, n_flight_nodes, HJB_DIST_MAX_NODES);
    if (!flight_offsets) return rfail(nullptr, HJB_E_INVALID, "%s: null flight_offsets", who);
    if (!all_finite(flight_offsets, (int64_t)D * n_flight_nodes)) return rfail(nullptr, HJB_E_INVALID, "%s: flight_offsets is not finite", who);
    if (const int bad = check_weights(nullptr, who, n_flight_nodes, flight_weights)) return bad;
    LookHostProblem P;
    if (const int bad = look_host_model(who, a, mode, n_nodes, offsets, weights, P)) return bad;
    if (n_starts == 0) return HJB_OK;
    if (!stats) return rfail(nullptr, HJB_E_INVALID, "%s: null stats", who);
    if (const int bad = check_traj(nullptr, who, D, "D", n_steps, n_starts, X0, stats)) return bad;
    if (const int bad = check_campaign_bounds(nullptr, who, D, n_starts, threshold, tol)) return bad;
    // the flight set as hjb_rollout_set_noise forms it: the thresholds of the sampler and the mask of the axes with an offset
    std::vector<double> thr((size_t)std::max(n_flight_nodes - 1, 1));
    (void)noise_table(n_flight_nodes, flight_weights, thr.data());
    int fmask = 0;
    for (int w = 0; w < n_flight_nodes; ++w)
        for (int a = 0; a < D; ++a)
            if (flight_offsets[a + (int64_t)D * w] != 0.0) fmask |= 1 << a;
    double lo[HJB_MAX_D], hi[HJB_MAX_D];                      // the grid's extent: the first and the last knot of every axis
    for (int a = 0, at = 0; a < D; at += n[a], ++a) {
        lo[a] = knots[at];
        hi[a] = knots[at + n[a] - 1];
    }
    // one start at a time, and of it one sample at a time: its nodes, its visited states; the start's costs, final states and flags
    std::vector<int32_t> nodes((size_t)std::max(n_steps, 1));
    std::vector<double> path((size_t)D * ((size_t)n_steps + 1)), cost((size_t)n_samples), xf((size_t)D * (size_t)n_samples);
    std::vector<uint8_t> left((size_t)n_samples);
    with_bool(dtype == HJB_F32, [&](auto f) {
        with_dim(D, [&](auto d) {
            using TV = std::conditional_t<decltype(f)::value, float, double>;
            constexpr int DD = decltype(d)::value;
            for (int64_t s = 0; s < n_starts; ++s) {
                for (int64_t m = 0; m < n_samples; ++m) {
                    const uint64_t stream = (uint64_t)first_stream + (uint64_t)(s * n_samples + m);
                    uint32_t rw[4] = {0u, 0u, 0u, 0u};
                    for (int k = 0; k < n_steps; ++k)         // the kernel's own loop
                        nodes[k] = noise_step_node(seed, stream, k, rw, thr.data(), n_flight_nodes - 1);
                    lookahead_rollout_host<DD, TV>(P.M, P.L, knots, P.rdx.data(), u_table, static_cast<const TV *>(values), n_steps,
                                                   value_plane_of_step, 1, X0 + (int64_t)DD * s, nodes.data(), fmask, flight_offsets,
                                                   xf.data() + (int64_t)DD * m, cost.data() + m, path.data(), nullptr, nullptr, nullptr);
                    bool out = false;                         // path [1, D * (n_steps + 1)]: state k at path[a + D * k]
                    for (int64_t e = 0; e < (int64_t)DD * ((int64_t)n_steps + 1); ++e) out = out || campaign_outside(path[e], lo[e % DD], hi[e % DD]);
                    left[m] = out ? 1 : 0;
                }
                campaign_reduce_start(n_samples, DD, cost.data(), xf.data(), left.data(), threshold != nullptr, threshold ? threshold[s] : 0.0, tol,
                                      stats + HJB_CAMPAIGN_NSTAT * s);
            }
        });
    });
    return HJB_OK;
}

}  // extern "C"
