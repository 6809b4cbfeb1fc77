// rollout_ctrl_lookahead_host.hip - hjb_rollout_set_control_lookahead, hjb_rollout_run_control_lookahead,
// hjb_rollout_control_lookahead_host and hjb_rollout_run_control_lookahead_campaign (include/hjbdp.h): the host side of the lookahead
// under a control-dependent node set (K35, kernels_rollout_ctrl_lookahead.h / rollout_ctrl_lookahead.hip,
// rollout_ctrl_lookahead_fly.hip; K36, kernels_rollout_ctrl_lookahead_campaign.h / rollout_ctrl_lookahead_campaign.hip).
// The setter makes hjb_rollout_set_lookahead's refusals (check_lookahead) and hjb_set_control_disturbance's of the table's shape
// and size, and keeps the set beside - not in the place of - hjb_rollout_set_lookahead's.  The run function is the run functions'
// one frame and chunk loop (run_call) with K35's launch; the campaign is the campaigns' one frame and device loop
// (run_campaign_call) on the actuator plant (CampaignPlan::actuator) with K36's launch.  The host twin flies
// ctrl_lookahead_rollout_host (hjbdp_ctrl_lookahead.h) with no device.  No kernel is instantiated in this unit.
#include "rollout_host.h"
#include "kernels_rollout_ctrl_lookahead.h"
#include "kernels_rollout_ctrl_lookahead_campaign.h"
#include "rollout_dispatch.h"

using namespace hjbhost;

namespace {

// What the setter and the host twin refuse of the table itself, after check_lookahead, in `who`'s name (n_nodes >= 1): a label
// count other than n_labels - before the table is read: one of the wrong size is refused, not read past - a table over the cap,
// an entry that is not finite
int check_control_table(Rollout *ro, const char *who, const char *owner, int D, int32_t n_labels, int32_t n_nodes, int32_t n_controls,
                        const double *offsets) {
    if (n_controls != n_labels) return rfail(ro, HJB_E_INVALID, "%s: n_controls=%d, %s has %d labels", who, n_controls, owner, n_labels);
    if ((int64_t)D * n_nodes * n_labels > HJB_CTRL_DIST_MAX_ENTRIES)
        return rfail(ro, HJB_E_UNSUPPORTED, "%s: a table of %d x %d x %d entries is over the limit of 2^26", who, D, n_nodes, n_labels);
    for (int64_t c = 0; c < (int64_t)n_nodes * n_labels; ++c)
        for (int a = 0; a < D; ++a)
            if (!std::isfinite(offsets[a + (int64_t)D * c]))
                return rfail(ro, HJB_E_INVALID, "%s: offset of axis %d, node %d, control %lld is not finite", who, a, (int)(c % n_nodes),
                             (long long)(c / n_nodes));
    return HJB_OK;
}

// What both run functions refuse of the object under ro->mu: hjb_rollout_run_greedy's refusals (check_lookahead_run without a set
// of hjb_rollout_set_lookahead's, which is not read), no per-control set, a flown run with no actuator set
int check_control_lookahead_run(Rollout *ro, const char *who, int fly_noise, int32_t n_steps, const int32_t *planes, int64_t n_traj) {
    if (const int bad = check_lookahead_run(ro, who, 0, n_steps, planes, n_traj, false)) return bad;
    if (ro->CL.n_nodes < 1) return rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_control_lookahead", who);
    if (fly_noise && ro->Act.n_nodes < 1)
        return rfail(ro, HJB_E_INVALID, "rollout: %s with fly_noise=1 before hjb_rollout_set_actuator_noise", who);
    return HJB_OK;
}

}  // namespace

extern "C" {

int32_t hjb_rollout_set_control_lookahead(void *rollout, int32_t mode, int32_t n_nodes, int32_t n_controls, const double *offsets,
                                          const double *weights) {
    Rollout *ro = (Rollout *)rollout;
    const char *const who = "hjb_rollout_set_control_lookahead";
    // the arguments that need no object first, then the object; every refusal before any device work
    if (const int bad = check_lookahead(ro, who, 0, mode, n_nodes, offsets, weights)) return bad;
    if (n_controls < 0) return rfail(ro, HJB_E_INVALID, "%s: n_controls=%d", who, n_controls);
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "%s: null handle", who);
    std::lock_guard<std::mutex> g(ro->mu);
    const int D = ro->D, nl = ro->R.n_labels;
    if (n_nodes > 0)
        if (const int bad = check_control_table(ro, who, "the object", D, nl, n_nodes, n_controls, offsets)) return bad;
    CtrlLookSet L{};
    L.mode = mode;
    std::vector<double> tab(n_nodes > 0 ? (size_t)n_nodes * (1 + (size_t)D * nl) : 0);
    const int64_t n_tab = n_nodes > 0 ? ctrl_look_table(D, n_nodes, nl, offsets, weights, L, tab.data()) : 0;
    const void *d = nullptr;
    if (const int st = attach_table(ro, who, tab.data(), (size_t)n_tab * sizeof(double), n_nodes > 0, ro->ctrl_look, &d, "lookahead table"))
        return st;
    ro->CL = L;
    ro->CL.tab = (const double *)d;
    return HJB_OK;
}

int32_t hjb_rollout_run_control_lookahead(void *rollout, int32_t fly_noise, int32_t n_steps, const int32_t *value_plane_of_step,
                                          int64_t n_traj, const double *X0, uint64_t seed, int64_t first_stream, double *X_final,
                                          double *cost, double *X_path, double *U_path, double *L_path, double *V_path, double *W_path,
                                          double *device_ms) {
    const Rollout *ro = (const Rollout *)rollout;
    const char *const who = "hjb_rollout_run_control_lookahead";
    ChunkPlan plan = affine_plan(ro, who, n_steps, value_plane_of_step, n_traj, X0, X_final, cost, X_path, U_path, device_ms);
    plan.path[2] = {L_path, 1, n_steps};
    plan.path[3] = {V_path, 1, n_steps};
    plan.path[4] = {W_path, 1, n_steps};
    return run_call(
        rollout, plan,
        [&](Rollout *o) {
            if (fly_noise != 0 && fly_noise != 1) return rfail(o, HJB_E_INVALID, "%s: fly_noise=%d is not 0 or 1", who, fly_noise);
            if (!fly_noise && W_path) return rfail(o, HJB_E_INVALID, "%s: W_path given with fly_noise=0 (a nominal plant draws no node)", who);
            return fly_noise ? check_streams(o, who, n_traj, first_stream) : HJB_OK;
        },
        [&](Rollout *o) { return check_control_lookahead_run(o, who, fly_noise, n_steps, value_plane_of_step, n_traj); }, nullptr,
        [&](const Chunk &c) {
            DCtrlLook A{};
            A.G = greedy_of_chunk(ro, c);
            A.L = ro->CL;
            if (!fly_noise) return launch_rollout_ctrl_lookahead(ro->val_bytes, c.lds_on, plan.W, A, c.lds, c.st);
            A.N = ro->Act;                                    // the call's seed, the chunk's first stream and its W_path, as K33's launch
            A.N.seed = seed;
            A.N.first = (uint64_t)first_stream + (uint64_t)c.i0;
            A.N.Wp = c.path[4];
            A.N.terms = actuator_terms(plan.W, c.R.n_u, A.N.live, c.R.B);   // B of the model in effect at this run
            bool lds_on;
            const size_t lds = actuator_lds(ro, &lds_on);
            return launch_rollout_ctrl_lookahead_fly(ro->val_bytes, lds_on, plan.W, A, lds, c.st);
        });
}

int32_t hjb_rollout_control_lookahead_host(int32_t D, const int32_t *n, const double *knots, int32_t n_labels, int32_t n_u,
                                           const double *u_table, const double *A, const double *B, const double *c, const double *q,
                                           const double *r, int32_t dtype, int32_t n_value_planes, const void *values, int32_t n_steps,
                                           const int32_t *value_plane_of_step, int64_t n_traj, const double *X0, double *X_final,
                                           double *cost, double *X_path, double *U_path, double *L_path, double *V_path, int32_t mode,
                                           int32_t n_nodes, int32_t n_controls, const double *offsets, const double *weights,
                                           const int32_t *nodes, int32_t n_flight_nodes, const double *eps, const double *base) {
    const char *const who = "hjb_rollout_control_lookahead_host";
    const AffineHostArgs a{D, n, knots, n_labels, n_u, u_table, A, B, c, q, r, dtype, n_value_planes, values, n_steps, value_plane_of_step};
    if (const int bad = affine_host_args(who, a, n_traj)) return bad;
    if (const int bad = check_lookahead(nullptr, who, 0, mode, n_nodes, offsets, weights)) return bad;
    if (n_nodes < 1) return rfail(nullptr, HJB_E_INVALID, "%s: n_nodes=%d < 1 (the lookahead needs a node set)", who, n_nodes);
    if (const int bad = check_control_table(nullptr, who, "the problem", D, n_labels, n_nodes, n_controls, offsets)) return bad;
    if (nodes) {
        if (n_flight_nodes < 1 || n_flight_nodes > HJB_DIST_MAX_NODES)
            return rfail(nullptr, HJB_E_INVALID, "%s: n_flight_nodes=%d not in 1..%d", who, n_flight_nodes, HJB_DIST_MAX_NODES);
        if (!eps) return rfail(nullptr, HJB_E_INVALID, "%s: nodes given with null eps", who);
        if (!all_finite(eps, (int64_t)n_u * n_flight_nodes)) return rfail(nullptr, HJB_E_INVALID, "%s: eps is not finite", who);
        if (!all_finite(base, (int64_t)D * n_flight_nodes)) return rfail(nullptr, HJB_E_INVALID, "%s: base is not finite", who);
    }
    AffineHostProblem P;
    if (const int bad = affine_host_model(who, a, P)) return bad;
    CtrlLookSet L{};
    L.mode = mode;
    std::vector<double> tab((size_t)n_nodes * (1 + (size_t)D * n_labels));
    (void)ctrl_look_table(D, n_nodes, n_labels, offsets, weights, L, tab.data());
    L.tab = tab.data();
    if (n_traj == 0) return HJB_OK;
    const int bad_traj = check_traj(nullptr, who, D, "D", n_steps, n_traj, X0, X_final);
    if (bad_traj) return bad_traj;
    if (nodes)
        for (int64_t e = 0; e < n_traj * (int64_t)n_steps; ++e)
            if (nodes[e] < 0 || nodes[e] >= n_flight_nodes)
                return rfail(nullptr, HJB_E_INVALID, "%s: nodes element %lld = %d outside [0, %d)", who, (long long)e, nodes[e], n_flight_nodes);
    CtrlLookPlant plant{};                                    // the actuator set as hjb_rollout_set_actuator_noise forms it, and B's terms
    if (nodes) ctrl_look_plant(D, n_u, n_flight_nodes, eps, base, P.M.B, plant);
    with_bool(dtype == HJB_F32, [&](auto f) {
        with_dim(D, [&](auto d) {
            using TV = std::conditional_t<decltype(f)::value, float, double>;
            ctrl_lookahead_rollout_host<decltype(d)::value, TV>(P.M, L, knots, P.rdx.data(), u_table, static_cast<const TV *>(values), n_steps,
                                                                value_plane_of_step, n_traj, X0, nodes, plant, X_final, cost, X_path,
                                                                U_path, L_path, V_path);
        });
    });
    return HJB_OK;
}

int32_t hjb_rollout_run_control_lookahead_campaign(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_starts,
                                                   int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream,
                                                   const double *threshold, const double *tol, double *stats, double *device_ms) {
    const CampaignCall call{"hjb_rollout_run_control_lookahead_campaign", n_steps, n_starts, n_samples, X0, seed, first_stream, threshold, tol,
                            device_ms};
    CampaignPlan plan;
    plan.stats[0] = stats;
    plan.planes[0] = value_plane_of_step;
    plan.actuator = true;
    return run_campaign_call(
        rollout, call, plan, nullptr,
        [&](Rollout *ro) { return check_control_lookahead_run(ro, call.who, 1, n_steps, value_plane_of_step, n_starts); },
        [&](const CampaignLaunch &c) {
            const Rollout *ro = (const Rollout *)rollout;
            const DCtrlLookCampaignArgs K{c.R[0], ro->dvalues, ro->CL, c.Na, c.C[0], c.X0};
            return launch_rollout_ctrl_lookahead_campaign(ro->val_bytes, c.lds_on, ro->D, K, c.lds, c.st, c.stats[0]);
        });
}

}  // extern "C"
