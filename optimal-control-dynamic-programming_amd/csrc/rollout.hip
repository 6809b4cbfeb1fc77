// rollout.hip - hjb_rollout_* and hjb_attitude_linear_response: the host side of the batched closed-loop rollouts
// (include/hjbdp.h).  An object holds one stored policy (hjb_rollout_create) and one model, the last one set:
//   affine (K16, kernels_rollout.h / rollout_affine.hip), attitude (K17, kernels_rollout_attitude.h / rollout_attitude.hip),
//   and the three that attach two more objects' policies as channels (pos-att, position, simplified attitude): their setters
//   and run functions are rollout_channels.hip.
// The linear attitude controller (K21, kernels_rollout_attitude_linear.h / rollout_attitude_linear.hip) needs no object.
// Beside the model an object may hold a noise node set (hjb_rollout_set_noise): hjb_rollout_run_noisy (K25,
// kernels_rollout_noisy.h / rollout_noisy.hip) flies the affine loop under it, and no other run function reads it.  The sampler's
// host twins hjb_rollout_noise_table / hjb_rollout_noise_draw (hjbdp_noise.h) need no device.
// And an actuator node set (hjb_rollout_set_actuator_noise): hjb_rollout_run_actuator (K33, kernels_rollout_actuator.h /
// rollout_actuator.hip) flies the affine loop under u (1 + eps_w) (+ an additive base) on K25's streams, and
// hjb_rollout_run_actuator_campaign (K34, rollout_campaign_host.hip) reduces those flights; no other run function reads it.
// And it may hold value planes (hjb_rollout_set_values): hjb_rollout_run_greedy (K26, kernels_rollout_greedy.h /
// rollout_greedy.hip) flies the affine loop by one-step lookahead on them, and no other run function reads them.  Its host twin
// hjb_rollout_greedy_host (hjbdp_greedy.h) needs no device and no object.
// And a lookahead node set (hjb_rollout_set_lookahead): hjb_rollout_run_lookahead (K27, kernels_rollout_lookahead.h /
// rollout_lookahead.hip, rollout_lookahead_fly.hip) flies the affine loop by lookahead under that set, on a nominal plant or under
// the noise set, and no other run function reads it.  Its host twin hjb_rollout_lookahead_host (hjbdp_lookahead.h) needs no device.
// And hjb_rollout_run_campaign (K28, kernels_rollout_campaign.h / rollout_campaign.hip) reduces the noisy flights of the stored labels
// per start on the device; its host side and the host reduce hjb_rollout_campaign_reduce are rollout_campaign_host.hip.
// hjb_rollout_run_lookahead_campaign (K29, kernels_rollout_lookahead_campaign.h) does the same for the lookahead controller; it and
// its host twin are rollout_lookahead_campaign_host.hip, on check_lookahead_run and look_host_args / look_host_model below.
// And a per-control lookahead node set (hjb_rollout_set_control_lookahead): hjb_rollout_run_control_lookahead (K35) and its
// campaign (K36) fly the affine loop by lookahead under it, on a nominal plant or under the actuator set; no other run function
// reads it.  They, the setter and the host twin are rollout_ctrl_lookahead_host.hip.
// Defined here for the host units (rollout_host.h): rfail, check_run / check_traj / check_quaternions (the run functions'
// refusals, all before any device work), check_lookahead, upload, attach_table (the table setters' tail), affine_plan and
// greedy_of_chunk (the affine run functions' plan and record), run_chunks (the chunk loop) and run_call (the run functions' entry
// frame: every run function here, in rollout_channels.hip and in rollout_ctrl_lookahead_host.hip is its plan, its hooks and its
// launch).  No kernel is instantiated in this unit.
#include "rollout_host.h"
#include "rollout_dispatch.h"
#include "kernels_rollout_attitude_linear.h"
#include "kernels_rollout_greedy.h"
#include "kernels_rollout_lookahead.h"

using namespace hjbhost;

namespace {

void release(Rollout *ro) {
    ro->att.reset();
    ro->noise.reset();
    ro->actuator.reset();
    ro->values.reset();
    ro->look.reset();
    ro->ctrl_look.reset();
    ro->data.reset();
    if (ro->stream) (void)hipStreamDestroy(ro->stream);
    ro->stream = nullptr;
}

template <typename TL>
int64_t first_bad_label(const void *labels, int64_t count, int64_t lo, int64_t hi) {
    const TL *l = static_cast<const TL *>(labels);
    for (int64_t i = 0; i < count; ++i)
        if ((int64_t)l[i] < lo || (int64_t)l[i] >= hi) return i;
    return -1;
}

// a pos-att, position or simplified attitude model goes, and with it its hold on the other two channels
void drop_attached(Rollout *ro) {
    if (!ro->att) return;
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    ro->att.reset();
}

// What hjb_rollout_create (who: "rollout") and hjb_rollout_greedy_host (its own name) refuse of a grid: an axis of fewer than two
// knots, a knot that is not finite, knots not strictly increasing, sizes that overflow.  -> the states and the knots of all axes
int check_grid(const char *who, int D, const int32_t *n, const double *knots, int64_t *nS_out, int64_t *n_knots_out) {
    int64_t nS = 1, n_knots = 0;
    for (int a = 0; a < D; ++a) {
        if (n[a] < 2) return rfail(nullptr, HJB_E_INVALID, "%s: axis %d has %d knots (need >= 2)", who, a, n[a]);
        const double *kk = knots + n_knots;
        for (int i = 0; i < n[a]; ++i)
            if (!std::isfinite(kk[i])) return rfail(nullptr, HJB_E_INVALID, "%s: knot %d of axis %d is not finite", who, i, a);
        for (int i = 0; i + 1 < n[a]; ++i)
            if (!(kk[i + 1] > kk[i])) return rfail(nullptr, HJB_E_INVALID, "%s: knots of axis %d not strictly increasing (at %d)", who, a, i);
        n_knots += n[a];
        if (n_knots > INT32_MAX || nS > kMaxStates / n[a]) return rfail(nullptr, HJB_E_INVALID, "%s: size overflow (grid)", who);
        nS *= n[a];
    }
    *nS_out = nS;
    *n_knots_out = n_knots;
    return HJB_OK;
}

}  // namespace

namespace hjbhost {

// What hjb_rollout_set_lookahead and hjb_rollout_lookahead_host refuse of a lookahead node set, hjb_set_disturbance's refusals, in
// `who`'s name (D < 1: the offsets are left to the caller, who knows D).  HJB_OK otherwise.
int check_lookahead(Rollout *ro, const char *who, int D, int32_t mode, int32_t n_nodes, const double *offsets, const double *weights) {
    if (mode != HJB_DIST_EXPECT && mode != HJB_DIST_WORST)
        return rfail(ro, HJB_E_INVALID, "%s: mode %d is not HJB_DIST_EXPECT / HJB_DIST_WORST", who, mode);
    if (n_nodes < 0 || n_nodes > HJB_DIST_MAX_NODES) return rfail(ro, HJB_E_INVALID, "%s: n_nodes=%d not in 0..%d", who, n_nodes, HJB_DIST_MAX_NODES);
    if (n_nodes > 0 && !offsets) return rfail(ro, HJB_E_INVALID, "%s: null offsets with n_nodes=%d", who, n_nodes);
    if (n_nodes > 0 && weights && mode == HJB_DIST_WORST) return rfail(ro, HJB_E_INVALID, "%s: weights given with HJB_DIST_WORST", who);
    for (int w = 0; weights && w < n_nodes; ++w)
        if (!std::isfinite(weights[w]) || weights[w] < 0) return rfail(ro, HJB_E_INVALID, "%s: weight %d is not finite or is negative", who, w);
    for (int w = 0; w < n_nodes; ++w)
        for (int a = 0; a < D; ++a)
            if (!std::isfinite(offsets[a + (int64_t)D * w])) return rfail(ro, HJB_E_INVALID, "%s: offset of axis %d, node %d is not finite", who, a, w);
    return HJB_OK;
}

int rfail(Rollout *ro, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ro) ro->err = buf;
    g_last_error = buf;
    return code;
}

bool all_finite(const double *p, int64_t n) { return !p || first_nonfinite(p, n, true) < 0; }

int check_run(Rollout *ro, int want, int method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj) {
    if (method != HJB_LOOKUP_NEAREST && method != HJB_LOOKUP_LINEAR) return rfail(ro, HJB_E_INVALID, "rollout: method %d", method);
    if (n_steps < 0) return rfail(ro, HJB_E_INVALID, "rollout: n_steps=%d < 0", n_steps);
    if (n_traj < 0) return rfail(ro, HJB_E_INVALID, "rollout: n_traj=%lld < 0", (long long)n_traj);
    static const struct { const char *held, *setter, *runner; } names[] = {
        {"", "", ""},
        {"affine", "hjb_rollout_set_model", "hjb_rollout_run"},
        {"attitude", "hjb_rollout_set_attitude_model", "hjb_rollout_run_attitude"},
        {"pos-att", "hjb_rollout_set_pos_att_model", "hjb_rollout_run_pos_att"},
        {"position", "hjb_rollout_set_position_model", "hjb_rollout_run_position"},
        {"simplified attitude", "hjb_rollout_set_attitude_simplified_model", "hjb_rollout_run_attitude_simplified"}};
    if (ro->model == kModelNone) return rfail(ro, HJB_E_INVALID, "rollout: run before %s", names[want].setter);
    if (ro->model != want)
        return rfail(ro, HJB_E_INVALID, "rollout: the object holds the %s model (%s): call %s", names[ro->model].held,
                     names[ro->model].setter, names[ro->model].runner);
    if (n_steps > 0 && !plane_of_step) return rfail(ro, HJB_E_INVALID, "rollout: null plane_of_step");
    // att is set exactly while the model is one of the three attaching ones: their setters install it with the model
    // (install_attached), every other setter ends in drop_attached.  A new setter has to do one or the other.
    const int n_planes = ro->att ? ro->att->n_planes : ro->n_planes;
    for (int k = 0; k < n_steps; ++k)
        if (plane_of_step[k] < 0 || plane_of_step[k] >= n_planes)
            return rfail(ro, HJB_E_INVALID, "rollout: plane_of_step[%d] = %d outside [0, %d)", k, plane_of_step[k], n_planes);
    return HJB_OK;
}

int check_traj(Rollout *ro, const char *pre, int W, const char *wname, int32_t n_steps, int64_t n_traj, const double *X0,
               const double *X_final) {
    if (!X0 || !X_final) return rfail(ro, HJB_E_INVALID, "%s: null X0 / X_final", pre);
    if (n_traj > INT64_MAX / (W * ((int64_t)n_steps + 1)) / 8)
        return rfail(ro, HJB_E_INVALID, "%s: size overflow (n_traj x %s x n_steps)", pre, wname);
    const int64_t bad = first_nonfinite(X0, (int64_t)W * n_traj, true);
    if (bad >= 0) return rfail(ro, HJB_E_INVALID, "%s: X0 element %lld is not finite", pre, (long long)bad);
    return HJB_OK;
}

int check_quaternions(Rollout *ro, const char *pre, int64_t n_traj, const double *X0) {
    for (int64_t i = 0; i < n_traj; ++i) {
        const double *q = X0 + HJB_ATT_W * i + 3;
        if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0)
            return rfail(ro, HJB_E_INVALID, "%s: X0 column %lld has an all-zero quaternion (0/0 at the first renormalisation)", pre,
                         (long long)i);
    }
    return HJB_OK;
}

// What hjb_rollout_set_noise and hjb_rollout_noise_table refuse of a weight vector (null: equal weights), said in `who`'s name:
// a weight that is not finite or is negative, weights that sum to 0.  HJB_OK otherwise.
int check_weights(Rollout *ro, const char *who, int32_t n_nodes, const double *weights) {
    if (!weights) return HJB_OK;
    double sum = 0.0;
    for (int w = 0; w < n_nodes; ++w) {
        if (!std::isfinite(weights[w]) || weights[w] < 0) return rfail(ro, HJB_E_INVALID, "%s: weight %d is not finite or is negative", who, w);
        sum = sum + weights[w];
    }
    if (!(sum > 0) || !std::isfinite(sum)) return rfail(ro, HJB_E_INVALID, "%s: the %d weights sum to 0 (or their sum overflows)", who, n_nodes);
    return HJB_OK;
}

int check_lookahead_run(Rollout *ro, const char *who, int fly_noise, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_traj,
                        bool own_set) {
    if (n_steps < 0) return rfail(ro, HJB_E_INVALID, "rollout: n_steps=%d < 0", n_steps);
    if (n_traj < 0) return rfail(ro, HJB_E_INVALID, "rollout: n_traj=%lld < 0", (long long)n_traj);
    if (ro->model == kModelNone) return rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_model", who);
    if (ro->model != kModelAffine)
        return rfail(ro, HJB_E_INVALID, "rollout: %s needs the affine model (hjb_rollout_set_model); the object holds another", who);
    if (own_set && ro->L.n_nodes < 1) return rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_lookahead", who);
    if (fly_noise && ro->N.n_nodes < 1) return rfail(ro, HJB_E_INVALID, "rollout: %s with fly_noise=1 before hjb_rollout_set_noise", who);
    if (n_steps > 0 && !value_plane_of_step) return rfail(ro, HJB_E_INVALID, "rollout: null value_plane_of_step");
    for (int k = 0; k < n_steps; ++k) {
        const int32_t p = value_plane_of_step[k];
        if (p >= 0 && ro->val_planes < 1)
            return rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_values (value_plane_of_step[%d] = %d; only -1 needs no values)",
                         who, k, p);
        if (p < -1 || p >= ro->val_planes)
            return rfail(ro, HJB_E_INVALID, "rollout: value_plane_of_step[%d] = %d outside [-1, %d)", k, p, ro->val_planes);
    }
    return HJB_OK;
}

int affine_host_args(const char *who, const AffineHostArgs &a, int64_t n_traj) {
    if (a.D < 1 || a.D > HJB_MAX_D) return rfail(nullptr, HJB_E_UNSUPPORTED, "%s: D=%d not in 1..%d", who, a.D, HJB_MAX_D);
    if (a.n_u < 1 || a.n_u > HJB_ROLLOUT_MAX_U) return rfail(nullptr, HJB_E_UNSUPPORTED, "%s: n_u=%d not in 1..%d", who, a.n_u, HJB_ROLLOUT_MAX_U);
    if (!a.n || !a.knots || !a.u_table || !a.A || !a.B)
        return rfail(nullptr, HJB_E_INVALID, "%s: null argument (n, knots, u_table, A and B are required)", who);
    if (a.n_labels < 1) return rfail(nullptr, HJB_E_INVALID, "%s: n_labels=%d < 1", who, a.n_labels);
    if (a.dtype != HJB_F32 && a.dtype != HJB_F64) return rfail(nullptr, HJB_E_INVALID, "%s: dtype %d is not HJB_F32 / HJB_F64", who, a.dtype);
    if (a.n_value_planes < 0) return rfail(nullptr, HJB_E_INVALID, "%s: n_value_planes=%d < 0", who, a.n_value_planes);
    if (a.n_value_planes > 0 && !a.values) return rfail(nullptr, HJB_E_INVALID, "%s: null values with n_value_planes=%d", who, a.n_value_planes);
    if (a.n_steps < 0 || n_traj < 0)
        return rfail(nullptr, HJB_E_INVALID, "%s: n_steps=%d, n_traj=%lld (both >= 0)", who, a.n_steps, (long long)n_traj);
    return HJB_OK;
}

int affine_host_model(const char *who, const AffineHostArgs &a, AffineHostProblem &P) {
    const int D = a.D, n_u = a.n_u;
    int64_t nS = 1, n_knots = 0;
    if (const int bad_grid = check_grid(who, D, a.n, a.knots, &nS, &n_knots)) return bad_grid;
    if (!all_finite(a.u_table, (int64_t)a.n_labels * n_u)) return rfail(nullptr, HJB_E_INVALID, "%s: u_table is not finite", who);
    if (!all_finite(a.A, (int64_t)D * D) || !all_finite(a.B, (int64_t)D * n_u) || !all_finite(a.c, D) || !all_finite(a.q, D) || !all_finite(a.r, n_u))
        return rfail(nullptr, HJB_E_INVALID, "%s: the model (A, B, c, q, r) is not finite", who);
    if (a.n_steps > 0 && !a.value_plane_of_step) return rfail(nullptr, HJB_E_INVALID, "%s: null value_plane_of_step", who);
    for (int k = 0; k < a.n_steps; ++k)
        if (a.value_plane_of_step[k] < -1 || a.value_plane_of_step[k] >= a.n_value_planes)
            return rfail(nullptr, HJB_E_INVALID, "%s: value_plane_of_step[%d] = %d outside [-1, %d)", who, k, a.value_plane_of_step[k],
                         a.n_value_planes);
    GreedyModel &M = P.M;
    P.rdx.assign((size_t)n_knots, 0.0);
    greedy_grid(D, a.n, a.knots, M, P.rdx.data());
    M.n_u = n_u;
    M.n_labels = a.n_labels;
    M.has_c = a.c ? 1 : 0;
    std::memcpy(M.A, a.A, sizeof(double) * D * D);
    std::memcpy(M.B, a.B, sizeof(double) * D * n_u);
    if (a.c) std::memcpy(M.c, a.c, sizeof(double) * D);
    if (a.q) std::memcpy(M.q, a.q, sizeof(double) * D);
    if (a.r) std::memcpy(M.r, a.r, sizeof(double) * n_u);
    return HJB_OK;
}

int look_host_args(const char *who, const AffineHostArgs &a, int64_t n_traj, int32_t mode, int32_t n_nodes, const double *offsets,
                   const double *weights) {
    if (const int bad = affine_host_args(who, a, n_traj)) return bad;
    if (const int bad = check_lookahead(nullptr, who, a.D, mode, n_nodes, offsets, weights)) return bad;
    if (n_nodes < 1) return rfail(nullptr, HJB_E_INVALID, "%s: n_nodes=%d < 1 (the lookahead needs a node set)", who, n_nodes);
    return HJB_OK;
}

int look_host_model(const char *who, const AffineHostArgs &a, int32_t mode, int32_t n_nodes, const double *offsets, const double *weights,
                    LookHostProblem &P) {
    if (const int bad = affine_host_model(who, a, P)) return bad;
    P.L.mode = mode;
    P.tab.assign((size_t)n_nodes * (1 + a.D), 0.0);
    (void)look_table(a.D, n_nodes, offsets, weights, P.L, P.tab.data());
    P.L.tab = P.tab.data();
    return HJB_OK;
}

int check_streams(Rollout *ro, const char *who, int64_t n_traj, int64_t first_stream) {
    if (first_stream < 0) return rfail(ro, HJB_E_INVALID, "%s: first_stream=%lld < 0", who, (long long)first_stream);
    if (n_traj > 0 && first_stream > INT64_MAX - n_traj)
        return rfail(ro, HJB_E_INVALID, "%s: first_stream + n_traj overflows (%lld + %lld)", who, (long long)first_stream, (long long)n_traj);
    return HJB_OK;
}

size_t noisy_lds(const Rollout *ro, bool *on) {
    const size_t lds = (size_t)(2 * (int64_t)ro->R.n_knots + (int64_t)ro->R.n_labels * ro->R.n_u + ro->N.n_tab) * sizeof(double);
    *on = ro->lds && lds <= kLdsMax;
    return lds;
}

size_t actuator_lds(const Rollout *ro, bool *on) {
    const size_t lds = (size_t)(2 * (int64_t)ro->R.n_knots + (int64_t)ro->R.n_labels * ro->R.n_u + ro->Act.n_tab) * sizeof(double);
    *on = ro->lds && lds <= kLdsMax;
    return lds;
}

DAttitude euler_attitude(double J1, double J2, double J3, double h) {
    DAttitude A{};
    A.h = h;
    A.J[0] = J1;
    A.J[1] = J2;
    A.J[2] = J3;
    A.c[0] = (J2 - J3) / J1;                          // spacecraft_dynamics_list :600-620
    A.c[1] = (J3 - J1) / J2;
    A.c[2] = (J1 - J2) / J3;
    return A;
}

int upload(Rollout *ro, DevData &dd, const void *src, size_t bytes, const void **out) {
    void *d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(bytes, 16)) != hipSuccess) return rfail(ro, HJB_E_NOMEM, "rollout: hipMalloc of %zu bytes failed", bytes);
    dd.allocs.push_back(d);
    if (bytes && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "rollout: upload failed");
    *out = d;
    return HJB_OK;
}

int run_chunks(Rollout *ro, const ChunkPlan &plan, const std::function<hipError_t(const Chunk &)> &launch) {
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(ro->device) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipSetDevice failed");
    const int W = plan.W;
    const int32_t n_steps = plan.n_steps;
    const int64_t n_traj = plan.n_traj, nc_max = std::min(n_traj, ro->chunk);
    const size_t xb = (size_t)nc_max * W * sizeof(double);
    const size_t cb = plan.cost ? (size_t)nc_max * sizeof(double) : 0;
    const size_t pb = (size_t)std::max(n_steps, 1) * sizeof(int32_t);
    const size_t fb = plan.flags ? (size_t)nc_max * sizeof(int32_t) : 0;
    size_t rows[kMaxPaths], pathb[kMaxPaths], need = 2 * xb + cb + pb + fb;     // rows: doubles per trajectory of a path asked for
    for (int p = 0; p < kMaxPaths; ++p) {
        rows[p] = plan.path[p].host ? (size_t)plan.path[p].rows * (size_t)plan.path[p].stages : 0;
        pathb[p] = (size_t)nc_max * rows[p] * sizeof(double);
        need += pathb[p];
    }
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipMemGetInfo failed");
    if (need + ((size_t)64 << 20) > fr)
        return rfail(ro, HJB_E_NOMEM, "rollout: a chunk of %lld trajectories needs %zu bytes, %zu free (lower option \"chunk\")",
                     (long long)nc_max, need, fr);
    std::vector<void *> bufs;
    auto done = [&](int code) {
        for (void *p : bufs) (void)hipFree(p);
        return code;
    };
    size_t failed = 0;                                        // the bytes of the allocation that failed
    auto dev = [&](size_t bytes) -> void * {                  // null for no bytes, and after a failure
        void *d = nullptr;
        if (!bytes || failed) return d;
        if (hipMalloc(&d, bytes) == hipSuccess) bufs.push_back(d);
        else failed = bytes;
        return d;
    };
    Chunk c{};
    double *const dX0 = (double *)dev(xb);
    c.X0 = dX0;
    c.Xf = (double *)dev(xb);
    c.cost = (double *)dev(cb);
    c.path[0] = (double *)dev(pathb[0]);
    c.path[1] = (double *)dev(pathb[1]);
    int32_t *const dplane = (int32_t *)dev(pb);
    for (int p = 2; p < kMaxPaths; ++p) c.path[p] = (double *)dev(pathb[p]);
    c.flags = (int32_t *)dev(fb);
    int32_t *din[kMaxInputs];
    for (int t = 0; t < kMaxInputs; ++t) c.input[t] = din[t] = (int32_t *)dev(plan.input[t] ? (size_t)nc_max * sizeof(int32_t) : 0);
    if (failed) return done(rfail(ro, HJB_E_NOMEM, "rollout: hipMalloc of %zu bytes failed", failed));
    hipStream_t st = c.st = ro->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess && n_steps > 0 && plan.plane_of_step) e = hipMemcpyAsync(dplane, plan.plane_of_step, pb, hipMemcpyHostToDevice, st);
    c.R = ro->R;
    c.R.plane_of_step = dplane;
    c.R.n_steps = n_steps;
    c.lds = (size_t)(2 * (int64_t)c.R.n_knots + (int64_t)c.R.n_labels * c.R.n_u) * sizeof(double);
    c.lds_on = ro->lds && c.lds <= kLdsMax;
    double ms_total = 0;
    for (int64_t i0 = 0; e == hipSuccess && i0 < n_traj; i0 += nc_max) {
        const int64_t nc = std::min(nc_max, n_traj - i0);
        c.i0 = i0;
        c.nc = nc;
        e = hipMemcpyAsync(dX0, plan.X0 + W * i0, (size_t)nc * W * sizeof(double), hipMemcpyHostToDevice, st);
        for (int t = 0; e == hipSuccess && t < kMaxInputs; ++t)
            if (din[t]) e = hipMemcpyAsync(din[t], plan.input[t] + i0, (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        (void)hipEventRecord(e0, st);
        e = launch(c);
        if (e != hipSuccess) break;
        (void)hipEventRecord(e1, st);
        e = hipMemcpyAsync(plan.X_final + W * i0, c.Xf, (size_t)nc * W * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && plan.cost) e = hipMemcpyAsync(plan.cost + i0, c.cost, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && plan.flags) e = hipMemcpyAsync(plan.flags + i0, c.flags, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        // paths: [nc, rows] on the device -> columns i0 .. i0+nc of [n_traj, rows] on the host
        for (int p = 0; e == hipSuccess && p < kMaxPaths; ++p)
            if (rows[p])
                e = hipMemcpy2DAsync(plan.path[p].host + i0, (size_t)n_traj * sizeof(double), c.path[p], (size_t)nc * sizeof(double),
                                     (size_t)nc * sizeof(double), rows[p], hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        ms_total += ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return done(rfail(ro, HJB_E_DEVICE, "%s: %s", plan.who, hipGetErrorString(e)));
    }
    if (plan.device_ms) *plan.device_ms = ms_total;
    return done(HJB_OK);
}

int run_call(void *rollout, const ChunkPlan &plan, const std::function<int(Rollout *)> &no_object, const std::function<int(Rollout *)> &controller,
             const std::function<int(Rollout *)> &starts, const std::function<hipError_t(const Chunk &)> &launch) {
    Rollout *ro = (Rollout *)rollout;
    if (no_object)
        if (const int bad = no_object(ro)) return bad;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    if (const int bad = controller(ro)) return bad;
    if (plan.n_traj == 0) {
        if (plan.device_ms) *plan.device_ms = 0.0;
        return HJB_OK;
    }
    if (const int bad = check_traj(ro, "rollout", plan.W, plan.wname, plan.n_steps, plan.n_traj, plan.X0, plan.X_final)) return bad;
    if (starts)
        if (const int bad = starts(ro)) return bad;
    if (plan.device_ms) *plan.device_ms = 0.0;
    return run_chunks(ro, plan, launch);
}

// The plan every run function of the affine model starts from: D doubles of state, X_path and U_path, the cost.  D and n_u are
// fixed by hjb_rollout_create, so they are read without the lock; of a null handle, which run_call refuses, nothing is read.
ChunkPlan affine_plan(const Rollout *ro, const char *who, int32_t n_steps, const int32_t *planes, int64_t n_traj, const double *X0,
                      double *X_final, double *cost, double *X_path, double *U_path, double *device_ms) {
    const int D = ro ? ro->D : 0;
    ChunkPlan plan{{who, D, "D", n_steps, planes, n_traj, X0, X_final, device_ms}};
    plan.path[0] = {X_path, D, n_steps + 1};
    plan.path[1] = {U_path, ro ? ro->R.n_u : 0, n_steps};
    plan.cost = cost;
    return plan;
}

// The greedy part of a chunk's launch record (hjb_rollout_run_greedy, hjb_rollout_run_lookahead): paths 0 .. 3 are X, U, L, V
DGreedy greedy_of_chunk(const Rollout *ro, const Chunk &c) {
    DGreedy G{};
    G.R = c.R;
    G.values = ro->dvalues;
    G.nc = c.nc;
    G.X0 = c.X0;
    G.Xf = c.Xf;
    G.cost = c.cost;
    G.Xp = c.path[0];
    G.Up = c.path[1];
    G.Lp = c.path[2];
    G.Vp = c.path[3];
    return G;
}

}  // namespace hjbhost

namespace {

// The object's noise set for a chunk of a call: the call's seed, the chunk's first stream - streams count through the call - and
// its W_path
DNoise noise_of_chunk(const Rollout *ro, const Chunk &c, uint64_t seed, int64_t first_stream, double *Wp) {
    DNoise N = ro->N;
    N.seed = seed;
    N.first = (uint64_t)first_stream + (uint64_t)c.i0;
    N.Wp = Wp;
    return N;
}

}  // namespace

namespace hjbhost {

// The shared tail of hjb_rollout_set_noise, _set_values, _set_lookahead and _set_control_lookahead, under ro->mu: `bytes` at src go to the object's device
// in a DevData of their own (any false: no table, the set is detached), and once the object's stream is idle `holder` takes it,
// which releases a table given earlier.  -> *dev, the table on the device (null for none); the caller's record fields follow
// HJB_OK.  `big`: how the HJB_E_NOMEM refusal calls a table large enough to be checked against the free memory first (null: none is).
int attach_table(Rollout *ro, const char *who, const void *src, size_t bytes, bool any, std::shared_ptr<DevData> &holder, const void **dev,
                 const char *big) {
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(ro->device) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipSetDevice failed");
    std::shared_ptr<DevData> nd;
    *dev = nullptr;
    if (any) {
        size_t fr = 0, tot = 0;
        if (big && hipMemGetInfo(&fr, &tot) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipMemGetInfo failed");
        if (big && bytes + ((size_t)64 << 20) > fr)
            return rfail(ro, HJB_E_NOMEM, "%s: %zu bytes of %s, %zu free on device %d", who, bytes, big, fr, ro->device);
        nd = std::make_shared<DevData>(ro->device);
        if (const int st = upload(ro, *nd, src, bytes, dev)) return st;
    }
    if (ro->stream) (void)hipStreamSynchronize(ro->stream);
    holder = std::move(nd);
    return HJB_OK;
}

}  // namespace hjbhost

extern "C" {

int32_t hjb_rollout_create(int32_t device, int32_t D, const int32_t *n, const double *knots, int32_t idx_dtype,
                           int32_t index_base, int32_t n_planes, const void *labels, int32_t n_labels, int32_t n_u,
                           const double *u_table, void **rollout_out) {
    if (!n || !knots || !labels || !u_table || !rollout_out) return rfail(nullptr, HJB_E_INVALID, "rollout: null argument");
    *rollout_out = nullptr;
    if (D < 1 || D > HJB_MAX_D) return rfail(nullptr, HJB_E_UNSUPPORTED, "rollout: D=%d not in 1..%d", D, HJB_MAX_D);
    if (n_u < 1 || n_u > HJB_ROLLOUT_MAX_U) return rfail(nullptr, HJB_E_UNSUPPORTED, "rollout: n_u=%d not in 1..%d", n_u, HJB_ROLLOUT_MAX_U);
    int idx_bytes = 0;
    if (idx_dtype == HJB_IDX_I32) idx_bytes = 4;
    else if (idx_dtype == HJB_IDX_U8) idx_bytes = 1;
    else if (idx_dtype == HJB_IDX_U16) idx_bytes = 2;
    else return rfail(nullptr, HJB_E_INVALID, "rollout: idx_dtype %d is not HJB_IDX_I32 / _U8 / _U16", idx_dtype);
    if (index_base != 0 && index_base != 1) return rfail(nullptr, HJB_E_INVALID, "rollout: index_base %d (0 or 1)", index_base);
    if (n_planes < 1) return rfail(nullptr, HJB_E_INVALID, "rollout: n_planes=%d < 1", n_planes);
    if (n_labels < 1) return rfail(nullptr, HJB_E_INVALID, "rollout: n_labels=%d < 1", n_labels);
    int64_t nS = 1, n_knots = 0;
    if (const int bad_grid = check_grid("rollout", D, n, knots, &nS, &n_knots)) return bad_grid;
    if ((int64_t)n_planes > kMaxStates / nS) return rfail(nullptr, HJB_E_INVALID, "rollout: size overflow (%lld states x %d planes)", (long long)nS, n_planes);
    const int64_t n_lab = nS * n_planes;
    const int64_t n_ut = (int64_t)n_labels * n_u;
    const int64_t bad_u = first_nonfinite(u_table, n_ut, true);
    if (bad_u >= 0) return rfail(nullptr, HJB_E_INVALID, "rollout: u_table element %lld is not finite", (long long)bad_u);
    const int64_t lo = index_base, hi = (int64_t)index_base + n_labels;
    const int64_t bad = idx_bytes == 4 ? first_bad_label<int32_t>(labels, n_lab, lo, hi)
                      : idx_bytes == 2 ? first_bad_label<uint16_t>(labels, n_lab, lo, hi)
                                       : first_bad_label<uint8_t>(labels, n_lab, lo, hi);
    if (bad >= 0) {
        const int64_t v = idx_bytes == 4 ? ((const int32_t *)labels)[bad] : idx_bytes == 2 ? ((const uint16_t *)labels)[bad] : ((const uint8_t *)labels)[bad];
        return rfail(nullptr, HJB_E_INVALID, "rollout: label %lld at flat position %lld (state %lld, plane %lld) outside [%lld, %lld)",
                     (long long)v, (long long)bad, (long long)(bad % nS), (long long)(bad / nS), (long long)lo, (long long)hi);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return rfail(nullptr, HJB_E_DEVICE, "no HIP device visible (libhjbdp has no CPU fallback)");
    if (device < 0 || device >= ndev) return rfail(nullptr, HJB_E_INVALID, "rollout: device %d", device);

    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(device) != hipSuccess) return rfail(nullptr, HJB_E_DEVICE, "hipSetDevice failed");
    const size_t lab_bytes = (size_t)n_lab * idx_bytes, tab_bytes = (size_t)(2 * n_knots + n_ut) * sizeof(double);
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return rfail(nullptr, HJB_E_DEVICE, "hipMemGetInfo failed");
    if (lab_bytes + tab_bytes + ((size_t)64 << 20) > fr)
        return rfail(nullptr, HJB_E_NOMEM, "rollout: %zu bytes of labels and tables, %zu free on device %d", lab_bytes + tab_bytes, fr, device);

    Rollout *ro = new Rollout;
    ro->device = device;
    ro->D = D;
    ro->idx_bytes = idx_bytes;
    ro->n_planes = n_planes;
    ro->data = std::make_shared<DevData>(device);
    DRollout &R = ro->R;
    R.n_u = n_u;
    R.n_labels = n_labels;
    R.index_base = index_base;
    std::vector<double> rdx((size_t)n_knots);
    greedy_grid(D, n, knots, R, rdx.data());                  // the grid description and 1/dx, as hjb_policy_lookup builds it
    for (int a = 0; a < D; ++a) {
        ro->grid_lo[a] = knots[R.koff[a]];
        ro->grid_hi[a] = knots[R.koff[a] + n[a] - 1];
    }
    int st = upload(ro, *ro->data, knots, (size_t)n_knots * sizeof(double), (const void **)&R.knots);
    if (!st) st = upload(ro, *ro->data, rdx.data(), rdx.size() * sizeof(double), (const void **)&R.rdx);
    if (!st) st = upload(ro, *ro->data, u_table, (size_t)n_ut * sizeof(double), (const void **)&R.u_table);
    if (!st) st = upload(ro, *ro->data, labels, lab_bytes, &R.labels);
    if (!st && hipStreamCreateWithFlags(&ro->stream, hipStreamNonBlocking) != hipSuccess) st = rfail(ro, HJB_E_DEVICE, "rollout: stream creation failed");
    if (st) {
        release(ro);
        delete ro;
        return st;
    }
    *rollout_out = ro;
    return HJB_OK;
}

int32_t hjb_rollout_set_model(void *rollout, const double *A, const double *B, const double *c, const double *q, const double *r) {
    Rollout *ro = (Rollout *)rollout;
    if (!ro || !A || !B) return rfail(ro, HJB_E_INVALID, "rollout: null argument (A and B are required)");
    std::lock_guard<std::mutex> g(ro->mu);
    const int D = ro->D, nu = ro->R.n_u;
    if (!all_finite(A, (int64_t)D * D)) return rfail(ro, HJB_E_INVALID, "rollout: A is not finite");
    if (!all_finite(B, (int64_t)D * nu)) return rfail(ro, HJB_E_INVALID, "rollout: B is not finite");
    if (!all_finite(c, D)) return rfail(ro, HJB_E_INVALID, "rollout: c is not finite");
    if (!all_finite(q, D)) return rfail(ro, HJB_E_INVALID, "rollout: q is not finite");
    if (!all_finite(r, nu)) return rfail(ro, HJB_E_INVALID, "rollout: r is not finite");
    DRollout &R = ro->R;
    std::memset(R.A, 0, sizeof R.A);
    std::memset(R.B, 0, sizeof R.B);
    std::memset(R.c, 0, sizeof R.c);
    std::memset(R.q, 0, sizeof R.q);
    std::memset(R.r, 0, sizeof R.r);
    std::memcpy(R.A, A, sizeof(double) * D * D);
    std::memcpy(R.B, B, sizeof(double) * D * nu);
    if (c) std::memcpy(R.c, c, sizeof(double) * D);
    if (q) std::memcpy(R.q, q, sizeof(double) * D);
    if (r) std::memcpy(R.r, r, sizeof(double) * nu);
    R.has_c = c ? 1 : 0;
    ro->model = kModelAffine;
    drop_attached(ro);
    return HJB_OK;
}

int32_t hjb_rollout_set_attitude_model(void *rollout, const double *inertia, double h, int32_t integrator, const double *q,
                                       const double *r) {
    Rollout *ro = (Rollout *)rollout;
    if (!ro || !inertia) return rfail(ro, HJB_E_INVALID, "rollout: null argument (inertia is required)");
    std::lock_guard<std::mutex> g(ro->mu);
    if (ro->D != 6 || ro->R.n_u != HJB_ATT_U)
        return rfail(ro, HJB_E_INVALID, "rollout: the attitude model needs D == 6 and n_u == 3 (this object: D=%d, n_u=%d)", ro->D, ro->R.n_u);
    for (int a = 0; a < 3; ++a)
        if (!(std::isfinite(inertia[a]) && inertia[a] > 0))
            return rfail(ro, HJB_E_INVALID, "rollout: inertia J%d = %g is not finite and > 0", a + 1, inertia[a]);
    if (!(std::isfinite(h) && h > 0)) return rfail(ro, HJB_E_INVALID, "rollout: h = %g is not finite and > 0", h);
    if (integrator != HJB_ATT_TAYLOR && integrator != HJB_ATT_RK4)
        return rfail(ro, HJB_E_INVALID, "rollout: integrator %d is not HJB_ATT_TAYLOR / HJB_ATT_RK4", integrator);
    if (!all_finite(q, HJB_ATT_W)) return rfail(ro, HJB_E_INVALID, "rollout: q is not finite");
    if (!all_finite(r, HJB_ATT_U)) return rfail(ro, HJB_E_INVALID, "rollout: r is not finite");
    ro->M = euler_attitude(inertia[0], inertia[1], inertia[2], h);
    if (q) std::memcpy(ro->M.q, q, sizeof ro->M.q);
    if (r) std::memcpy(ro->M.r, r, sizeof ro->M.r);
    ro->integrator = integrator;
    ro->model = kModelAttitude;
    drop_attached(ro);
    return HJB_OK;
}

int32_t hjb_rollout_set_option(void *rollout, const char *key, int64_t value) {
    Rollout *ro = (Rollout *)rollout;
    if (!ro || !key) return rfail(ro, HJB_E_INVALID, "rollout: null argument");
    std::lock_guard<std::mutex> g(ro->mu);
    if (!strcmp(key, "chunk")) {
        if (value < 1 || value > kMaxChunk) return rfail(ro, HJB_E_INVALID, "rollout: chunk %lld not in 1..%lld", (long long)value, (long long)kMaxChunk);
        ro->chunk = value;
        return HJB_OK;
    }
    if (!strcmp(key, "lds")) {
        if (value != 0 && value != 1) return rfail(ro, HJB_E_INVALID, "rollout: lds %lld is not 0 or 1", (long long)value);
        ro->lds = value == 1;
        return HJB_OK;
    }
    return rfail(ro, HJB_E_INVALID, "rollout: unknown option '%s'", key);
}

int32_t hjb_rollout_run(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                        const double *X0, double *X_final, double *cost, double *X_path, double *U_path, double *device_ms) {
    const Rollout *ro = (const Rollout *)rollout;
    const ChunkPlan plan = affine_plan(ro, "hjb_rollout_run", n_steps, plane_of_step, n_traj, X0, X_final, cost, X_path, U_path, device_ms);
    return run_call(
        rollout, plan, nullptr, [&](Rollout *o) { return check_run(o, kModelAffine, method, n_steps, plane_of_step, n_traj); }, nullptr,
        [&](const Chunk &c) {
            return launch_rollout(ro->idx_bytes, method, c.lds_on, plan.W, c.R, c.nc, c.lds, c.st, c.X0, c.Xf, c.cost, c.path[0], c.path[1]);
        });
}

int32_t hjb_rollout_set_noise(void *rollout, int32_t n_nodes, const double *offsets, const double *weights) {
    Rollout *ro = (Rollout *)rollout;
    // the arguments that need no object first, then the object; every refusal before any device work
    if (n_nodes < 0 || n_nodes > HJB_DIST_MAX_NODES)
        return rfail(ro, HJB_E_INVALID, "hjb_rollout_set_noise: n_nodes=%d not in 0..%d", n_nodes, HJB_DIST_MAX_NODES);
    if (n_nodes > 0 && !offsets) return rfail(ro, HJB_E_INVALID, "hjb_rollout_set_noise: null offsets with n_nodes=%d", n_nodes);
    if (const int bad = n_nodes > 0 ? check_weights(ro, "hjb_rollout_set_noise", n_nodes, weights) : HJB_OK) return bad;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "hjb_rollout_set_noise: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    const int D = ro->D;
    int mask = 0;
    for (int w = 0; w < n_nodes; ++w)
        for (int a = 0; a < D; ++a) {
            const double d = offsets[a + (int64_t)D * w];
            if (!std::isfinite(d)) return rfail(ro, HJB_E_INVALID, "hjb_rollout_set_noise: offset of axis %d, node %d is not finite", a, w);
            if (d != 0.0) mask |= 1 << a;
        }
    // the node block as K25 reads it: [T (W - 1) | d (W x n_axes, node index fastest)]
    int n_axes = 0;
    for (int a = 0; a < D; ++a) n_axes += (mask >> a) & 1;
    std::vector<double> tab((size_t)std::max(n_nodes - 1, 0) + (size_t)n_nodes * n_axes);
    if (n_nodes > 0) {
        (void)noise_table(n_nodes, weights, tab.data());
        double *row = tab.data() + (n_nodes - 1);
        for (int a = 0; a < D; ++a) {
            if (!((mask >> a) & 1)) continue;
            for (int w = 0; w < n_nodes; ++w) row[w] = offsets[a + (int64_t)D * w];
            row += n_nodes;
        }
    }
    const void *d = nullptr;
    if (const int st = attach_table(ro, "hjb_rollout_set_noise", tab.data(), tab.size() * sizeof(double), n_nodes > 0, ro->noise, &d)) return st;
    ro->N = DNoise{};
    ro->N.n_nodes = n_nodes;
    ro->N.mask = mask;
    ro->N.n_axes = n_axes;
    ro->N.n_tab = (int32_t)tab.size();
    ro->N.tab = (const double *)d;
    return HJB_OK;
}

int32_t hjb_rollout_run_noisy(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                              const double *X0, uint64_t seed, int64_t first_stream, double *X_final, double *cost, double *X_path,
                              double *U_path, double *W_path, double *device_ms) {
    const Rollout *ro = (const Rollout *)rollout;
    const char *const who = "hjb_rollout_run_noisy";
    ChunkPlan plan = affine_plan(ro, who, n_steps, plane_of_step, n_traj, X0, X_final, cost, X_path, U_path, device_ms);
    plan.path[2] = {W_path, 1, n_steps};
    return run_call(
        rollout, plan, [&](Rollout *o) { return check_streams(o, who, n_traj, first_stream); },
        [&](Rollout *o) {
            if (const int bad = check_run(o, kModelAffine, method, n_steps, plane_of_step, n_traj)) return bad;
            return o->N.n_nodes < 1 ? rfail(o, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_noise", who) : HJB_OK;
        },
        nullptr,
        [&](const Chunk &c) {
            bool lds_on;
            const size_t lds = noisy_lds(ro, &lds_on);
            return launch_rollout_noisy(ro->idx_bytes, method, lds_on, plan.W, c.R, noise_of_chunk(ro, c, seed, first_stream, c.path[2]), c.nc, lds,
                                        c.st, c.X0, c.Xf, c.cost, c.path[0], c.path[1]);
        });
}

int32_t hjb_rollout_set_actuator_noise(void *rollout, int32_t n_nodes, const double *eps, const double *base, const double *weights) {
    Rollout *ro = (Rollout *)rollout;
    const char *const who = "hjb_rollout_set_actuator_noise";
    // hjb_rollout_set_noise's shape: the arguments that need no object first, then the object; every refusal before any device work
    if (n_nodes < 0 || n_nodes > HJB_DIST_MAX_NODES) return rfail(ro, HJB_E_INVALID, "%s: n_nodes=%d not in 0..%d", who, n_nodes, HJB_DIST_MAX_NODES);
    if (n_nodes > 0 && !eps) return rfail(ro, HJB_E_INVALID, "%s: null eps with n_nodes=%d", who, n_nodes);
    if (const int bad = n_nodes > 0 ? check_weights(ro, who, n_nodes, weights) : HJB_OK) return bad;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "%s: null handle", who);
    std::lock_guard<std::mutex> g(ro->mu);
    const int D = ro->D, nu = ro->R.n_u;
    int live = 0, base_mask = 0;
    for (int w = 0; w < n_nodes; ++w)
        for (int j = 0; j < nu; ++j) {
            const double e = eps[j + (int64_t)nu * w];
            if (!std::isfinite(e)) return rfail(ro, HJB_E_INVALID, "%s: eps of input %d, node %d is not finite", who, j, w);
            if (e != 0.0) live |= 1 << j;
        }
    for (int w = 0; base && w < n_nodes; ++w)
        for (int a = 0; a < D; ++a) {
            const double d = base[a + (int64_t)D * w];
            if (!std::isfinite(d)) return rfail(ro, HJB_E_INVALID, "%s: base of axis %d, node %d is not finite", who, a, w);
            if (d != 0.0) base_mask |= 1 << a;
        }
    // the node block as K33 reads it: [T (W - 1) | eps rows of the live inputs | base rows of the base axes], node index fastest
    int n_rows = 0;
    for (int j = 0; j < nu; ++j) n_rows += (live >> j) & 1;
    for (int a = 0; a < D; ++a) n_rows += (base_mask >> a) & 1;
    std::vector<double> tab((size_t)std::max(n_nodes - 1, 0) + (size_t)n_nodes * n_rows);
    if (n_nodes > 0) {
        (void)noise_table(n_nodes, weights, tab.data());
        double *row = tab.data() + (n_nodes - 1);
        for (int j = 0; j < nu; ++j) {
            if (!((live >> j) & 1)) continue;
            for (int w = 0; w < n_nodes; ++w) row[w] = eps[j + (int64_t)nu * w];
            row += n_nodes;
        }
        for (int a = 0; a < D; ++a) {
            if (!((base_mask >> a) & 1)) continue;
            for (int w = 0; w < n_nodes; ++w) row[w] = base[a + (int64_t)D * w];
            row += n_nodes;
        }
    }
    const void *d = nullptr;
    if (const int st = attach_table(ro, who, tab.data(), tab.size() * sizeof(double), n_nodes > 0, ro->actuator, &d)) return st;
    ro->Act = DActuator{};
    ro->Act.n_nodes = n_nodes;
    ro->Act.live = live;
    ro->Act.base_mask = base_mask;
    ro->Act.n_tab = (int32_t)tab.size();
    ro->Act.tab = (const double *)d;
    return HJB_OK;
}

int32_t hjb_rollout_run_actuator(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                 const double *X0, uint64_t seed, int64_t first_stream, double *X_final, double *cost, double *X_path,
                                 double *U_path, double *W_path, double *device_ms) {
    const Rollout *ro = (const Rollout *)rollout;
    const char *const who = "hjb_rollout_run_actuator";
    ChunkPlan plan = affine_plan(ro, who, n_steps, plane_of_step, n_traj, X0, X_final, cost, X_path, U_path, device_ms);
    plan.path[2] = {W_path, 1, n_steps};
    return run_call(
        rollout, plan, [&](Rollout *o) { return check_streams(o, who, n_traj, first_stream); },
        [&](Rollout *o) {
            if (const int bad = check_run(o, kModelAffine, method, n_steps, plane_of_step, n_traj)) return bad;
            return o->Act.n_nodes < 1 ? rfail(o, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_actuator_noise", who) : HJB_OK;
        },
        nullptr,
        [&](const Chunk &c) {
            bool lds_on;
            const size_t lds = actuator_lds(ro, &lds_on);
            DActuator N = ro->Act;                            // the call's seed, the chunk's first stream and its W_path, as noise_of_chunk
            N.seed = seed;
            N.first = (uint64_t)first_stream + (uint64_t)c.i0;
            N.Wp = c.path[2];
            N.terms = actuator_terms(plan.W, c.R.n_u, N.live, c.R.B);       // B of the model in effect at this run
            return launch_rollout_actuator(ro->idx_bytes, method, lds_on, plan.W, c.R, N, c.nc, lds, c.st, c.X0, c.Xf, c.cost, c.path[0],
                                           c.path[1]);
        });
}

int32_t hjb_rollout_noise_table(int32_t n_nodes, const double *weights, double *thresholds) {
    if (n_nodes < 1 || n_nodes > HJB_DIST_MAX_NODES)
        return rfail(nullptr, HJB_E_INVALID, "hjb_rollout_noise_table: n_nodes=%d not in 1..%d", n_nodes, HJB_DIST_MAX_NODES);
    if (n_nodes > 1 && !thresholds) return rfail(nullptr, HJB_E_INVALID, "hjb_rollout_noise_table: null thresholds");
    if (const int bad = check_weights(nullptr, "hjb_rollout_noise_table", n_nodes, weights)) return bad;
    (void)noise_table(n_nodes, weights, thresholds);
    return HJB_OK;
}

int32_t hjb_rollout_noise_draw(uint64_t seed, int64_t first_stream, int64_t n_traj, int32_t n_steps, int32_t n_nodes,
                               const double *thresholds, int32_t *nodes) {
    const char *const who = "hjb_rollout_noise_draw";
    if (const int bad = check_streams(nullptr, who, n_traj, first_stream)) return bad;
    if (n_traj < 0 || n_steps < 0) return rfail(nullptr, HJB_E_INVALID, "%s: n_traj=%lld, n_steps=%d (both >= 0)", who, (long long)n_traj, n_steps);
    if (n_nodes < 1 || n_nodes > HJB_DIST_MAX_NODES) return rfail(nullptr, HJB_E_INVALID, "%s: n_nodes=%d not in 1..%d", who, n_nodes, HJB_DIST_MAX_NODES);
    if (n_nodes > 1 && !thresholds) return rfail(nullptr, HJB_E_INVALID, "%s: null thresholds", who);
    if (n_traj > 0 && n_steps > 0 && !nodes) return rfail(nullptr, HJB_E_INVALID, "%s: null nodes", who);
    for (int w = 0; w + 1 < n_nodes; ++w)
        if (!(thresholds[w] >= 0 && thresholds[w] <= 4294967296.0) || (w > 0 && thresholds[w] < thresholds[w - 1]))
            return rfail(nullptr, HJB_E_INVALID, "%s: thresholds[%d] = %g is outside [0, 2^32] or below its predecessor", who, w, thresholds[w]);
    // the kernel's own loop (noise_step_node)
    for (int64_t i = 0; i < n_traj; ++i) {
        const uint64_t s = (uint64_t)first_stream + (uint64_t)i;
        uint32_t rw[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k < n_steps; ++k) {
            nodes[i + n_traj * k] = noise_step_node(seed, s, k, rw, thresholds, n_nodes - 1);
        }
    }
    return HJB_OK;
}

int32_t hjb_rollout_set_values(void *rollout, int32_t dtype, int32_t n_planes, const void *values) {
    Rollout *ro = (Rollout *)rollout;
    const char *const who = "hjb_rollout_set_values";
    // the arguments that need no object first, then the object; every refusal before any device work
    if (dtype != HJB_F32 && dtype != HJB_F64)
        return rfail(ro, HJB_E_INVALID, "%s: dtype %d is not HJB_F32 / HJB_F64 (convert float16 planes on the host)", who, dtype);
    if (n_planes < 0) return rfail(ro, HJB_E_INVALID, "%s: n_planes=%d < 0", who, n_planes);
    if (n_planes > 0 && !values) return rfail(ro, HJB_E_INVALID, "%s: null values with n_planes=%d", who, n_planes);
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "%s: null handle", who);
    std::lock_guard<std::mutex> g(ro->mu);
    const int64_t nS = ro->R.nS;
    if ((int64_t)n_planes > kMaxStates / nS)
        return rfail(ro, HJB_E_INVALID, "%s: size overflow (%lld states x %d planes)", who, (long long)nS, n_planes);
    const int vb = dtype == HJB_F32 ? 4 : 8;
    const void *d = nullptr;
    if (const int st = attach_table(ro, who, values, (size_t)nS * (size_t)n_planes * vb, n_planes > 0, ro->values, &d, "value planes")) return st;
    ro->dvalues = d;
    ro->val_planes = n_planes;
    ro->val_bytes = vb;
    return HJB_OK;
}

int32_t hjb_rollout_run_greedy(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_traj, const double *X0,
                               double *X_final, double *cost, double *X_path, double *U_path, double *L_path, double *V_path,
                               double *device_ms) {
    const Rollout *ro = (const Rollout *)rollout;
    const char *const who = "hjb_rollout_run_greedy";
    ChunkPlan plan = affine_plan(ro, who, n_steps, value_plane_of_step, n_traj, X0, X_final, cost, X_path, U_path, device_ms);
    plan.path[2] = {L_path, 1, n_steps};
    plan.path[3] = {V_path, 1, n_steps};
    return run_call(
        rollout, plan, nullptr, [&](Rollout *o) { return check_lookahead_run(o, who, 0, n_steps, value_plane_of_step, n_traj, false); }, nullptr,
        [&](const Chunk &c) { return launch_rollout_greedy(ro->val_bytes, c.lds_on, plan.W, greedy_of_chunk(ro, c), c.lds, c.st); });
}

int32_t hjb_rollout_greedy_host(int32_t D, const int32_t *n, const double *knots, int32_t n_labels, int32_t n_u, const double *u_table,
                                const double *A, const double *B, const double *c, const double *q, const double *r, int32_t dtype,
                                int32_t n_value_planes, const void *values, int32_t n_steps, const int32_t *value_plane_of_step,
                                int64_t n_traj, const double *X0, double *X_final, double *cost, double *X_path, double *U_path,
                                double *L_path, double *V_path) {
    const char *const who = "hjb_rollout_greedy_host";
    const AffineHostArgs a{D, n, knots, n_labels, n_u, u_table, A, B, c, q, r, dtype, n_value_planes, values, n_steps, value_plane_of_step};
    if (const int bad = affine_host_args(who, a, n_traj)) return bad;
    AffineHostProblem P;
    if (const int bad = affine_host_model(who, a, P)) return bad;
    if (n_traj == 0) return HJB_OK;
    const int bad_traj = check_traj(nullptr, who, D, "D", n_steps, n_traj, X0, X_final);
    if (bad_traj) return bad_traj;
    with_bool(dtype == HJB_F32, [&](auto f) {
        with_dim(D, [&](auto d) {
            using TV = std::conditional_t<decltype(f)::value, float, double>;
            greedy_rollout_host<decltype(d)::value, TV>(P.M, knots, P.rdx.data(), u_table, static_cast<const TV *>(values), n_steps,
                                                        value_plane_of_step, n_traj, X0, X_final, cost, X_path, U_path, L_path, V_path);
        });
    });
    return HJB_OK;
}

int32_t hjb_rollout_set_lookahead(void *rollout, int32_t mode, int32_t n_nodes, const double *offsets, const double *weights) {
    Rollout *ro = (Rollout *)rollout;
    const char *const who = "hjb_rollout_set_lookahead";
    // the arguments that need no object first, then the object; every refusal before any device work
    if (const int bad = check_lookahead(ro, who, 0, mode, n_nodes, offsets, weights)) return bad;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "%s: null handle", who);
    std::lock_guard<std::mutex> g(ro->mu);
    const int D = ro->D;
    if (const int bad = check_lookahead(ro, who, D, mode, n_nodes, offsets, weights)) return bad;
    LookSet L{};
    L.mode = mode;
    std::vector<double> tab((size_t)n_nodes * (1 + D));
    const int n_tab = look_table(D, n_nodes, offsets, weights, L, tab.data());
    const void *d = nullptr;
    if (const int st = attach_table(ro, who, tab.data(), (size_t)n_tab * sizeof(double), n_nodes > 0, ro->look, &d)) return st;
    ro->L = L;
    ro->L.tab = (const double *)d;
    return HJB_OK;
}

int32_t hjb_rollout_run_lookahead(void *rollout, int32_t fly_noise, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_traj,
                                  const double *X0, uint64_t seed, int64_t first_stream, double *X_final, double *cost, double *X_path,
                                  double *U_path, double *L_path, double *V_path, double *W_path, double *device_ms) {
    const Rollout *ro = (const Rollout *)rollout;
    const char *const who = "hjb_rollout_run_lookahead";
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
        [&](Rollout *o) { return check_lookahead_run(o, who, fly_noise, n_steps, value_plane_of_step, n_traj); }, nullptr,
        [&](const Chunk &c) {
            DLook A{};
            A.G = greedy_of_chunk(ro, c);
            A.L = ro->L;
            if (!fly_noise) return launch_rollout_lookahead(ro->val_bytes, c.lds_on, plan.W, A, c.lds, c.st);
            A.N = noise_of_chunk(ro, c, seed, first_stream, c.path[4]);
            bool lds_on;
            const size_t lds = noisy_lds(ro, &lds_on);
            return launch_rollout_lookahead_fly(ro->val_bytes, lds_on, plan.W, A, lds, c.st);
        });
}

int32_t hjb_rollout_lookahead_host(int32_t D, const int32_t *n, const double *knots, int32_t n_labels, int32_t n_u, const double *u_table,
                                   const double *A, const double *B, const double *c, const double *q, const double *r, int32_t dtype,
                                   int32_t n_value_planes, const void *values, int32_t n_steps, const int32_t *value_plane_of_step,
                                   int64_t n_traj, const double *X0, double *X_final, double *cost, double *X_path, double *U_path,
                                   double *L_path, double *V_path, int32_t mode, int32_t n_nodes, const double *offsets,
                                   const double *weights, const int32_t *nodes, int32_t n_flight_nodes, const double *flight_offsets) {
    const char *const who = "hjb_rollout_lookahead_host";
    const AffineHostArgs a{D, n, knots, n_labels, n_u, u_table, A, B, c, q, r, dtype, n_value_planes, values, n_steps, value_plane_of_step};
    if (const int bad = look_host_args(who, a, n_traj, mode, n_nodes, offsets, weights)) return bad;
    if (nodes) {
        if (n_flight_nodes < 1 || n_flight_nodes > HJB_DIST_MAX_NODES)
            return rfail(nullptr, HJB_E_INVALID, "%s: n_flight_nodes=%d not in 1..%d", who, n_flight_nodes, HJB_DIST_MAX_NODES);
        if (!flight_offsets) return rfail(nullptr, HJB_E_INVALID, "%s: nodes given with null flight_offsets", who);
        if (!all_finite(flight_offsets, (int64_t)D * n_flight_nodes)) return rfail(nullptr, HJB_E_INVALID, "%s: flight_offsets is not finite", who);
    }
    LookHostProblem P;
    if (const int bad = look_host_model(who, a, mode, n_nodes, offsets, weights, P)) return bad;
    if (n_traj == 0) return HJB_OK;
    const int bad_traj = check_traj(nullptr, who, D, "D", n_steps, n_traj, X0, X_final);
    if (bad_traj) return bad_traj;
    if (nodes)
        for (int64_t e = 0; e < n_traj * (int64_t)n_steps; ++e)
            if (nodes[e] < 0 || nodes[e] >= n_flight_nodes)
                return rfail(nullptr, HJB_E_INVALID, "%s: nodes element %lld = %d outside [0, %d)", who, (long long)e, nodes[e], n_flight_nodes);
    int fmask = 0;                                            // the flight set's mask, as hjb_rollout_set_noise forms it
    for (int w = 0; nodes && w < n_flight_nodes; ++w)
        for (int a = 0; a < D; ++a)
            if (flight_offsets[a + (int64_t)D * w] != 0.0) fmask |= 1 << a;
    with_bool(dtype == HJB_F32, [&](auto f) {
        with_dim(D, [&](auto d) {
            using TV = std::conditional_t<decltype(f)::value, float, double>;
            lookahead_rollout_host<decltype(d)::value, TV>(P.M, P.L, knots, P.rdx.data(), u_table, static_cast<const TV *>(values), n_steps,
                                                           value_plane_of_step, n_traj, X0, nodes, fmask, flight_offsets, X_final, cost,
                                                           X_path, U_path, L_path, V_path);
        });
    });
    return HJB_OK;
}

int32_t hjb_rollout_run_attitude(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                 const double *X0, double *X_final, double *cost, double *X_path, double *U_path, double *A_path,
                                 double *device_ms) {
    const Rollout *ro = (const Rollout *)rollout;
    const ChunkPlan plan{{"hjb_rollout_run_attitude", HJB_ATT_W, "7", n_steps, plane_of_step, n_traj, X0, X_final, device_ms},
                         {{X_path, HJB_ATT_W, n_steps + 1}, {U_path, HJB_ATT_U, n_steps}, {A_path, 3, n_steps}}, cost};
    return run_call(
        rollout, plan, nullptr, [&](Rollout *o) { return check_run(o, kModelAttitude, method, n_steps, plane_of_step, n_traj); },
        [&](Rollout *o) { return check_quaternions(o, "rollout", n_traj, X0); },
        [&](const Chunk &c) {
            return launch_rollout_attitude(ro->idx_bytes, method, c.lds_on, ro->integrator, c.R, ro->M, c.nc, c.lds, c.st, c.X0, c.Xf, c.cost,
                                           c.path[0], c.path[1], c.path[2]);
        });
}

int32_t hjb_attitude_linear_response(int32_t device, const double *inertia, double h, int32_t integrator, const double *K,
                                     const double *C, const double *qc, const double *u_limit, int32_t cost_form,
                                     const double *weights, int32_t n_steps, int64_t n_traj, const double *X0, double *X_final,
                                     double *cost, double *X_path, double *U_path, double *A_path, int64_t chunk, double *device_ms) {
    const char *const who = "hjb_attitude_linear_response";
    if (device_ms) *device_ms = 0.0;
    // every refusal first: none of them needs a device
    if (!inertia || !K || !C) return rfail(nullptr, HJB_E_INVALID, "%s: null argument (inertia, K and C are required)", who);
    if (device < 0) return rfail(nullptr, HJB_E_INVALID, "%s: device %d", who, device);
    for (int a = 0; a < 3; ++a)
        if (!(std::isfinite(inertia[a]) && inertia[a] > 0))
            return rfail(nullptr, HJB_E_INVALID, "%s: inertia J%d = %g is not finite and > 0", who, a + 1, inertia[a]);
    if (!(std::isfinite(h) && h > 0)) return rfail(nullptr, HJB_E_INVALID, "%s: h = %g is not finite and > 0", who, h);
    if (integrator != HJB_ATT_TAYLOR && integrator != HJB_ATT_RK4)
        return rfail(nullptr, HJB_E_INVALID, "%s: integrator %d is not HJB_ATT_TAYLOR / HJB_ATT_RK4", who, integrator);
    if (cost_form != HJB_ATTL_COST_QUAT && cost_form != HJB_ATTL_COST_ANGLE)
        return rfail(nullptr, HJB_E_INVALID, "%s: cost_form %d is not HJB_ATTL_COST_QUAT / HJB_ATTL_COST_ANGLE", who, cost_form);
    if (!all_finite(K, 9)) return rfail(nullptr, HJB_E_INVALID, "%s: K is not finite", who);
    if (!all_finite(C, 9)) return rfail(nullptr, HJB_E_INVALID, "%s: C is not finite", who);
    if (!all_finite(qc, 16)) return rfail(nullptr, HJB_E_INVALID, "%s: qc is not finite", who);
    if (!all_finite(u_limit, 3)) return rfail(nullptr, HJB_E_INVALID, "%s: u_limit is not finite", who);
    for (int a = 0; u_limit && a < 3; ++a)
        if (u_limit[a] < 0) return rfail(nullptr, HJB_E_INVALID, "%s: u_limit[%d] = %g < 0", who, a, u_limit[a]);
    if (!all_finite(weights, 10)) return rfail(nullptr, HJB_E_INVALID, "%s: weights is not finite", who);
    if (n_steps < 0) return rfail(nullptr, HJB_E_INVALID, "%s: n_steps=%d < 0", who, n_steps);
    if (n_traj < 0) return rfail(nullptr, HJB_E_INVALID, "%s: n_traj=%lld < 0", who, (long long)n_traj);
    if (chunk < 0 || chunk > kMaxChunk)
        return rfail(nullptr, HJB_E_INVALID, "%s: chunk %lld not in 0..%lld", who, (long long)chunk, (long long)kMaxChunk);
    if (n_traj == 0) return HJB_OK;
    int bad_traj = check_traj(nullptr, who, HJB_ATT_W, "7", n_steps, n_traj, X0, X_final);
    if (!bad_traj) bad_traj = check_quaternions(nullptr, who, n_traj, X0);
    if (bad_traj) return bad_traj;
    DAttLinear M{};
    M.A = euler_attitude(inertia[0], inertia[1], inertia[2], h);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {                 // column-major in, row-major kept
            M.K[3 * r + c] = K[r + 3 * c];
            M.C[3 * r + c] = C[r + 3 * c];
        }
        for (int c = 0; c < 4; ++c) M.qc[4 * r + c] = qc ? qc[r + 4 * c] : (r == c ? 1.0 : 0.0);
    }
    if (u_limit) std::memcpy(M.L, u_limit, sizeof M.L);
    M.has_limit = u_limit ? 1 : 0;
    if (weights) std::memcpy(M.w, weights, sizeof M.w);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return rfail(nullptr, HJB_E_DEVICE, "no HIP device visible (libhjbdp has no CPU fallback)");
    if (device >= ndev) return rfail(nullptr, HJB_E_INVALID, "%s: device %d (%d visible)", who, device, ndev);
    // a transient object without a policy: run_chunks reads its device, chunk and stream only
    Rollout ro;
    ro.device = device;
    if (chunk > 0) ro.chunk = chunk;
    {
        std::shared_lock<std::shared_mutex> lk(g_capture_mu);
        if (hipSetDevice(device) != hipSuccess) return rfail(nullptr, HJB_E_DEVICE, "hipSetDevice failed");
        if (hipStreamCreateWithFlags(&ro.stream, hipStreamNonBlocking) != hipSuccess) {
            ro.stream = nullptr;
            return rfail(nullptr, HJB_E_DEVICE, "%s: stream creation failed", who);
        }
    }
    ChunkPlan plan{{who, HJB_ATT_W, "7", n_steps, nullptr, n_traj, X0, X_final, device_ms},
                   {{X_path, HJB_ATT_W, n_steps + 1}, {U_path, HJB_ATT_U, n_steps}, {A_path, 3, n_steps}}, cost};
    const int st = run_chunks(&ro, plan, [&](const Chunk &c) {
        DAttLinear Mk = M;
        Mk.n_steps = c.R.n_steps;
        return launch_rollout_attitude_linear(integrator, cost_form, Mk, c.nc, c.st, c.X0, c.Xf, c.cost, c.path[0], c.path[1], c.path[2]);
    });
    {
        std::shared_lock<std::shared_mutex> lk(g_capture_mu);
        (void)hipSetDevice(device);
        release(&ro);
    }
    return st;
}

int32_t hjb_rollout_destroy(void *rollout) {
    Rollout *ro = (Rollout *)rollout;
    if (!ro) return HJB_OK;
    {
        std::lock_guard<std::mutex> g(ro->mu);
        std::shared_lock<std::shared_mutex> lk(g_capture_mu);
        (void)hipSetDevice(ro->device);
        if (ro->stream) (void)hipStreamSynchronize(ro->stream);
        release(ro);
    }
    delete ro;
    return HJB_OK;
}

const char *hjb_rollout_last_error(void *rollout) {
    Rollout *ro = (Rollout *)rollout;
    return ro ? ro->err.c_str() : g_last_error.c_str();
}

}  // extern "C"
