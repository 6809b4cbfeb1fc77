// rollout.hip - hjb_rollout_* and hjb_attitude_linear_response: the host side of the batched closed-loop rollouts
// (include/hjbdp.h).  An object holds one stored policy (hjb_rollout_create) and one model, the last one set:
//   affine (K16, kernels_rollout.h, launched from this unit), attitude (K17, kernels_rollout_attitude.h / rollout_attitude.hip),
//   and the three that attach two more objects' policies as channels: pos-att (K18, kernels_rollout_pos_att.h /
//   rollout_pos_att.hip; its fault campaigns K23, kernels_rollout_pos_att_faults.h / rollout_pos_att_faults.hip), position (K19,
//   kernels_rollout_position.h / rollout_position.hip), simplified attitude (K20, kernels_rollout_attitude_simplified.h /
//   rollout_attitude_simplified.hip).
// The linear attitude controller (K21, kernels_rollout_attitude_linear.h / rollout_attitude_linear.hip) needs no object.
// Beside the model an object may hold a noise node set (hjb_rollout_set_noise): hjb_rollout_run_noisy (K25,
// kernels_rollout_noisy.h / rollout_noisy.hip) flies the affine loop under it, and no other run function reads it.  The sampler's
// host twins hjb_rollout_noise_table / hjb_rollout_noise_draw (hjbdp_noise.h) need no device.
// And it may hold value planes (hjb_rollout_set_values): hjb_rollout_run_greedy (K26, kernels_rollout_greedy.h /
// rollout_greedy.hip) flies the affine loop by one-step lookahead on them, and no other run function reads them.  Its host twin
// hjb_rollout_greedy_host (hjbdp_greedy.h) needs no device and no object.
// Shared here: the attached-channels record and attach_channels (the three attaching setters), check_run / check_traj /
// check_quaternions (the run functions' refusals, all before any device work), lds_bytes, run_chunks (the chunk loop).
#include "hjbdp_host.h"
#include "kernels_rollout.h"
#include "kernels_rollout_attitude.h"
#include "kernels_rollout_pos_att.h"
#include "kernels_rollout_pos_att_faults.h"
#include "kernels_rollout_position.h"
#include "kernels_rollout_attitude_simplified.h"
#include "kernels_rollout_attitude_linear.h"
#include "kernels_rollout_noisy.h"
#include "kernels_rollout_greedy.h"
#include "rollout_dispatch.h"
#include <memory>

using namespace hjbhost;

namespace {

// the model an object holds: the last setter called wins.  The last three keep an Attached record in Rollout::att, the others none
enum { kModelNone = 0, kModelAffine = 1, kModelAttitude = 2, kModelPosAtt = 3, kModelPosition = 4, kModelAttSimplified = 5 };

// Device allocations with shared ownership: an object's grid, table and labels live as long as the object or a pos-att, position
// or simplified attitude model that reads them (hjb_rollout_set_pos_att_model / hjb_rollout_set_position_model /
// hjb_rollout_set_attitude_simplified_model on another object) does.  Freed under the
// last owner's locks (destroy / set_*model).
struct DevData {
    int device = 0;
    std::vector<void *> allocs;
    ~DevData() {
        if (allocs.empty()) return;
        (void)hipSetDevice(device);
        for (void *p : allocs) (void)hipFree(p);
    }
};

// What a model of three channels holds of the two other objects (y and z, or 2 and 3): their policies' descriptors, with the
// device data kept alive.  The model's own members sit on top (PosAtt, Position, AttSimplified).
struct Attached {
    DPaChan c[2]{};
    std::shared_ptr<DevData> data[2];
    int n_planes = 0;               // of the three channels, the fewest
    virtual ~Attached() = default;
};

// The pos-att model of channel x's object
struct PosAtt : Attached {
    std::shared_ptr<DevData> coef;
    DPosAtt M{};
    int max_steps = 0;              // (n_nodes - 1) / (2 substeps)
    double h = 0;                   // as given (M.hs is h / substeps)
    // the fault controller of channel x (hjb_rollout_set_pos_att_fault_controller): read by hjb_rollout_run_pos_att_faults alone
    bool has_xf = false;
    DPaChan cxf{};
    std::shared_ptr<DevData> data_xf;
    int planes_xf = 0;
};

// The position model of channel x's object
struct Position : Attached {
    std::shared_ptr<DevData> table;     // n_sub and the sub-step rows
    DPosition M{};
    int max_steps = 0;              // stages the table holds
};

// The simplified attitude model of channel 1's object
struct AttSimplified : Attached {
    DAttSimplified M{};
    int dynamics = HJB_ATTS_FULL;
};

struct Rollout {
    std::mutex mu;                  // one call at a time per object
    int device = 0, D = 0, idx_bytes = 4, n_planes = 0;
    int model = kModelNone, integrator = HJB_ATT_TAYLOR;
    int64_t chunk = (int64_t)1 << 20;
    bool lds = true;                // option "lds": stage the tables in LDS when they fit (false: never)
    DRollout R{};                   // device pointers filled by create; model by set_model
    DAttitude M{};                  // the attitude model (set_attitude_model)
    std::unique_ptr<Attached> att;  // the PosAtt / Position / AttSimplified of model kModelPosAtt / kModelPosition / kModelAttSimplified
    std::shared_ptr<DevData> data;
    // the noise node set (hjb_rollout_set_noise): N.n_nodes > 0 while one is set; read by hjb_rollout_run_noisy alone
    DNoise N{};
    std::shared_ptr<DevData> noise;     // N.tab: thresholds, then the masked axes' offsets
    // the value planes (hjb_rollout_set_values): val_planes > 0 while some are set; read by hjb_rollout_run_greedy alone
    std::shared_ptr<DevData> values;
    const void *dvalues = nullptr;      // [nS, val_planes] column-major, float or double
    int val_planes = 0, val_bytes = 8;
    hipStream_t stream = nullptr;
    std::string err;
};

constexpr int64_t kMaxChunk = (int64_t)1 << 30;
constexpr size_t kLdsMax = 32 << 10;        // knots + 1/dx + u_table staged in LDS up to this size

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

void release(Rollout *ro) {
    ro->att.reset();
    ro->noise.reset();
    ro->values.reset();
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

// K16's 72 instantiations (label type x method x LDS x D) and the launch of the one asked for
hipError_t launch_rollout(int idx_bytes, int method, bool lds_on, int D, const DRollout &R, int64_t nc, size_t lds, hipStream_t st,
                          const double *X0, double *Xf, double *cost, double *Xp, double *Up) {
    const dim3 b(256), g((unsigned)((nc + 255) / 256));
    with_label_type(idx_bytes, [&](auto tl) {
        with_int<HJB_LOOKUP_NEAREST, HJB_LOOKUP_LINEAR>(method, [&](auto m) {
            with_bool(lds_on, [&](auto l) {
                with_dim(D, [&](auto d) {
                    using TL = typename decltype(tl)::type;
                    constexpr bool LDS = decltype(l)::value;
                    hipLaunchKernelGGL((k_rollout<decltype(d)::value, TL, decltype(m)::value, LDS>), g, b, LDS ? lds : 0, st, R, nc, X0,
                                       Xf, cost, Xp, Up);
                });
            });
        });
    });
    return hipGetLastError();
}

bool all_finite(const double *p, int64_t n) { return !p || first_nonfinite(p, n, true) < 0; }

// The argument checks every run function of an object makes before any device work: method, sizes, that the object holds the
// model this entry point runs (`want`), plane_of_step against the planes all of the model's channels have.
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

// The checks on the trajectories every run function makes next (pre: "rollout", or the entry point's name where there is no
// object): null X0 / X_final, the sizes of W doubles per trajectory and stage (wname: how the message spells W), a finite X0.
int check_traj(Rollout *ro, const char *pre, int W, const char *wname, int32_t n_steps, int64_t n_traj, const double *X0,
               const double *X_final) {
    if (!X0 || !X_final) return rfail(ro, HJB_E_INVALID, "%s: null X0 / X_final", pre);
    if (n_traj > INT64_MAX / (W * ((int64_t)n_steps + 1)) / 8)
        return rfail(ro, HJB_E_INVALID, "%s: size overflow (n_traj x %s x n_steps)", pre, wname);
    const int64_t bad = first_nonfinite(X0, (int64_t)W * n_traj, true);
    if (bad >= 0) return rfail(ro, HJB_E_INVALID, "%s: X0 element %lld is not finite", pre, (long long)bad);
    return HJB_OK;
}

// K17 and K21 renormalise the quaternion X0[3..6] of a 7-state column after the first step: all zeros would be 0/0
int check_quaternions(Rollout *ro, const char *pre, int64_t n_traj, const double *X0) {
    for (int64_t i = 0; i < n_traj; ++i) {
        const double *q = X0 + HJB_ATT_W * i + 3;
        if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0)
            return rfail(ro, HJB_E_INVALID, "%s: X0 column %lld has an all-zero quaternion (0/0 at the first renormalisation)", pre,
                         (long long)i);
    }
    return HJB_OK;
}

// a pos-att, position or simplified attitude model goes, and with it its hold on the other two channels
void drop_attached(Rollout *ro) {
    if (!ro->att) return;
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    ro->att.reset();
}

// what K18, K19 and K20 read of an object's policy (kernels_rollout_pos_att.h)
DPaChan pa_channel(const DRollout &R) {
    DPaChan c{};
    for (int a = 0; a < 4; ++a) {
        c.n[a] = R.n[a];
        c.koff[a] = R.koff[a];
        c.uniform[a] = R.uniform[a];
        c.x0[a] = R.x0[a];
        c.inv_h[a] = R.inv_h[a];
        c.stride[a] = R.stride[a];
    }
    c.nS = R.nS;
    c.n_knots = R.n_knots;
    c.n_labels = R.n_labels;
    c.index_base = R.index_base;
    c.knots = R.knots;
    c.rdx = R.rdx;
    c.u_table = R.u_table;
    c.labels = R.labels;
    return c;
}

DPaChan on_planes(DPaChan c, const int32_t *plane_of_step) {
    c.plane_of_step = plane_of_step;
    return c;
}

// the LDS bytes of the channels' [knots | 1/dx | u_table], `width` u_table doubles per label
size_t lds_bytes(std::initializer_list<const DPaChan *> chans, int width) {
    int64_t nk = 0, nl = 0;
    for (const DPaChan *c : chans) {
        nk += c->n_knots;
        nl += c->n_labels;
    }
    return (size_t)(2 * nk + width * nl) * sizeof(double);
}

// Another object's policy as a channel: a snapshot with a share of its device data, taken under that object's own lock
struct ChanSnap {
    DPaChan c{};
    std::shared_ptr<DevData> data;
    int D = 0, n_u = 0, device = 0, idx_bytes = 0, n_planes = 0;
};

ChanSnap snap_channel(Rollout *o) {
    std::lock_guard<std::mutex> g(o->mu);
    ChanSnap s;
    s.c = pa_channel(o->R);
    s.data = o->data;
    s.D = o->D;
    s.n_u = o->R.n_u;
    s.device = o->device;
    s.idx_bytes = o->idx_bytes;
    s.n_planes = o->n_planes;
    return s;
}

// a snapshot against the object rx it is attached to (under rx's lock): one device, one label type
int check_channel(Rollout *rx, const ChanSnap &s, const char *name, const char *rx_name, const char *sharers) {
    if (s.device != rx->device)
        return rfail(rx, HJB_E_INVALID, "rollout: %s is on device %d, %s on device %d", name, s.device, rx_name, rx->device);
    if (s.idx_bytes != rx->idx_bytes)
        return rfail(rx, HJB_E_INVALID, "rollout: %s has %d-byte labels, %s %d-byte labels (the %s share one label type)", name,
                     s.idx_bytes, rx_name, rx->idx_bytes, sharers);
    return HJB_OK;
}

// What the setters of a three-channel model share.  rs: the three objects, names: their handles' names in the messages, model:
// the model's name there; every channel needs D == D and n_u == n_u.  Snapshots the two other channels under their own locks
// (in order), then takes rs[0]'s lock into lk - the caller holds it to its end - and checks the three against each other;
// at gets the snapshots and the fewest planes.  On a refusal the snapshots' shares of the other objects' device data go with
// this frame, under rs[0]'s lock when it was taken and without g_capture_mu: a share frees device memory only as the last owner,
// that is when the other object was destroyed in between (a refused setter of the earlier form freed the same way).
int attach_channels(Rollout *const (&rs)[3], const char *const (&names)[3], const char *model, int D, int n_u, Attached &at,
                    std::unique_lock<std::mutex> &lk) {
    Rollout *rx = rs[0];
    if (!rs[0] || !rs[1] || !rs[2]) return rfail(rx, HJB_E_INVALID, "rollout: null handle (three channel objects are required)");
    if (rs[0] == rs[1] || rs[0] == rs[2] || rs[1] == rs[2]) return rfail(rx, HJB_E_INVALID, "rollout: the same object passed for two channels");
    const char *const needs = "rollout: the %s model needs D == %d and n_u == %d (%s: D=%d, n_u=%d)";
    ChanSnap sn[2];
    for (int t = 0; t < 2; ++t) {
        sn[t] = snap_channel(rs[1 + t]);
        if (sn[t].D != D || sn[t].n_u != n_u) return rfail(rx, HJB_E_INVALID, needs, model, D, n_u, names[1 + t], sn[t].D, sn[t].n_u);
    }
    lk = std::unique_lock<std::mutex>(rx->mu);
    if (rx->D != D || rx->R.n_u != n_u) return rfail(rx, HJB_E_INVALID, needs, model, D, n_u, names[0], rx->D, rx->R.n_u);
    for (int t = 0; t < 2; ++t) {
        const int bad = check_channel(rx, sn[t], names[1 + t], names[0], "three channels");
        if (bad) return bad;
    }
    at.n_planes = std::min(rx->n_planes, std::min(sn[0].n_planes, sn[1].n_planes));
    for (int t = 0; t < 2; ++t) {
        at.c[t] = sn[t].c;
        at.data[t] = std::move(sn[t].data);
    }
    return HJB_OK;
}

// under rx's lock and g_capture_mu, on rx's device: the model takes the place of (and releases) whatever was attached
void install_attached(Rollout *rx, std::unique_ptr<Attached> at, int model) {
    if (rx->stream) (void)hipStreamSynchronize(rx->stream);
    rx->att = std::move(at);
    rx->model = model;
}

// The chunk loop the run functions share: W doubles of state per trajectory; per step n_up control rows (U_path) and n_e more
// path rows (E_path: the attitude loop's angles, the pos-att loop's Force_Moment).  Per chunk: upload X0, launch(R, nc, lds, lds_on, stream, X0, Xf, cost, Xp, Up, Ep, Fl) (the
// kernel of the entry point `who`; Fl: nc int32 flags, allocated when `flags` is asked for: the position loop's off_schedule),
// download X_final / cost / flags and the paths ([nc, rows] on the device -> columns i0 .. i0+nc of
// [n_traj, rows] on the host); device_ms sums the launches' event times.  plane_of_step may be null for a loop without a policy
// (hjb_attitude_linear_response): nothing is uploaded then.  pre(i0, nc, stream) runs per chunk after X0's upload and before the
// launch's first event (hjb_rollout_run_pos_att_faults uploads its per-trajectory inputs there, at the chunk's own offset).
template <typename Launch, typename Pre>
int run_chunks(Rollout *ro, const char *who, int W, int n_up, int n_e, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
               const double *X0, double *X_final, double *cost, double *X_path, double *U_path, double *E_path, int32_t *flags,
               double *device_ms, Launch launch, Pre pre) {
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(ro->device) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipSetDevice failed");
    const int nu = n_up;
    const int64_t nc_max = std::min(n_traj, ro->chunk);
    const size_t xb = (size_t)nc_max * W * sizeof(double);
    const size_t xpb = X_path ? (size_t)nc_max * W * ((size_t)n_steps + 1) * sizeof(double) : 0;
    const size_t upb = U_path ? (size_t)nc_max * nu * (size_t)n_steps * sizeof(double) : 0;
    const size_t epb = E_path ? (size_t)nc_max * n_e * (size_t)n_steps * sizeof(double) : 0;
    const size_t cb = cost ? (size_t)nc_max * sizeof(double) : 0;
    const size_t pb = (size_t)std::max(n_steps, 1) * sizeof(int32_t);
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipMemGetInfo failed");
    const size_t fb = flags ? (size_t)nc_max * sizeof(int32_t) : 0;
    const size_t need = 2 * xb + xpb + upb + epb + cb + pb + fb;
    if (need + ((size_t)64 << 20) > fr)
        return rfail(ro, HJB_E_NOMEM, "rollout: a chunk of %lld trajectories needs %zu bytes, %zu free (lower option \"chunk\")",
                     (long long)nc_max, need, fr);
    void *bufs[8] = {};
    auto done = [&](int code) {
        for (void *p : bufs) if (p) (void)hipFree(p);
        return code;
    };
    const size_t sizes[8] = {xb, xb, cb, xpb, upb, pb, epb, fb};
    for (int b = 0; b < 8; ++b)
        if (sizes[b] && hipMalloc(&bufs[b], sizes[b]) != hipSuccess) return done(rfail(ro, HJB_E_NOMEM, "rollout: hipMalloc of %zu bytes failed", sizes[b]));
    double *dX0 = (double *)bufs[0], *dXf = (double *)bufs[1], *dC = (double *)bufs[2], *dXp = (double *)bufs[3], *dUp = (double *)bufs[4];
    double *dEp = (double *)bufs[6];
    int32_t *dFl = (int32_t *)bufs[7];
    hipStream_t st = ro->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess && n_steps > 0 && plane_of_step) e = hipMemcpyAsync(bufs[5], plane_of_step, pb, hipMemcpyHostToDevice, st);
    DRollout R = ro->R;
    R.plane_of_step = (const int32_t *)bufs[5];
    R.n_steps = n_steps;
    const size_t lds = (size_t)(2 * (int64_t)R.n_knots + (int64_t)R.n_labels * R.n_u) * sizeof(double);
    const bool lds_on = ro->lds && lds <= kLdsMax;
    double ms_total = 0;
    for (int64_t i0 = 0; e == hipSuccess && i0 < n_traj; i0 += nc_max) {
        const int64_t nc = std::min(nc_max, n_traj - i0);
        e = hipMemcpyAsync(dX0, X0 + W * i0, (size_t)nc * W * sizeof(double), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        e = pre(i0, nc, st);
        if (e != hipSuccess) break;
        (void)hipEventRecord(e0, st);
        e = launch(R, nc, lds, lds_on, st, dX0, dXf, dC, dXp, dUp, dEp, dFl);
        if (e != hipSuccess) break;
        (void)hipEventRecord(e1, st);
        e = hipMemcpyAsync(X_final + W * i0, dXf, (size_t)nc * W * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && cost) e = hipMemcpyAsync(cost + i0, dC, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && flags) e = hipMemcpyAsync(flags + i0, dFl, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        // paths: [nc, rows] on the device -> columns i0 .. i0+nc of [n_traj, rows] on the host
        if (e == hipSuccess && X_path)
            e = hipMemcpy2DAsync(X_path + i0, (size_t)n_traj * sizeof(double), dXp, (size_t)nc * sizeof(double), (size_t)nc * sizeof(double),
                                 (size_t)W * (n_steps + 1), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && U_path && n_steps > 0)
            e = hipMemcpy2DAsync(U_path + i0, (size_t)n_traj * sizeof(double), dUp, (size_t)nc * sizeof(double), (size_t)nc * sizeof(double),
                                 (size_t)nu * n_steps, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && E_path && n_steps > 0)
            e = hipMemcpy2DAsync(E_path + i0, (size_t)n_traj * sizeof(double), dEp, (size_t)nc * sizeof(double), (size_t)nc * sizeof(double),
                                 (size_t)n_e * n_steps, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        ms_total += ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return done(rfail(ro, HJB_E_DEVICE, "%s: %s", who, hipGetErrorString(e)));
    }
    if (device_ms) *device_ms = ms_total;
    return done(HJB_OK);
}

template <typename Launch>
int run_chunks(Rollout *ro, const char *who, int W, int n_up, int n_e, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
               const double *X0, double *X_final, double *cost, double *X_path, double *U_path, double *E_path, int32_t *flags,
               double *device_ms, Launch launch) {
    return run_chunks(ro, who, W, n_up, n_e, n_steps, plane_of_step, n_traj, X0, X_final, cost, X_path, U_path, E_path, flags, device_ms,
                      launch, [](int64_t, int64_t, hipStream_t) { return hipSuccess; });
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

}  // namespace

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
    for (int a = 0; a < D; ++a) {
        if (n[a] < 2) return rfail(nullptr, HJB_E_INVALID, "rollout: axis %d has %d knots (need >= 2)", a, n[a]);
        const double *kk = knots + n_knots;
        for (int i = 0; i < n[a]; ++i)
            if (!std::isfinite(kk[i])) return rfail(nullptr, HJB_E_INVALID, "rollout: knot %d of axis %d is not finite", i, a);
        for (int i = 0; i + 1 < n[a]; ++i)
            if (!(kk[i + 1] > kk[i])) return rfail(nullptr, HJB_E_INVALID, "rollout: knots of axis %d not strictly increasing (at %d)", a, i);
        n_knots += n[a];
        if (n_knots > INT32_MAX || nS > kMaxStates / n[a]) return rfail(nullptr, HJB_E_INVALID, "rollout: size overflow (grid)");
        nS *= n[a];
    }
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
    ro->data = std::make_shared<DevData>();
    ro->data->device = device;
    DRollout &R = ro->R;
    R.n_u = n_u;
    R.n_labels = n_labels;
    R.index_base = index_base;
    R.n_knots = (int32_t)n_knots;
    R.nS = nS;
    std::vector<double> kk(knots, knots + n_knots), rdx(n_knots, 0.0);
    int64_t s = 1, off = 0;
    for (int a = 0; a < D; ++a) {
        const double *k = kk.data() + off;
        for (int i = 0; i + 1 < n[a]; ++i) rdx[off + i] = 1.0 / (k[i + 1] - k[i]);     // as hjb_policy_lookup builds it
        const double hstep = (k[n[a] - 1] - k[0]) / (n[a] - 1);
        double dev = 0;
        for (int i = 0; i < n[a]; ++i) dev = std::max(dev, std::fabs(k[i] - (k[0] + i * hstep)));
        R.uniform[a] = dev <= 1.5 * hstep ? 1 : 0;
        R.x0[a] = k[0];
        R.inv_h[a] = 1.0 / hstep;
        R.n[a] = n[a];
        R.koff[a] = (int32_t)off;
        R.stride[a] = s;
        s *= n[a];
        off += n[a];
    }
    auto dev_upload = [&](const void *src, size_t bytes, void **out) -> int {
        void *d = nullptr;
        if (hipMalloc(&d, std::max<size_t>(bytes, 16)) != hipSuccess) return rfail(ro, HJB_E_NOMEM, "rollout: hipMalloc of %zu bytes failed", bytes);
        ro->data->allocs.push_back(d);
        if (hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "rollout: upload failed");
        *out = d;
        return HJB_OK;
    };
    void *dk = nullptr, *dr = nullptr, *du = nullptr, *dl = nullptr;
    int st = dev_upload(kk.data(), kk.size() * sizeof(double), &dk);
    if (!st) st = dev_upload(rdx.data(), rdx.size() * sizeof(double), &dr);
    if (!st) st = dev_upload(u_table, (size_t)n_ut * sizeof(double), &du);
    if (!st) st = dev_upload(labels, lab_bytes, &dl);
    if (!st && hipStreamCreateWithFlags(&ro->stream, hipStreamNonBlocking) != hipSuccess) st = rfail(ro, HJB_E_DEVICE, "rollout: stream creation failed");
    if (st) {
        release(ro);
        delete ro;
        return st;
    }
    R.knots = (const double *)dk;
    R.rdx = (const double *)dr;
    R.u_table = (const double *)du;
    R.labels = dl;
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
    DAttitude &M = ro->M;
    M = DAttitude{};
    M.h = h;
    const double J1 = inertia[0], J2 = inertia[1], J3 = inertia[2];
    M.J[0] = J1;
    M.J[1] = J2;
    M.J[2] = J3;
    M.c[0] = (J2 - J3) / J1;                          // spacecraft_dynamics_list :600-620
    M.c[1] = (J3 - J1) / J2;
    M.c[2] = (J1 - J2) / J3;
    if (q) std::memcpy(M.q, q, sizeof M.q);
    if (r) std::memcpy(M.r, r, sizeof M.r);
    ro->integrator = integrator;
    ro->model = kModelAttitude;
    drop_attached(ro);
    return HJB_OK;
}

int32_t hjb_rollout_set_pos_att_model(void *rollout_x, void *rollout_y, void *rollout_z, const double *inertia, double mass,
                                      double t_dist, double h, int32_t substeps, const double *rsw2eci, int32_t n_nodes,
                                      const double *orbit_coef) {
    Rollout *rx = (Rollout *)rollout_x, *ry = (Rollout *)rollout_y, *rz = (Rollout *)rollout_z;
    // the arguments that need no object first (decided without a device), then the objects
    if (!inertia || !rsw2eci || !orbit_coef) return rfail(rx, HJB_E_INVALID, "rollout: null argument (inertia, rsw2eci and orbit_coef are required)");
    if (!all_finite(inertia, 9)) return rfail(rx, HJB_E_INVALID, "rollout: inertia is not finite");
    if (!all_finite(rsw2eci, 9)) return rfail(rx, HJB_E_INVALID, "rollout: rsw2eci is not finite");
    if (!(std::isfinite(mass) && mass > 0)) return rfail(rx, HJB_E_INVALID, "rollout: mass = %g is not finite and > 0", mass);
    if (!std::isfinite(t_dist)) return rfail(rx, HJB_E_INVALID, "rollout: t_dist = %g is not finite", t_dist);
    if (!(std::isfinite(h) && h > 0)) return rfail(rx, HJB_E_INVALID, "rollout: h = %g is not finite and > 0", h);
    if (substeps < 1) return rfail(rx, HJB_E_INVALID, "rollout: substeps = %d < 1", substeps);
    if (n_nodes < 1 || (n_nodes - 1) % (2 * (int64_t)substeps) != 0)
        return rfail(rx, HJB_E_INVALID, "rollout: n_nodes = %d is not 2 * substeps * k + 1 (substeps = %d)", n_nodes, substeps);
    const int64_t bad = first_nonfinite(orbit_coef, 5 * (int64_t)n_nodes, true);
    if (bad >= 0) return rfail(rx, HJB_E_INVALID, "rollout: orbit_coef element %lld is not finite", (long long)bad);
    DPosAtt M{};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {                       // column-major in, row-major kept
            M.J[3 * r + c] = inertia[r + 3 * c];
            M.RSW[3 * r + c] = rsw2eci[r + 3 * c];
        }
    const double dj = pa_det3(M.J), dr = pa_det3(M.RSW);
    if (!(std::isfinite(dj) && dj != 0.0)) return rfail(rx, HJB_E_INVALID, "rollout: inertia is singular (determinant %g)", dj);
    if (!(std::isfinite(dr) && dr != 0.0)) return rfail(rx, HJB_E_INVALID, "rollout: rsw2eci is singular (determinant %g)", dr);
    pa_inv3(M.J, M.Jinv);
    pa_inv3(M.RSW, M.RSWinv);
    if (!all_finite(M.Jinv, 9)) return rfail(rx, HJB_E_INVALID, "rollout: inertia is singular (its inverse is not finite)");
    if (!all_finite(M.RSWinv, 9)) return rfail(rx, HJB_E_INVALID, "rollout: rsw2eci is singular (its inverse is not finite)");
    M.mass = mass;
    M.t_dist = t_dist;
    M.hs = h / substeps;
    M.substeps = substeps;
    auto pa = std::make_unique<PosAtt>();
    pa->M = M;
    pa->h = h;
    pa->max_steps = (int)((n_nodes - 1) / (2 * (int64_t)substeps));
    std::unique_lock<std::mutex> g;
    const int bad_chan = attach_channels({rx, ry, rz}, {"rollout_x", "rollout_y", "rollout_z"}, "pos-att", 4, 4, *pa, g);
    if (bad_chan) return bad_chan;
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(rx->device) != hipSuccess) return rfail(rx, HJB_E_DEVICE, "hipSetDevice failed");
    pa->coef = std::make_shared<DevData>();
    pa->coef->device = rx->device;
    const size_t cb = (size_t)5 * n_nodes * sizeof(double);
    void *d = nullptr;
    if (hipMalloc(&d, cb) != hipSuccess) return rfail(rx, HJB_E_NOMEM, "rollout: hipMalloc of %zu bytes failed", cb);
    pa->coef->allocs.push_back(d);
    if (hipMemcpy(d, orbit_coef, cb, hipMemcpyHostToDevice) != hipSuccess) return rfail(rx, HJB_E_DEVICE, "rollout: upload failed");
    pa->M.coef = (const double *)d;
    install_attached(rx, std::move(pa), kModelPosAtt);
    return HJB_OK;
}

int32_t hjb_rollout_set_pos_att_fault_controller(void *rollout_x, void *rollout_xf) {
    Rollout *rx = (Rollout *)rollout_x, *rf = (Rollout *)rollout_xf;
    if (!rx) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    if (rx == rf) return rfail(rx, HJB_E_INVALID, "rollout: the same object passed as channel x and as its fault controller");
    // the fault controller's snapshot first (its own lock), then channel x's lock
    ChanSnap sf;
    if (rf) sf = snap_channel(rf);
    std::lock_guard<std::mutex> g(rx->mu);
    if (rx->model != kModelPosAtt || !rx->att)
        return rfail(rx, HJB_E_INVALID, "rollout: the fault controller attaches to the pos-att model: call hjb_rollout_set_pos_att_model first");
    if (rf) {
        if (sf.D != 4 || sf.n_u != 4)
            return rfail(rx, HJB_E_INVALID, "rollout: the fault controller needs D == 4 and n_u == 4 (rollout_xf: D=%d, n_u=%d)", sf.D, sf.n_u);
        const int bad = check_channel(rx, sf, "rollout_xf", "rollout_x", "four controllers");
        if (bad) return bad;
    }
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(rx->device) != hipSuccess) return rfail(rx, HJB_E_DEVICE, "hipSetDevice failed");
    if (rx->stream) (void)hipStreamSynchronize(rx->stream);
    PosAtt &pa = static_cast<PosAtt &>(*rx->att);
    pa.has_xf = rf != nullptr;
    pa.cxf = sf.c;
    pa.data_xf = std::move(sf.data);                        // replaces (and releases) a fault controller attached earlier
    pa.planes_xf = sf.n_planes;
    return HJB_OK;
}

int32_t hjb_rollout_set_position_model(void *rollout_x, void *rollout_y, void *rollout_z, double tol, int32_t n_steps, int32_t max_sub,
                                       const int32_t *n_sub, const double *table) {
    Rollout *rx = (Rollout *)rollout_x, *ry = (Rollout *)rollout_y, *rz = (Rollout *)rollout_z;
    // the arguments that need no object first (decided without a device), then the objects
    if (!n_sub || !table) return rfail(rx, HJB_E_INVALID, "rollout: null argument (n_sub and table are required)");
    if (!(std::isfinite(tol) && tol > 0)) return rfail(rx, HJB_E_INVALID, "rollout: tol = %g is not finite and > 0", tol);
    if (n_steps < 1) return rfail(rx, HJB_E_INVALID, "rollout: n_steps = %d < 1 (the stages the table holds)", n_steps);
    if (max_sub < 1 || max_sub > HJB_POS_MAX_SUB)
        return rfail(rx, HJB_E_INVALID, "rollout: max_sub = %d not in 1..%d", max_sub, HJB_POS_MAX_SUB);
    for (int k = 0; k < n_steps; ++k)
        if (n_sub[k] < 1 || n_sub[k] > max_sub)
            return rfail(rx, HJB_E_INVALID, "rollout: n_sub[%d] = %d not in 1..%d (max_sub)", k, n_sub[k], max_sub);
    const int64_t n_tab = (int64_t)HJB_POS_ROW * max_sub * n_steps;
    const int64_t bad = first_nonfinite(table, n_tab, true);
    if (bad >= 0) return rfail(rx, HJB_E_INVALID, "rollout: table element %lld is not finite", (long long)bad);
    auto ps = std::make_unique<Position>();
    ps->M.tol = tol;
    ps->M.max_sub = max_sub;
    ps->max_steps = n_steps;
    std::unique_lock<std::mutex> g;
    const int bad_chan = attach_channels({rx, ry, rz}, {"rollout_x", "rollout_y", "rollout_z"}, "position", 2, 1, *ps, g);
    if (bad_chan) return bad_chan;
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(rx->device) != hipSuccess) return rfail(rx, HJB_E_DEVICE, "hipSetDevice failed");
    ps->table = std::make_shared<DevData>();
    ps->table->device = rx->device;
    const size_t tb = (size_t)n_tab * sizeof(double), nb = (size_t)n_steps * sizeof(int32_t);
    void *dt = nullptr, *dn = nullptr;
    if (hipMalloc(&dt, tb) != hipSuccess) return rfail(rx, HJB_E_NOMEM, "rollout: hipMalloc of %zu bytes failed", tb);
    ps->table->allocs.push_back(dt);
    if (hipMalloc(&dn, nb) != hipSuccess) return rfail(rx, HJB_E_NOMEM, "rollout: hipMalloc of %zu bytes failed", nb);
    ps->table->allocs.push_back(dn);
    if (hipMemcpy(dt, table, tb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dn, n_sub, nb, hipMemcpyHostToDevice) != hipSuccess)
        return rfail(rx, HJB_E_DEVICE, "rollout: upload failed");
    ps->M.table = (const double *)dt;
    ps->M.n_sub = (const int32_t *)dn;
    install_attached(rx, std::move(ps), kModelPosition);
    return HJB_OK;
}

int32_t hjb_rollout_set_attitude_simplified_model(void *rollout_1, void *rollout_2, void *rollout_3, const double *inertia, double h,
                                                  int32_t substeps, int32_t dynamics, const double *qw, const double *qt,
                                                  const double *r) {
    Rollout *r1 = (Rollout *)rollout_1, *r2 = (Rollout *)rollout_2, *r3 = (Rollout *)rollout_3;
    // the arguments that need no object first (decided without a device), then the objects
    if (!inertia) return rfail(r1, HJB_E_INVALID, "rollout: null argument (inertia is required)");
    if (!all_finite(inertia, 9)) return rfail(r1, HJB_E_INVALID, "rollout: inertia is not finite");
    if (!(std::isfinite(h) && h > 0)) return rfail(r1, HJB_E_INVALID, "rollout: h = %g is not finite and > 0", h);
    if (substeps < 1) return rfail(r1, HJB_E_INVALID, "rollout: substeps = %d < 1", substeps);
    if (dynamics != HJB_ATTS_FULL && dynamics != HJB_ATTS_DIAGONAL)
        return rfail(r1, HJB_E_INVALID, "rollout: dynamics %d is not HJB_ATTS_FULL / HJB_ATTS_DIAGONAL", dynamics);
    if (dynamics == HJB_ATTS_DIAGONAL && substeps != 1)
        return rfail(r1, HJB_E_INVALID, "rollout: substeps = %d with HJB_ATTS_DIAGONAL (one RK4 step per stage: substeps must be 1)", substeps);
    if (!all_finite(qw, 3)) return rfail(r1, HJB_E_INVALID, "rollout: qw is not finite");
    if (!all_finite(qt, 3)) return rfail(r1, HJB_E_INVALID, "rollout: qt is not finite");
    if (!all_finite(r, 3)) return rfail(r1, HJB_E_INVALID, "rollout: r is not finite");
    DAttSimplified M{};
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) M.J[3 * a + c] = inertia[a + 3 * c];       // column-major in, row-major kept
    const double dj = pa_det3(M.J);
    if (!(std::isfinite(dj) && dj != 0.0)) return rfail(r1, HJB_E_INVALID, "rollout: inertia is singular (determinant %g)", dj);
    pa_inv3(M.J, M.Jinv);
    if (!all_finite(M.Jinv, 9)) return rfail(r1, HJB_E_INVALID, "rollout: inertia is singular (its inverse is not finite)");
    const double J1 = M.J[0], J2 = M.J[4], J3 = M.J[8];
    if (dynamics == HJB_ATTS_DIAGONAL && !(J1 > 0 && J2 > 0 && J3 > 0))
        return rfail(r1, HJB_E_INVALID, "rollout: inertia has diagonal (%g, %g, %g), HJB_ATTS_DIAGONAL needs it > 0", J1, J2, J3);
    M.A.h = h;
    M.A.J[0] = J1;
    M.A.J[1] = J2;
    M.A.J[2] = J3;
    M.A.c[0] = (J2 - J3) / J1;                        // as hjb_rollout_set_attitude_model forms them
    M.A.c[1] = (J3 - J1) / J2;
    M.A.c[2] = (J1 - J2) / J3;
    if (qw) std::memcpy(M.qw, qw, sizeof M.qw);
    if (qt) std::memcpy(M.qt, qt, sizeof M.qt);
    if (r) std::memcpy(M.r, r, sizeof M.r);
    M.hs = h / substeps;
    M.substeps = substeps;
    auto as = std::make_unique<AttSimplified>();
    as->M = M;
    as->dynamics = dynamics;
    std::unique_lock<std::mutex> g;
    const int bad_chan = attach_channels({r1, r2, r3}, {"rollout_1", "rollout_2", "rollout_3"}, "simplified attitude", 2, 1, *as, g);
    if (bad_chan) return bad_chan;
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(r1->device) != hipSuccess) return rfail(r1, HJB_E_DEVICE, "hipSetDevice failed");
    install_attached(r1, std::move(as), kModelAttSimplified);
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
    Rollout *ro = (Rollout *)rollout;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    const int bad_arg = check_run(ro, kModelAffine, method, n_steps, plane_of_step, n_traj);
    if (bad_arg) return bad_arg;
    if (device_ms) *device_ms = 0.0;
    if (n_traj == 0) return HJB_OK;
    const int D = ro->D;
    const int bad_traj = check_traj(ro, "rollout", D, "D", n_steps, n_traj, X0, X_final);
    if (bad_traj) return bad_traj;
    const int idx_bytes = ro->idx_bytes;
    return run_chunks(ro, "hjb_rollout_run", D, ro->R.n_u, 0, n_steps, plane_of_step, n_traj, X0, X_final, cost, X_path, U_path, nullptr, nullptr,
                      device_ms,
                      [&](const DRollout &R, int64_t nc, size_t lds, bool lds_on, hipStream_t st, double *dX0, double *dXf, double *dC,
                          double *dXp, double *dUp, double *, int32_t *) {
                          return launch_rollout(idx_bytes, method, lds_on, D, R, nc, lds, st, dX0, dXf, dC, dXp, dUp);
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
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(ro->device) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipSetDevice failed");
    std::shared_ptr<DevData> nd;
    void *d = nullptr;
    if (n_nodes > 0) {
        nd = std::make_shared<DevData>();
        nd->device = ro->device;
        const size_t tb = tab.size() * sizeof(double);
        if (hipMalloc(&d, std::max<size_t>(tb, 16)) != hipSuccess) return rfail(ro, HJB_E_NOMEM, "rollout: hipMalloc of %zu bytes failed", tb);
        nd->allocs.push_back(d);
        if (tb && hipMemcpy(d, tab.data(), tb, hipMemcpyHostToDevice) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "rollout: upload failed");
    }
    if (ro->stream) (void)hipStreamSynchronize(ro->stream);
    ro->noise = std::move(nd);                                // replaces (and releases) a node set given earlier
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
    Rollout *ro = (Rollout *)rollout;
    // every refusal before any device work, the outputs untouched; the one that needs no object first
    if (first_stream < 0) return rfail(ro, HJB_E_INVALID, "hjb_rollout_run_noisy: first_stream=%lld < 0", (long long)first_stream);
    if (n_traj > 0 && first_stream > INT64_MAX - n_traj)
        return rfail(ro, HJB_E_INVALID, "hjb_rollout_run_noisy: first_stream + n_traj overflows (%lld + %lld)", (long long)first_stream,
                     (long long)n_traj);
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    const int bad_arg = check_run(ro, kModelAffine, method, n_steps, plane_of_step, n_traj);
    if (bad_arg) return bad_arg;
    if (ro->N.n_nodes < 1) return rfail(ro, HJB_E_INVALID, "rollout: hjb_rollout_run_noisy before hjb_rollout_set_noise");
    if (n_traj == 0) {
        if (device_ms) *device_ms = 0.0;
        return HJB_OK;
    }
    const int D = ro->D;
    const int bad_traj = check_traj(ro, "rollout", D, "D", n_steps, n_traj, X0, X_final);
    if (bad_traj) return bad_traj;
    if (device_ms) *device_ms = 0.0;
    const int idx_bytes = ro->idx_bytes;
    const bool lds_wanted = ro->lds;
    DNoise N = ro->N;
    N.seed = seed;
    int64_t chunk_i0 = 0;                                     // the chunk's offset in the call: streams count through the call
    return run_chunks(ro, "hjb_rollout_run_noisy", D, ro->R.n_u, 1, n_steps, plane_of_step, n_traj, X0, X_final, cost, X_path, U_path, W_path,
                      nullptr, device_ms,
                      [&](const DRollout &R, int64_t nc, size_t lds, bool, hipStream_t st, double *dX0, double *dXf, double *dC, double *dXp,
                          double *dUp, double *dWp, int32_t *) {
                          DNoise Nc = N;
                          Nc.first = (uint64_t)first_stream + (uint64_t)chunk_i0;
                          Nc.Wp = dWp;
                          const size_t lds_all = lds + (size_t)N.n_tab * sizeof(double);
                          return launch_rollout_noisy(idx_bytes, method, lds_wanted && lds_all <= kLdsMax, D, R, Nc, nc, lds_all, st, dX0,
                                                      dXf, dC, dXp, dUp);
                      },
                      [&](int64_t i0, int64_t, hipStream_t) {
                          chunk_i0 = i0;
                          return hipSuccess;
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
    if (first_stream < 0) return rfail(nullptr, HJB_E_INVALID, "%s: first_stream=%lld < 0", who, (long long)first_stream);
    if (n_traj < 0 || n_steps < 0) return rfail(nullptr, HJB_E_INVALID, "%s: n_traj=%lld, n_steps=%d (both >= 0)", who, (long long)n_traj, n_steps);
    if (n_traj > 0 && first_stream > INT64_MAX - n_traj)
        return rfail(nullptr, HJB_E_INVALID, "%s: first_stream + n_traj overflows (%lld + %lld)", who, (long long)first_stream, (long long)n_traj);
    if (n_nodes < 1 || n_nodes > HJB_DIST_MAX_NODES) return rfail(nullptr, HJB_E_INVALID, "%s: n_nodes=%d not in 1..%d", who, n_nodes, HJB_DIST_MAX_NODES);
    if (n_nodes > 1 && !thresholds) return rfail(nullptr, HJB_E_INVALID, "%s: null thresholds", who);
    if (n_traj > 0 && n_steps > 0 && !nodes) return rfail(nullptr, HJB_E_INVALID, "%s: null nodes", who);
    for (int w = 0; w + 1 < n_nodes; ++w)
        if (!(thresholds[w] >= 0 && thresholds[w] <= 4294967296.0) || (w > 0 && thresholds[w] < thresholds[w - 1]))
            return rfail(nullptr, HJB_E_INVALID, "%s: thresholds[%d] = %g is outside [0, 2^32] or below its predecessor", who, w, thresholds[w]);
    // the kernel's own loop: a Philox call when (k & 3) == 0, one word per step
    for (int64_t i = 0; i < n_traj; ++i) {
        const uint64_t s = (uint64_t)first_stream + (uint64_t)i;
        uint32_t rw[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k < n_steps; ++k) {
            if ((k & 3) == 0) noise_block(seed, s, (uint32_t)k >> 2, rw);
            nodes[i + n_traj * k] = noise_node(thresholds, n_nodes - 1, noise_next_word(rw));
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
    const size_t bytes = (size_t)nS * (size_t)n_planes * vb;
    std::shared_lock<std::shared_mutex> lk(g_capture_mu);
    if (hipSetDevice(ro->device) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipSetDevice failed");
    std::shared_ptr<DevData> vd;
    void *d = nullptr;
    if (n_planes > 0) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "hipMemGetInfo failed");
        if (bytes + ((size_t)64 << 20) > fr)
            return rfail(ro, HJB_E_NOMEM, "%s: %zu bytes of value planes, %zu free on device %d", who, bytes, fr, ro->device);
        vd = std::make_shared<DevData>();
        vd->device = ro->device;
        if (hipMalloc(&d, std::max<size_t>(bytes, 16)) != hipSuccess) return rfail(ro, HJB_E_NOMEM, "rollout: hipMalloc of %zu bytes failed", bytes);
        vd->allocs.push_back(d);
        if (hipMemcpy(d, values, bytes, hipMemcpyHostToDevice) != hipSuccess) return rfail(ro, HJB_E_DEVICE, "rollout: upload failed");
    }
    if (ro->stream) (void)hipStreamSynchronize(ro->stream);
    ro->values = std::move(vd);                               // replaces (and releases) planes given earlier
    ro->dvalues = d;
    ro->val_planes = n_planes;
    ro->val_bytes = vb;
    return HJB_OK;
}

int32_t hjb_rollout_run_greedy(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_traj, const double *X0,
                               double *X_final, double *cost, double *X_path, double *U_path, double *L_path, double *V_path,
                               double *device_ms) {
    Rollout *ro = (Rollout *)rollout;
    const char *const who = "hjb_rollout_run_greedy";
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    // every refusal before any device work, the outputs untouched
    if (n_steps < 0) return rfail(ro, HJB_E_INVALID, "rollout: n_steps=%d < 0", n_steps);
    if (n_traj < 0) return rfail(ro, HJB_E_INVALID, "rollout: n_traj=%lld < 0", (long long)n_traj);
    if (ro->model == kModelNone) return rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_model", who);
    if (ro->model != kModelAffine)
        return rfail(ro, HJB_E_INVALID, "rollout: %s needs the affine model (hjb_rollout_set_model); the object holds another", who);
    if (n_steps > 0 && !value_plane_of_step) return rfail(ro, HJB_E_INVALID, "rollout: null value_plane_of_step");
    for (int k = 0; k < n_steps; ++k) {
        const int32_t p = value_plane_of_step[k];
        if (p >= 0 && ro->val_planes < 1)
            return rfail(ro, HJB_E_INVALID, "rollout: %s before hjb_rollout_set_values (value_plane_of_step[%d] = %d; only -1 needs no values)",
                         who, k, p);
        if (p < -1 || p >= ro->val_planes)
            return rfail(ro, HJB_E_INVALID, "rollout: value_plane_of_step[%d] = %d outside [-1, %d)", k, p, ro->val_planes);
    }
    if (n_traj == 0) {
        if (device_ms) *device_ms = 0.0;
        return HJB_OK;
    }
    const int D = ro->D;
    const int bad_traj = check_traj(ro, "rollout", D, "D", n_steps, n_traj, X0, X_final);
    if (bad_traj) return bad_traj;
    if (device_ms) *device_ms = 0.0;
    // the two per-step scalars share run_chunks' extra path rows: [L | V], each [n_traj, n_steps]; one of them asked for goes
    // straight to its buffer, both go through one host block
    const int n_e = (L_path ? 1 : 0) + (V_path ? 1 : 0);
    const size_t per = (size_t)n_traj * (size_t)n_steps;
    std::vector<double> both;
    double *E_path = L_path ? L_path : V_path;
    if (n_e == 2) {
        both.resize(2 * per);
        E_path = both.data();
    }
    const int val_bytes = ro->val_bytes;
    const void *dvalues = ro->dvalues;
    const int st = run_chunks(ro, who, D, ro->R.n_u, n_e, n_steps, value_plane_of_step, n_traj, X0, X_final, cost, X_path, U_path, E_path,
                              nullptr, device_ms,
                              [&](const DRollout &R, int64_t nc, size_t lds, bool lds_on, hipStream_t s, double *dX0, double *dXf, double *dC,
                                  double *dXp, double *dUp, double *dEp, int32_t *) {
                                  DGreedy G{};
                                  G.R = R;
                                  G.values = dvalues;
                                  G.nc = nc;
                                  G.X0 = dX0;
                                  G.Xf = dXf;
                                  G.cost = dC;
                                  G.Xp = dXp;
                                  G.Up = dUp;
                                  G.Lp = L_path ? dEp : nullptr;
                                  G.Vp = V_path ? dEp + (L_path ? (size_t)nc * n_steps : 0) : nullptr;
                                  return launch_rollout_greedy(val_bytes, lds_on, D, G, lds, s);
                              });
    if (st == HJB_OK && n_e == 2) {
        std::memcpy(L_path, both.data(), per * sizeof(double));
        std::memcpy(V_path, both.data() + per, per * sizeof(double));
    }
    return st;
}

int32_t hjb_rollout_greedy_host(int32_t D, const int32_t *n, const double *knots, int32_t n_labels, int32_t n_u, const double *u_table,
                                const double *A, const double *B, const double *c, const double *q, const double *r, int32_t dtype,
                                int32_t n_value_planes, const void *values, int32_t n_steps, const int32_t *value_plane_of_step,
                                int64_t n_traj, const double *X0, double *X_final, double *cost, double *X_path, double *U_path,
                                double *L_path, double *V_path) {
    const char *const who = "hjb_rollout_greedy_host";
    if (D < 1 || D > HJB_MAX_D) return rfail(nullptr, HJB_E_UNSUPPORTED, "%s: D=%d not in 1..%d", who, D, HJB_MAX_D);
    if (n_u < 1 || n_u > HJB_ROLLOUT_MAX_U) return rfail(nullptr, HJB_E_UNSUPPORTED, "%s: n_u=%d not in 1..%d", who, n_u, HJB_ROLLOUT_MAX_U);
    if (!n || !knots || !u_table || !A || !B) return rfail(nullptr, HJB_E_INVALID, "%s: null argument (n, knots, u_table, A and B are required)", who);
    if (n_labels < 1) return rfail(nullptr, HJB_E_INVALID, "%s: n_labels=%d < 1", who, n_labels);
    if (dtype != HJB_F32 && dtype != HJB_F64) return rfail(nullptr, HJB_E_INVALID, "%s: dtype %d is not HJB_F32 / HJB_F64", who, dtype);
    if (n_value_planes < 0) return rfail(nullptr, HJB_E_INVALID, "%s: n_value_planes=%d < 0", who, n_value_planes);
    if (n_value_planes > 0 && !values) return rfail(nullptr, HJB_E_INVALID, "%s: null values with n_value_planes=%d", who, n_value_planes);
    if (n_steps < 0 || n_traj < 0) return rfail(nullptr, HJB_E_INVALID, "%s: n_steps=%d, n_traj=%lld (both >= 0)", who, n_steps, (long long)n_traj);
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
    if (!all_finite(u_table, (int64_t)n_labels * n_u)) return rfail(nullptr, HJB_E_INVALID, "%s: u_table is not finite", who);
    if (!all_finite(A, (int64_t)D * D) || !all_finite(B, (int64_t)D * n_u) || !all_finite(c, D) || !all_finite(q, D) || !all_finite(r, n_u))
        return rfail(nullptr, HJB_E_INVALID, "%s: the model (A, B, c, q, r) is not finite", who);
    if (n_steps > 0 && !value_plane_of_step) return rfail(nullptr, HJB_E_INVALID, "%s: null value_plane_of_step", who);
    for (int k = 0; k < n_steps; ++k)
        if (value_plane_of_step[k] < -1 || value_plane_of_step[k] >= n_value_planes)
            return rfail(nullptr, HJB_E_INVALID, "%s: value_plane_of_step[%d] = %d outside [-1, %d)", who, k, value_plane_of_step[k], n_value_planes);
    if (n_traj == 0) return HJB_OK;
    const int bad_traj = check_traj(nullptr, who, D, "D", n_steps, n_traj, X0, X_final);
    if (bad_traj) return bad_traj;
    GreedyModel M{};
    std::vector<double> rdx((size_t)n_knots);
    greedy_grid(D, n, knots, M, rdx.data());
    M.n_u = n_u;
    M.n_labels = n_labels;
    M.has_c = c ? 1 : 0;
    std::memcpy(M.A, A, sizeof(double) * D * D);
    std::memcpy(M.B, B, sizeof(double) * D * n_u);
    if (c) std::memcpy(M.c, c, sizeof(double) * D);
    if (q) std::memcpy(M.q, q, sizeof(double) * D);
    if (r) std::memcpy(M.r, r, sizeof(double) * n_u);
    with_bool(dtype == HJB_F32, [&](auto f) {
        with_dim(D, [&](auto d) {
            using TV = std::conditional_t<decltype(f)::value, float, double>;
            greedy_rollout_host<decltype(d)::value, TV>(M, knots, rdx.data(), u_table, static_cast<const TV *>(values), n_steps,
                                                        value_plane_of_step, n_traj, X0, X_final, cost, X_path, U_path, L_path, V_path);
        });
    });
    return HJB_OK;
}

int32_t hjb_rollout_run_attitude(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                 const double *X0, double *X_final, double *cost, double *X_path, double *U_path, double *A_path,
                                 double *device_ms) {
    Rollout *ro = (Rollout *)rollout;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    const int bad_arg = check_run(ro, kModelAttitude, method, n_steps, plane_of_step, n_traj);
    if (bad_arg) return bad_arg;
    if (device_ms) *device_ms = 0.0;
    if (n_traj == 0) return HJB_OK;
    int bad_traj = check_traj(ro, "rollout", HJB_ATT_W, "7", n_steps, n_traj, X0, X_final);
    if (!bad_traj) bad_traj = check_quaternions(ro, "rollout", n_traj, X0);
    if (bad_traj) return bad_traj;
    const int idx_bytes = ro->idx_bytes, integ = ro->integrator;
    const DAttitude M = ro->M;
    return run_chunks(ro, "hjb_rollout_run_attitude", HJB_ATT_W, HJB_ATT_U, 3, n_steps, plane_of_step, n_traj, X0, X_final, cost, X_path, U_path,
                      A_path, nullptr, device_ms,
                      [&](const DRollout &R, int64_t nc, size_t lds, bool lds_on, hipStream_t st, double *dX0, double *dXf, double *dC,
                          double *dXp, double *dUp, double *dAp, int32_t *) {
                          return launch_rollout_attitude(idx_bytes, method, lds_on, integ, R, M, nc, lds, st, dX0, dXf, dC, dXp, dUp, dAp);
                      });
}

int32_t hjb_rollout_run_pos_att(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj, const double *X0,
                                double *X_final, double *X_path, double *F_path, double *FM_path) {
    Rollout *ro = (Rollout *)rollout_x;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    const int bad_arg = check_run(ro, kModelPosAtt, HJB_LOOKUP_NEAREST, n_steps, plane_of_step, n_traj);
    if (bad_arg) return bad_arg;
    const PosAtt &pa = static_cast<const PosAtt &>(*ro->att);
    if (n_steps > pa.max_steps)
        return rfail(ro, HJB_E_INVALID, "rollout: n_steps = %d, the orbit table covers %d stages ((n_nodes - 1) / (2 substeps))", n_steps,
                     pa.max_steps);
    if (n_traj == 0) return HJB_OK;
    const int bad_traj = check_traj(ro, "rollout", HJB_PA_W, "13", n_steps, n_traj, X0, X_final);
    if (bad_traj) return bad_traj;
    const int idx_bytes = ro->idx_bytes;
    const DPaChan cx0 = pa_channel(ro->R);
    const size_t lds3 = lds_bytes({&cx0, &pa.c[0], &pa.c[1]}, 4);
    const bool lds3_on = ro->lds && lds3 <= kLdsMax;
    return run_chunks(ro, "hjb_rollout_run_pos_att", HJB_PA_W, HJB_PA_F, HJB_PA_FM, n_steps, plane_of_step, n_traj, X0, X_final, nullptr,
                      X_path, F_path, FM_path, nullptr, nullptr,
                      [&](const DRollout &R, int64_t nc, size_t, bool, hipStream_t st, double *dX0, double *dXf, double *, double *dXp,
                          double *dFp, double *dFMp, int32_t *) {
                          const int32_t *pl = R.plane_of_step;
                          DPosAtt M = pa.M;
                          M.n_steps = R.n_steps;
                          return launch_rollout_pos_att(idx_bytes, lds3_on, on_planes(cx0, pl), on_planes(pa.c[0], pl), on_planes(pa.c[1], pl),
                                                        M, nc, lds3, st, dX0, dXf, dXp, dFp, dFMp);
                      });
}

int32_t hjb_rollout_run_pos_att_faults(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                       const double *X0, const int32_t *fault_mask, const int32_t *fault_stage,
                                       const int32_t *switch_stage, double pos_tol, double att_tol, double *X_final, double *impulse,
                                       int32_t *settle_stage, double *X_path, double *F_path, double *FM_path, double *device_ms) {
    Rollout *ro = (Rollout *)rollout_x;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    // every refusal before any device work, the outputs untouched
    const int bad_arg = check_run(ro, kModelPosAtt, HJB_LOOKUP_NEAREST, n_steps, plane_of_step, n_traj);
    if (bad_arg) return bad_arg;
    const PosAtt &pa = static_cast<const PosAtt &>(*ro->att);
    if (n_steps > pa.max_steps)
        return rfail(ro, HJB_E_INVALID, "rollout: n_steps = %d, the orbit table covers %d stages ((n_nodes - 1) / (2 substeps))", n_steps,
                     pa.max_steps);
    if (pa.has_xf)
        for (int k = 0; k < n_steps; ++k)
            if (plane_of_step[k] >= pa.planes_xf)
                return rfail(ro, HJB_E_INVALID, "rollout: plane_of_step[%d] = %d outside [0, %d) (the fault controller's planes)", k,
                             plane_of_step[k], pa.planes_xf);
    if (!(pos_tol >= 0)) return rfail(ro, HJB_E_INVALID, "rollout: pos_tol = %g is NaN or negative", pos_tol);
    if (!(att_tol >= 0)) return rfail(ro, HJB_E_INVALID, "rollout: att_tol = %g is NaN or negative", att_tol);
    if (n_traj == 0) {
        if (device_ms) *device_ms = 0.0;
        return HJB_OK;
    }
    const int bad_traj = check_traj(ro, "rollout", HJB_PA_W, "13", n_steps, n_traj, X0, X_final);
    if (bad_traj) return bad_traj;
    for (int64_t i = 0; i < n_traj; ++i) {
        if (fault_mask && (fault_mask[i] & ~0xFFF))
            return rfail(ro, HJB_E_INVALID, "rollout: fault_mask[%lld] = 0x%x has a bit above 11 (twelve thrusters)", (long long)i,
                         (unsigned)fault_mask[i]);
        if (fault_stage && fault_stage[i] < 0)
            return rfail(ro, HJB_E_INVALID, "rollout: fault_stage[%lld] = %d < 0", (long long)i, fault_stage[i]);
        if (switch_stage && switch_stage[i] < 0)
            return rfail(ro, HJB_E_INVALID, "rollout: switch_stage[%lld] = %d < 0", (long long)i, switch_stage[i]);
        if (switch_stage && switch_stage[i] < n_steps && !pa.has_xf)
            return rfail(ro, HJB_E_INVALID, "rollout: switch_stage[%lld] = %d hands over within the %d stages, but no fault controller is "
                         "attached (hjb_rollout_set_pos_att_fault_controller)", (long long)i, switch_stage[i], n_steps);
    }
    const int idx_bytes = ro->idx_bytes;
    const DPaChan cx0 = pa_channel(ro->R);
    const size_t lds4 = lds_bytes({&cx0, &pa.c[0], &pa.c[1], &pa.cxf}, 4);
    const bool lds4_on = ro->lds && lds4 <= kLdsMax;
    DPaFault Q{};
    Q.h = pa.h;
    Q.p2 = pos_tol * pos_tol;
    Q.a2 = att_tol * att_tol;
    // the per-trajectory inputs on the device: allocated at the first chunk (for the largest), uploaded per chunk at its offset
    const int32_t *const host_in[3] = {fault_mask, fault_stage, switch_stage};
    int32_t *dev_in[3] = {nullptr, nullptr, nullptr};
    const int64_t nc_max = std::min(n_traj, ro->chunk);
    const int st = run_chunks(ro, "hjb_rollout_run_pos_att_faults", HJB_PA_W, HJB_PA_F, HJB_PA_FM, n_steps, plane_of_step, n_traj, X0, X_final,
                              impulse, X_path, F_path, FM_path, settle_stage, device_ms,
                              [&](const DRollout &R, int64_t nc, size_t, bool, hipStream_t s, double *dX0, double *dXf, double *dImp, double *dXp,
                                  double *dFp, double *dFMp, int32_t *dSettle) {
                                  const int32_t *pl = R.plane_of_step;
                                  DPosAtt M = pa.M;
                                  M.n_steps = R.n_steps;
                                  DPaFault Qc = Q;
                                  Qc.mask = dev_in[0];
                                  Qc.fault_stage = dev_in[1];
                                  Qc.switch_stage = dev_in[2];
                                  Qc.impulse = dImp;
                                  Qc.settle = dSettle;
                                  return launch_rollout_pos_att_faults(idx_bytes, lds4_on, on_planes(cx0, pl), on_planes(pa.c[0], pl),
                                                                       on_planes(pa.c[1], pl), on_planes(pa.cxf, pl), M, Qc, nc, lds4, s,
                                                                       dX0, dXf, dXp, dFp, dFMp);
                              },
                              [&](int64_t i0, int64_t nc, hipStream_t s) {
                                  for (int t = 0; t < 3; ++t) {
                                      if (!host_in[t]) continue;
                                      hipError_t e = hipSuccess;
                                      if (!dev_in[t]) e = hipMalloc((void **)&dev_in[t], (size_t)nc_max * sizeof(int32_t));
                                      if (e == hipSuccess)
                                          e = hipMemcpyAsync(dev_in[t], host_in[t] + i0, (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice, s);
                                      if (e != hipSuccess) return e;
                                  }
                                  return hipSuccess;
                              });
    {
        std::shared_lock<std::shared_mutex> lk(g_capture_mu);
        (void)hipSetDevice(ro->device);
        for (int32_t *p : dev_in)
            if (p) (void)hipFree(p);
    }
    return st;
}

int32_t hjb_rollout_run_position(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj, const double *X0,
                                 double *X_final, double *X_path, double *A_path, int32_t *off_schedule) {
    Rollout *ro = (Rollout *)rollout_x;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    const int bad_arg = check_run(ro, kModelPosition, HJB_LOOKUP_NEAREST, n_steps, plane_of_step, n_traj);
    if (bad_arg) return bad_arg;
    const Position &ps = static_cast<const Position &>(*ro->att);
    if (n_steps > ps.max_steps)
        return rfail(ro, HJB_E_INVALID, "rollout: n_steps = %d, the RKF45 table covers %d stages", n_steps, ps.max_steps);
    if (n_traj == 0) return HJB_OK;
    // this entry point's own null check (off_schedule is required): check_traj's of X0 / X_final cannot fire after it
    if (!X0 || !X_final || !off_schedule) return rfail(ro, HJB_E_INVALID, "rollout: null X0 / X_final / off_schedule");
    const int bad_traj = check_traj(ro, "rollout", HJB_POS_W, "6", n_steps, n_traj, X0, X_final);
    if (bad_traj) return bad_traj;
    const int idx_bytes = ro->idx_bytes;
    const DPaChan cx0 = pa_channel(ro->R);
    const size_t lds3 = lds_bytes({&cx0, &ps.c[0], &ps.c[1]}, 1);
    const bool lds3_on = ro->lds && lds3 <= kLdsMax;
    return run_chunks(ro, "hjb_rollout_run_position", HJB_POS_W, HJB_POS_A, 0, n_steps, plane_of_step, n_traj, X0, X_final, nullptr,
                      X_path, A_path, nullptr, off_schedule, nullptr,
                      [&](const DRollout &R, int64_t nc, size_t, bool, hipStream_t st, double *dX0, double *dXf, double *, double *dXp,
                          double *dAp, double *, int32_t *dOff) {
                          const int32_t *pl = R.plane_of_step;
                          DPosition M = ps.M;
                          M.n_steps = R.n_steps;
                          return launch_rollout_position(idx_bytes, lds3_on, on_planes(cx0, pl), on_planes(ps.c[0], pl), on_planes(ps.c[1], pl),
                                                         M, nc, lds3, st, dX0, dXf, dXp, dAp, dOff);
                      });
}

int32_t hjb_rollout_run_attitude_simplified(void *rollout_1, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                            const double *X0, double *X_final, double *cost, double *X_path, double *U_path,
                                            double *A_path) {
    Rollout *ro = (Rollout *)rollout_1;
    if (!ro) return rfail(nullptr, HJB_E_INVALID, "rollout: null handle");
    std::lock_guard<std::mutex> g(ro->mu);
    const int bad_arg = check_run(ro, kModelAttSimplified, HJB_LOOKUP_NEAREST, n_steps, plane_of_step, n_traj);
    if (bad_arg) return bad_arg;
    const AttSimplified &as = static_cast<const AttSimplified &>(*ro->att);
    if (n_traj == 0) return HJB_OK;
    const int bad_traj = check_traj(ro, "rollout", HJB_ATT_W, "7", n_steps, n_traj, X0, X_final);
    if (bad_traj) return bad_traj;
    const int idx_bytes = ro->idx_bytes;
    const DPaChan c10 = pa_channel(ro->R);
    const size_t lds3 = lds_bytes({&c10, &as.c[0], &as.c[1]}, 1);
    const bool lds3_on = ro->lds && lds3 <= kLdsMax;
    return run_chunks(ro, "hjb_rollout_run_attitude_simplified", HJB_ATT_W, HJB_ATT_U, 3, n_steps, plane_of_step, n_traj, X0, X_final, cost,
                      X_path, U_path, A_path, nullptr, nullptr,
                      [&](const DRollout &R, int64_t nc, size_t, bool, hipStream_t st, double *dX0, double *dXf, double *dC, double *dXp,
                          double *dUp, double *dAp, int32_t *) {
                          const int32_t *pl = R.plane_of_step;
                          DAttSimplified M = as.M;
                          M.n_steps = R.n_steps;
                          return launch_rollout_attitude_simplified(idx_bytes, lds3_on, as.dynamics, on_planes(c10, pl), on_planes(as.c[0], pl),
                                                                    on_planes(as.c[1], pl), M, nc, lds3, st, dX0, dXf, dC, dXp, dUp, dAp);
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
    M.A.h = h;
    const double J1 = inertia[0], J2 = inertia[1], J3 = inertia[2];
    M.A.J[0] = J1;
    M.A.J[1] = J2;
    M.A.J[2] = J3;
    M.A.c[0] = (J2 - J3) / J1;                        // as hjb_rollout_set_attitude_model forms them
    M.A.c[1] = (J3 - J1) / J2;
    M.A.c[2] = (J1 - J2) / J3;
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
    const int st = run_chunks(&ro, who, HJB_ATT_W, HJB_ATT_U, 3, n_steps, nullptr, n_traj, X0, X_final, cost, X_path, U_path, A_path,
                              nullptr, device_ms,
                              [&](const DRollout &R, int64_t nc, size_t, bool, hipStream_t s, double *dX0, double *dXf, double *dC,
                                  double *dXp, double *dUp, double *dAp, int32_t *) {
                                  DAttLinear Mk = M;
                                  Mk.n_steps = R.n_steps;
                                  return launch_rollout_attitude_linear(integrator, cost_form, Mk, nc, s, dX0, dXf, dC, dXp, dUp, dAp);
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
