// rollout_channels.hip - the rollout models that attach two more objects' policies as channels (rollout_host.h: the object, the
// refusals and the chunk loop, defined in rollout.hip):
//   pos-att (K18, kernels_rollout_pos_att.h / rollout_pos_att.hip; its fault campaigns K23, kernels_rollout_pos_att_faults.h /
//   rollout_pos_att_faults.hip), position (K19, kernels_rollout_position.h / rollout_position.hip), simplified attitude (K20,
//   kernels_rollout_attitude_simplified.h / rollout_attitude_simplified.hip).
// Here: the models' records on top of Attached, attach_channels (the three attaching setters share it), the fault-controller
// setter and the four run functions.
#include "rollout_host.h"
#include "kernels_rollout_pos_att_faults.h"
#include "kernels_rollout_position.h"
#include "kernels_rollout_attitude_simplified.h"

using namespace hjbhost;

namespace {

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

// The channels of a chunk's launch: the object's own policy, the two it has attached and `extra` (the fault controller's; null:
// three channels), each on the chunk's planes; the LDS bytes of their [knots | 1/dx | u_table], `width` u_table doubles per
// label, and the placement (option "lds" and the bytes fit kLdsMax).  Under ro->mu.
struct Channels {
    DPaChan c[4];
    size_t lds;
    bool lds_on;
};

Channels channels(const Rollout *ro, const Chunk &k, int width, const DPaChan *extra = nullptr) {
    Channels ch{{pa_channel(ro->R), ro->att->c[0], ro->att->c[1], extra ? *extra : DPaChan{}}};
    int64_t nk = 0, nl = 0;
    for (DPaChan &c : ch.c) {
        c.plane_of_step = k.R.plane_of_step;
        nk += c.n_knots;
        nl += c.n_labels;
    }
    ch.lds = (size_t)(2 * nk + width * nl) * sizeof(double);
    ch.lds_on = ro->lds && ch.lds <= kLdsMax;
    return ch;
}

// a model's record for a chunk: the stages the call runs
template <typename TM>
TM for_chunk(TM M, const Chunk &k) {
    M.n_steps = k.R.n_steps;
    return M;
}

// the model of three channels an object holds, as its run function reads it (check_run has passed: att is of that type)
template <typename TA>
const TA &attached(const Rollout *ro) {
    return static_cast<const TA &>(*ro->att);
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

// A model's 3x3 matrices (`name` in the messages): column-major in, row-major kept in `rows`, with the inverse.  A singular one
// is refused: every determinant first, then every inverse, in the order given.
struct Mat3 {
    const char *name;
    const double *in;
    double (&rows)[9], (&inv)[9];
};

int invert3(Rollout *ro, std::initializer_list<Mat3> ms) {
    for (const Mat3 &m : ms) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) m.rows[3 * r + c] = m.in[r + 3 * c];
        const double d = pa_det3(m.rows);
        if (!(std::isfinite(d) && d != 0.0)) return rfail(ro, HJB_E_INVALID, "rollout: %s is singular (determinant %g)", m.name, d);
    }
    for (const Mat3 &m : ms) {
        pa_inv3(m.rows, m.inv);
        if (!all_finite(m.inv, 9)) return rfail(ro, HJB_E_INVALID, "rollout: %s is singular (its inverse is not finite)", m.name);
    }
    return HJB_OK;
}

// What both pos-att run functions refuse under the lock: check_run's, then more stages than the orbit table covers
int check_pos_att_run(Rollout *ro, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj) {
    if (const int bad = check_run(ro, kModelPosAtt, HJB_LOOKUP_NEAREST, n_steps, plane_of_step, n_traj)) return bad;
    const int max_steps = attached<PosAtt>(ro).max_steps;
    if (n_steps > max_steps)
        return rfail(ro, HJB_E_INVALID, "rollout: n_steps = %d, the orbit table covers %d stages ((n_nodes - 1) / (2 substeps))", n_steps, max_steps);
    return HJB_OK;
}

}  // namespace

extern "C" {

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
    if (const int singular = invert3(rx, {{"inertia", inertia, M.J, M.Jinv}, {"rsw2eci", rsw2eci, M.RSW, M.RSWinv}})) return singular;
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
    pa->coef = std::make_shared<DevData>(rx->device);
    if (const int st = upload(rx, *pa->coef, orbit_coef, (size_t)5 * n_nodes * sizeof(double), (const void **)&pa->M.coef)) return st;
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
    ps->table = std::make_shared<DevData>(rx->device);
    int st = upload(rx, *ps->table, table, (size_t)n_tab * sizeof(double), (const void **)&ps->M.table);
    if (!st) st = upload(rx, *ps->table, n_sub, (size_t)n_steps * sizeof(int32_t), (const void **)&ps->M.n_sub);
    if (st) return st;
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
    if (const int singular = invert3(r1, {{"inertia", inertia, M.J, M.Jinv}})) return singular;
    const double J1 = M.J[0], J2 = M.J[4], J3 = M.J[8];
    if (dynamics == HJB_ATTS_DIAGONAL && !(J1 > 0 && J2 > 0 && J3 > 0))
        return rfail(r1, HJB_E_INVALID, "rollout: inertia has diagonal (%g, %g, %g), HJB_ATTS_DIAGONAL needs it > 0", J1, J2, J3);
    M.A = euler_attitude(J1, J2, J3, h);
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

int32_t hjb_rollout_run_pos_att(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj, const double *X0,
                                double *X_final, double *X_path, double *F_path, double *FM_path) {
    const Rollout *ro = (const Rollout *)rollout_x;
    const ChunkPlan plan{{"hjb_rollout_run_pos_att", HJB_PA_W, "13", n_steps, plane_of_step, n_traj, X0, X_final, nullptr},
                         {{X_path, HJB_PA_W, n_steps + 1}, {F_path, HJB_PA_F, n_steps}, {FM_path, HJB_PA_FM, n_steps}}};
    return run_call(
        rollout_x, plan, nullptr, [&](Rollout *o) { return check_pos_att_run(o, n_steps, plane_of_step, n_traj); }, nullptr,
        [&](const Chunk &c) {
            const Channels ch = channels(ro, c, 4);
            return launch_rollout_pos_att(ro->idx_bytes, ch.lds_on, ch.c[0], ch.c[1], ch.c[2], for_chunk(attached<PosAtt>(ro).M, c), c.nc, ch.lds,
                                          c.st, c.X0, c.Xf, c.path[0], c.path[1], c.path[2]);
        });
}

int32_t hjb_rollout_run_pos_att_faults(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                       const double *X0, const int32_t *fault_mask, const int32_t *fault_stage,
                                       const int32_t *switch_stage, double pos_tol, double att_tol, double *X_final, double *impulse,
                                       int32_t *settle_stage, double *X_path, double *F_path, double *FM_path, double *device_ms) {
    const Rollout *ro = (const Rollout *)rollout_x;
    const ChunkPlan plan{{"hjb_rollout_run_pos_att_faults", HJB_PA_W, "13", n_steps, plane_of_step, n_traj, X0, X_final, device_ms},
                         {{X_path, HJB_PA_W, n_steps + 1}, {F_path, HJB_PA_F, n_steps}, {FM_path, HJB_PA_FM, n_steps}}, impulse, settle_stage,
                         {fault_mask, fault_stage, switch_stage}};
    return run_call(
        rollout_x, plan, nullptr,
        [&](Rollout *o) {
            if (const int bad = check_pos_att_run(o, n_steps, plane_of_step, n_traj)) return bad;
            const PosAtt &pa = attached<PosAtt>(o);
            if (pa.has_xf)
                for (int k = 0; k < n_steps; ++k)
                    if (plane_of_step[k] >= pa.planes_xf)
                        return rfail(o, HJB_E_INVALID, "rollout: plane_of_step[%d] = %d outside [0, %d) (the fault controller's planes)", k,
                                     plane_of_step[k], pa.planes_xf);
            if (!(pos_tol >= 0)) return rfail(o, HJB_E_INVALID, "rollout: pos_tol = %g is NaN or negative", pos_tol);
            if (!(att_tol >= 0)) return rfail(o, HJB_E_INVALID, "rollout: att_tol = %g is NaN or negative", att_tol);
            return HJB_OK;
        },
        [&](Rollout *o) {
            const bool has_xf = attached<PosAtt>(o).has_xf;
            for (int64_t i = 0; i < n_traj; ++i) {
                if (fault_mask && (fault_mask[i] & ~0xFFF))
                    return rfail(o, HJB_E_INVALID, "rollout: fault_mask[%lld] = 0x%x has a bit above 11 (twelve thrusters)", (long long)i,
                                 (unsigned)fault_mask[i]);
                if (fault_stage && fault_stage[i] < 0)
                    return rfail(o, HJB_E_INVALID, "rollout: fault_stage[%lld] = %d < 0", (long long)i, fault_stage[i]);
                if (switch_stage && switch_stage[i] < 0)
                    return rfail(o, HJB_E_INVALID, "rollout: switch_stage[%lld] = %d < 0", (long long)i, switch_stage[i]);
                if (switch_stage && switch_stage[i] < n_steps && !has_xf)
                    return rfail(o, HJB_E_INVALID, "rollout: switch_stage[%lld] = %d hands over within the %d stages, but no fault controller is "
                                 "attached (hjb_rollout_set_pos_att_fault_controller)", (long long)i, switch_stage[i], n_steps);
            }
            return HJB_OK;
        },
        [&](const Chunk &c) {
            const PosAtt &pa = attached<PosAtt>(ro);
            const Channels ch = channels(ro, c, 4, &pa.cxf);
            DPaFault Q{};
            Q.h = pa.h;
            Q.p2 = pos_tol * pos_tol;
            Q.a2 = att_tol * att_tol;
            Q.mask = c.input[0];
            Q.fault_stage = c.input[1];
            Q.switch_stage = c.input[2];
            Q.impulse = c.cost;
            Q.settle = c.flags;
            return launch_rollout_pos_att_faults(ro->idx_bytes, ch.lds_on, ch.c[0], ch.c[1], ch.c[2], ch.c[3], for_chunk(pa.M, c), Q, c.nc, ch.lds,
                                                 c.st, c.X0, c.Xf, c.path[0], c.path[1], c.path[2]);
        });
}

int32_t hjb_rollout_run_position(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj, const double *X0,
                                 double *X_final, double *X_path, double *A_path, int32_t *off_schedule) {
    const Rollout *ro = (const Rollout *)rollout_x;
    const ChunkPlan plan{{"hjb_rollout_run_position", HJB_POS_W, "6", n_steps, plane_of_step, n_traj, X0, X_final, nullptr},
                         {{X_path, HJB_POS_W, n_steps + 1}, {A_path, HJB_POS_A, n_steps}}, nullptr, off_schedule};
    return run_call(
        rollout_x, plan, nullptr,
        [&](Rollout *o) {
            if (const int bad = check_run(o, kModelPosition, HJB_LOOKUP_NEAREST, n_steps, plane_of_step, n_traj)) return bad;
            const int max_steps = attached<Position>(o).max_steps;
            if (n_steps > max_steps) return rfail(o, HJB_E_INVALID, "rollout: n_steps = %d, the RKF45 table covers %d stages", n_steps, max_steps);
            // this entry point's own null check, the last before the empty call, which needs none of the three (off_schedule is
            // required): check_traj's of X0 / X_final cannot fire after it
            if (n_traj > 0 && (!X0 || !X_final || !off_schedule)) return rfail(o, HJB_E_INVALID, "rollout: null X0 / X_final / off_schedule");
            return HJB_OK;
        },
        nullptr,
        [&](const Chunk &c) {
            const Channels ch = channels(ro, c, 1);
            return launch_rollout_position(ro->idx_bytes, ch.lds_on, ch.c[0], ch.c[1], ch.c[2], for_chunk(attached<Position>(ro).M, c), c.nc, ch.lds,
                                           c.st, c.X0, c.Xf, c.path[0], c.path[1], c.flags);
        });
}

int32_t hjb_rollout_run_attitude_simplified(void *rollout_1, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                            const double *X0, double *X_final, double *cost, double *X_path, double *U_path,
                                            double *A_path) {
    const Rollout *ro = (const Rollout *)rollout_1;
    const ChunkPlan plan{{"hjb_rollout_run_attitude_simplified", HJB_ATT_W, "7", n_steps, plane_of_step, n_traj, X0, X_final, nullptr},
                         {{X_path, HJB_ATT_W, n_steps + 1}, {U_path, HJB_ATT_U, n_steps}, {A_path, 3, n_steps}}, cost};
    return run_call(
        rollout_1, plan, nullptr, [&](Rollout *o) { return check_run(o, kModelAttSimplified, HJB_LOOKUP_NEAREST, n_steps, plane_of_step, n_traj); },
        nullptr, [&](const Chunk &c) {
            const AttSimplified &as = attached<AttSimplified>(ro);
            const Channels ch = channels(ro, c, 1);
            return launch_rollout_attitude_simplified(ro->idx_bytes, ch.lds_on, as.dynamics, ch.c[0], ch.c[1], ch.c[2], for_chunk(as.M, c), c.nc,
                                                      ch.lds, c.st, c.X0, c.Xf, c.cost, c.path[0], c.path[1], c.path[2]);
        });
}

}  // extern "C"
