// rollout_host.h - what the host units of the rollouts share (host only; include/hjbdp.h is the public ABI): the object,
// its refusals, the upload, the chunk loop with the run functions' entry frame (run_call), and the campaigns' entry frame and
// device loop.  Defined in rollout.hip (the campaigns' checks, frame and loop: rollout_campaign_host.hip); rollout_channels.hip,
// rollout_ctrl_lookahead_host.hip and the four rollout_*campaign*_host.hip are the other readers.
// The frame of the nine run functions, stated once (run_call): every refusal before any device work and in one order, the
// outputs untouched - what needs no object, the null handle, the object's lock, the controller's checks, the empty call, the
// trajectories, what is refused per trajectory - then the chunk loop.  An entry point is its hooks, its plan and its launch.
#pragma once
#include "hjbdp_host.h"
// the records an object holds: DRollout, DAttitude, DNoise, DActuator, DPaChan (a unit includes the other kernel headers whose launch it calls)
#include "kernels_rollout.h"
#include "kernels_rollout_attitude.h"
#include "kernels_rollout_noisy.h"
#include "kernels_rollout_actuator.h"
#include "kernels_rollout_campaign.h"
#include "kernels_rollout_campaign_hist.h"
#include "kernels_rollout_pos_att.h"
#include "kernels_rollout_greedy.h"
#include "hjbdp_lookahead.h"
#include "hjbdp_ctrl_lookahead.h"
#include <functional>
#include <memory>

namespace hjbhost {

// the model an object holds: the last setter called wins.  The last three keep an Attached record in Rollout::att, the others none
enum { kModelNone = 0, kModelAffine = 1, kModelAttitude = 2, kModelPosAtt = 3, kModelPosition = 4, kModelAttSimplified = 5 };

// Device allocations with shared ownership: an object's grid, table and labels live as long as the object or a pos-att, position
// or simplified attitude model that reads them (hjb_rollout_set_pos_att_model / hjb_rollout_set_position_model /
// hjb_rollout_set_attitude_simplified_model on another object) does.  Freed under the
// last owner's locks (destroy / set_*model).
struct DevData {
    int device;
    std::vector<void *> allocs;
    explicit DevData(int dev) : device(dev) {}
    ~DevData() {
        if (allocs.empty()) return;
        (void)hipSetDevice(device);
        for (void *p : allocs) (void)hipFree(p);
    }
};

// What a model of three channels holds of the two other objects (y and z, or 2 and 3): their policies' descriptors, with the
// device data kept alive.  The model's own members sit on top (PosAtt, Position, AttSimplified in rollout_channels.hip).
struct Attached {
    DPaChan c[2]{};
    std::shared_ptr<DevData> data[2];
    int n_planes = 0;               // of the three channels, the fewest
    virtual ~Attached() = default;
};

struct Rollout {
    std::mutex mu;                  // one call at a time per object
    int device = 0, D = 0, idx_bytes = 4, n_planes = 0;
    int model = kModelNone, integrator = HJB_ATT_TAYLOR;
    int64_t chunk = (int64_t)1 << 20;
    bool lds = true;                // option "lds": stage the tables in LDS when they fit (false: never)
    DRollout R{};                   // device pointers filled by create; model by set_model
    double grid_lo[HJB_MAX_D] = {}, grid_hi[HJB_MAX_D] = {};   // the first and the last knot of every axis (create): the campaign's extent
    DAttitude M{};                  // the attitude model (set_attitude_model)
    std::unique_ptr<Attached> att;  // the PosAtt / Position / AttSimplified of model kModelPosAtt / kModelPosition / kModelAttSimplified
    std::shared_ptr<DevData> data;
    // the noise node set (hjb_rollout_set_noise): N.n_nodes > 0 while one is set; read by hjb_rollout_run_noisy, _run_campaign,
    // _run_lookahead (fly_noise) and _run_lookahead_campaign
    DNoise N{};
    std::shared_ptr<DevData> noise;     // N.tab: thresholds, then the masked axes' offsets
    // the actuator node set (hjb_rollout_set_actuator_noise): Act.n_nodes > 0 while one is set; read by hjb_rollout_run_actuator and
    // _run_actuator_campaign alone
    hjb::DActuator Act{};
    std::shared_ptr<DevData> actuator;  // Act.tab: thresholds, then the live inputs' eps rows, then the base axes' rows
    // the value planes (hjb_rollout_set_values): val_planes > 0 while some are set; read by hjb_rollout_run_greedy, _run_lookahead and
    // _run_lookahead_campaign
    std::shared_ptr<DevData> values;
    const void *dvalues = nullptr;      // [nS, val_planes] column-major, float or double
    int val_planes = 0, val_bytes = 8;
    // the lookahead node set (hjb_rollout_set_lookahead): L.n_nodes > 0 while one is set; read by hjb_rollout_run_lookahead and
    // _run_lookahead_campaign
    hjb::LookSet L{};
    std::shared_ptr<DevData> look;      // L.tab: the weights, then the masked axes' offsets
    // the per-control lookahead node set (hjb_rollout_set_control_lookahead): CL.n_nodes > 0 while one is set; read by
    // hjb_rollout_run_control_lookahead and _run_control_lookahead_campaign alone
    hjb::CtrlLookSet CL{};
    std::shared_ptr<DevData> ctrl_look; // CL.tab: the weights, then every label's masked axes' offsets
    hipStream_t stream = nullptr;
    std::string err;
};

constexpr int64_t kMaxChunk = (int64_t)1 << 30;
constexpr size_t kLdsMax = 32 << 10;        // knots + 1/dx + u_table staged in LDS up to this size

int rfail(Rollout *ro, int code, const char *fmt, ...);

bool all_finite(const double *p, int64_t n);      // a null p is finite

// The argument checks every run function of an object makes before any device work: method, sizes, that the object holds the
// model this entry point runs (`want`), plane_of_step against the planes all of the model's channels have.
int check_run(Rollout *ro, int want, int method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj);

// The checks on the trajectories every run function makes next (pre: "rollout", or the entry point's name where there is no
// object): null X0 / X_final, the sizes of W doubles per trajectory and stage (wname: how the message spells W), a finite X0.
int check_traj(Rollout *ro, const char *pre, int W, const char *wname, int32_t n_steps, int64_t n_traj, const double *X0,
               const double *X_final);

// What hjb_rollout_run_lookahead and hjb_rollout_run_lookahead_campaign refuse of the object and the value planes, in `who`'s name
// (n_traj: the trajectories or the starts): negative sizes, no or another model, no lookahead set, fly_noise without a noise set,
// value_plane_of_step against the planes of hjb_rollout_set_values (-1 needs none).  Under ro->mu.  own_set false: the caller
// brings the lookahead set (HJB_PAIR_GREEDY's one zero node), the object need not hold one.
int check_lookahead_run(Rollout *ro, const char *who, int fly_noise, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_traj,
                        bool own_set = true);

// What hjb_rollout_set_noise, hjb_rollout_noise_table and hjb_rollout_lookahead_campaign_host refuse of a weight vector (null: equal
// weights), in `who`'s name: a weight that is not finite or is negative, weights that sum to 0.
int check_weights(Rollout *ro, const char *who, int32_t n_nodes, const double *weights);

// The affine problem of the host twins (hjb_rollout_greedy_host, hjb_rollout_lookahead_host, hjb_rollout_lookahead_campaign_host)
// as their common arguments give it, and the records the twins' loops read of it.  The refusals are in `who`'s name and in two
// parts: *_host_args, everything up to the sizes (n_traj: the trajectories or the starts), and *_host_model, the grid, the
// tables, the model and the planes of the steps, which also fills the records.  look_host_* put the lookahead node set on top of
// the affine part: its refusals end look_host_args, its table (L.tab points into tab) ends look_host_model.
struct AffineHostArgs {
    int32_t D;
    const int32_t *n;
    const double *knots;
    int32_t n_labels, n_u;
    const double *u_table, *A, *B, *c, *q, *r;
    int32_t dtype, n_value_planes;
    const void *values;
    int32_t n_steps;
    const int32_t *value_plane_of_step;
};
struct AffineHostProblem {
    hjb::GreedyModel M{};
    std::vector<double> rdx;
};
struct LookHostProblem : AffineHostProblem {
    hjb::LookSet L{};
    std::vector<double> tab;
};
int affine_host_args(const char *who, const AffineHostArgs &a, int64_t n_traj);
int affine_host_model(const char *who, const AffineHostArgs &a, AffineHostProblem &P);
int look_host_args(const char *who, const AffineHostArgs &a, int64_t n_traj, int32_t mode, int32_t n_nodes, const double *offsets,
                   const double *weights);
int look_host_model(const char *who, const AffineHostArgs &a, int32_t mode, int32_t n_nodes, const double *offsets, const double *weights,
                    LookHostProblem &P);

// What hjb_rollout_run_noisy, hjb_rollout_run_lookahead (fly_noise) and hjb_rollout_noise_draw refuse of their streams, in `who`'s
// name: first_stream < 0, first_stream + n_traj overflowing
int check_streams(Rollout *ro, const char *who, int64_t n_traj, int64_t first_stream);

// The noisy LDS rule (hjb_rollout_run_noisy, hjb_rollout_run_lookahead with fly_noise, the campaigns): the object's tables
// [knots | 1/dx | u_table] and the node block of its noise set together, staged (*on) when option "lds" is on and they fit kLdsMax.
// -> the bytes
size_t noisy_lds(const Rollout *ro, bool *on);
// ... and the same rule for the actuator flights (hjb_rollout_run_actuator, _run_actuator_campaign): the tables and the node block of
// the actuator set together
size_t actuator_lds(const Rollout *ro, bool *on);

// What hjb_rollout_set_lookahead, hjb_rollout_set_control_lookahead and the lookaheads' host twins refuse of a lookahead node set,
// hjb_set_disturbance's refusals, in `who`'s name: the mode, n_nodes outside 0..HJB_DIST_MAX_NODES, null offsets, weights with
// HJB_DIST_WORST, a weight that is not finite or is negative, and of offsets [D, n_nodes] an entry that is not finite (D < 1: the
// offsets are left to the caller, who knows their shape)
int check_lookahead(Rollout *ro, const char *who, int D, int32_t mode, int32_t n_nodes, const double *offsets, const double *weights);

// The shared tail of the setters that give an object a table (noise, values, both lookahead sets), under ro->mu: `bytes` at src
// go to the object's device in a DevData of their own (any false: no table, the set is detached), and once the object's stream is
// idle `holder` takes it, which releases a table given earlier.  -> *dev, the table on the device (null for none).  `big`: how the
// HJB_E_NOMEM refusal calls a table large enough to be checked against the free memory first (null: none is).
int attach_table(Rollout *ro, const char *who, const void *src, size_t bytes, bool any, std::shared_ptr<DevData> &holder, const void **dev,
                 const char *big = nullptr);

// What the campaigns (hjb_rollout_run_campaign, hjb_rollout_run_lookahead_campaign, their host forms) refuse of their sizes, in
// `who`'s name: n_samples < 1, n_starts * n_samples overflowing; and of their bounds: a NaN threshold, a NaN or negative tol
// (n_starts >= 0 and D are the caller's).  Defined in rollout_campaign_host.hip.
int check_campaign_sizes(Rollout *ro, const char *who, int64_t n_starts, int64_t n_samples);
int check_campaign_bounds(Rollout *ro, const char *who, int D, int64_t n_starts, const double *threshold, const double *tol);
// ... and, with the sizes first, of their streams: first_stream < 0, first_stream + n_starts * n_samples overflowing
int check_campaign_streams(Rollout *ro, const char *who, int64_t n_starts, int64_t n_samples, int64_t first_stream);

// The launches of a campaign call, as run_campaign_launches hands them to the call's launch function - built once per call, only
// C[r].block0 and C[r].n_blocks move from launch to launch: the object's record with each plane list on the device (R[1] is the
// pair's second), the noise set with the call's seed and first stream, one DCampaign per record - one geometry, each its own
// partials - the LDS bytes and the placement of noisy_lds, X0 [D, n_starts]
// and every record's stats [8, n_starts] on the device.  In a histogram call (K30) lds is the launch's dynamic LDS bytes and
// lds_on the tables' placement as campaign_hist_form decided them, and H the histogram's record; H.hist is null otherwise.  In a
// pair call (K31) pair_cost [lanes] doubles and pair_left [lanes] bytes are the pair scratch, lanes = nb_max * G of a launch and
// never n_starts * M, and Lg HJB_PAIR_GREEDY's set (one zero node of weight 1; Lg.tab null unless a side is greedy).  In an actuator
// call (K34, CampaignPlan::actuator) Na is the actuator set with the call's seed and first stream and lds / lds_on are
// actuator_lds'; N is then not read.
struct CampaignLaunch {
    hjb::DRollout R[2];
    hjb::DNoise N;
    hjb::DActuator Na;
    hjb::DCampaign C[3];
    size_t lds;
    bool lds_on;
    hipStream_t st;
    const double *X0;
    double *stats[3];
    hjb::DCampHist H;
    double *pair_cost;
    uint8_t *pair_left;
    hjb::LookSet Lg;
};

// The histogram of a campaign call (K30), on the host: lo, hi [n_starts], n_bins and the output hist [n_bins + 2, n_starts]
struct CampaignHistCall {
    const double *lo, *hi;
    int32_t n_bins;
    int64_t *hist;
};
// What the histogram entry points refuse of it, in `who`'s name (n_starts >= 0 the caller's): n_bins outside 1 ..
// HJB_CAMPAIGN_MAX_BINS; with n_starts > 0 a null lo, hi or hist, a lo or hi that is not finite, !(lo < hi), a scale that is not finite
int check_campaign_hist(Rollout *ro, const char *who, int64_t n_starts, const CampaignHistCall &h);

// What the five campaign run functions have in common of their arguments (hjb_rollout_run_campaign, _run_campaign_hist,
// _run_lookahead_campaign, _run_lookahead_campaign_hist, _run_campaign_pair)
struct CampaignCall {
    const char *who;                // the entry point, for the error texts
    int32_t n_steps;
    int64_t n_starts, n_samples;
    const double *X0;
    uint64_t seed;
    int64_t first_stream;
    const double *threshold, *tol;
    double *device_ms;              // optional: the sum of the launches' event times
};

// What a campaign call holds on the device beside X0 and the thresholds: its records with their host outputs (1; the pair's 3:
// A, B and d), its lists of the steps' planes (1; the pair's 2), the histogram or none, the pair scratch and HJB_PAIR_GREEDY's
// one-node lookahead table
struct CampaignPlan {
    int n_records = 1;
    double *stats[3] = {};          // [8, n_starts] each, on the host
    int n_plane_lists = 1;
    const int32_t *planes[2] = {};  // [n_steps] each, on the host
    const CampaignHistCall *hist = nullptr;
    bool pair_scratch = false, greedy = false;
    bool actuator = false;          // K34: the plant is the actuator set (CampaignLaunch::Na)
};

// The device side of a campaign call whose arguments have been checked (n_starts >= 1; rollout_campaign_host.hip), the one loop of
// all five run functions: X0, the thresholds and the plan's plane lists uploaded once, the call's block list walked in launches
// of at most option "chunk" lanes (campaign_geometry, hjbdp_campaign.h, whose byte count is the HJB_E_NOMEM bound) - `launch`
// starts everything that runs between a launch's two events on c.st, and the loop synchronises once per launch - and the plan's
// records downloaded.  With plan.hist (K30) the call also holds [3, n_starts] doubles (lo, hi, scale) and hist
// [n_bins + 2, n_starts] int64, zeroed once on the call's stream before the first launch and downloaded after the last.  Under
// ro->mu.
int run_campaign_launches(Rollout *ro, const CampaignCall &call, const CampaignPlan &plan,
                          const std::function<hipError_t(const CampaignLaunch &)> &launch);

// The frame of the five run functions: every refusal before any device work and in one order, the outputs untouched -
// check_campaign_streams, `no_object` (what the call refuses before it needs an object; may be empty), the null handle, the
// object's lock, `controller` (check_run and the noise set, or check_lookahead_run, or one of these per side; under the lock),
// n_starts == 0 (HJB_OK, *device_ms = 0), null stats, check_traj, check_campaign_bounds, check_campaign_hist - then
// run_campaign_launches.
int run_campaign_call(void *rollout, const CampaignCall &call, const CampaignPlan &plan, const std::function<int(Rollout *)> &no_object,
                      const std::function<int(Rollout *)> &controller, const std::function<hipError_t(const CampaignLaunch &)> &launch);

// K17 and K21 renormalise the quaternion X0[3..6] of a 7-state column after the first step: all zeros would be 0/0
int check_quaternions(Rollout *ro, const char *pre, int64_t n_traj, const double *X0);

// The attitude loops' constants from the principal inertias: h, J and the Euler coefficients (q and r zero)
DAttitude euler_attitude(double J1, double J2, double J3, double h);

// `bytes` at src on the device (the current one), owned by dd: at least 16 bytes are allocated, nothing is copied for none
int upload(Rollout *ro, DevData &dd, const void *src, size_t bytes, const void **out);

// The chunk loop the run functions share.  A run function fills a ChunkPlan - the RunCall, what its frame reads, and the outputs
// on top; run_chunks calls its launch once per chunk of at most Rollout::chunk trajectories with that chunk's device buffers.
constexpr int kMaxPaths = 5, kMaxInputs = 3;

struct RunCall {
    const char *who;                // the entry point, for the error text
    int W;                          // doubles of state per trajectory
    const char *wname;              // how a message spells W
    int32_t n_steps;
    const int32_t *plane_of_step;   // null for a loop without a policy (hjb_attitude_linear_response): nothing is uploaded then
    int64_t n_traj;
    const double *X0;
    double *X_final;
    double *device_ms;              // optional: the sum of the launches' event times
};

struct ChunkPlan : RunCall {
    // per-step outputs, [n_traj, rows * stages] on the host; a null host pointer is an output not asked for
    struct Path { double *host; int rows, stages; } path[kMaxPaths] = {};
    double *cost = nullptr;         // [n_traj], optional
    int32_t *flags = nullptr;       // [n_traj], optional (the position loop's off_schedule, the fault campaigns' settle_stage)
    const int32_t *input[kMaxInputs] = {};      // per-trajectory inputs, [n_traj] each; a null entry is skipped
};

struct Chunk {
    DRollout R;                     // the object's, with plane_of_step (on the device) and n_steps set
    int64_t nc, i0;                 // trajectories i0 .. i0 + nc of the call
    size_t lds;                     // bytes of R's [knots | 1/dx | u_table]
    bool lds_on;                    // option "lds" and lds <= kLdsMax
    hipStream_t st;
    const double *X0;
    double *Xf, *cost;              // cost, flags, path[p], input[t]: null where the plan has none
    int32_t *flags;
    double *path[kMaxPaths];        // [nc, rows * stages], trajectory index fastest
    const int32_t *input[kMaxInputs];
};

// Per chunk: X0 and the inputs uploaded (at the chunk's offset), launch(chunk) between two events, X_final / cost / flags and the
// paths downloaded (columns i0 .. i0 + nc of the host's [n_traj, rows * stages]).  Holds g_capture_mu shared for the whole call.
int run_chunks(Rollout *ro, const ChunkPlan &plan, const std::function<hipError_t(const Chunk &)> &launch);

// The frame of the nine run functions of an object: `no_object` (what the call refuses before it needs an object; may be empty),
// the null handle, the object's lock, `controller` (everything under the lock up to the empty call: check_run or
// check_lookahead_run, the noise set, the stages a model's table covers, the fault planes, the tolerances), n_traj == 0 (HJB_OK,
// *device_ms = 0), check_traj, `starts` (what is refused per trajectory; may be empty), *device_ms = 0, run_chunks with `launch`.
// A plan is made before the lock: of the object it may read what hjb_rollout_create fixed (D, n_u), and of a null handle nothing.
int run_call(void *rollout, const ChunkPlan &plan, const std::function<int(Rollout *)> &no_object, const std::function<int(Rollout *)> &controller,
             const std::function<int(Rollout *)> &starts, const std::function<hipError_t(const Chunk &)> &launch);

// The plan every run function of the affine model starts from: D doubles of state, X_path and U_path, the cost (of a null handle,
// which run_call refuses, nothing is read); and the greedy part of a chunk's launch record (hjb_rollout_run_greedy, _run_lookahead,
// _run_control_lookahead): paths 0 .. 3 are X, U, L, V
ChunkPlan affine_plan(const Rollout *ro, const char *who, int32_t n_steps, const int32_t *planes, int64_t n_traj, const double *X0,
                      double *X_final, double *cost, double *X_path, double *U_path, double *device_ms);
hjb::DGreedy greedy_of_chunk(const Rollout *ro, const Chunk &c);

}  // namespace hjbhost
