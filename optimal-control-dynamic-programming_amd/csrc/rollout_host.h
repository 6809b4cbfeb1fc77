// rollout_host.h - what the host units of the rollouts share (host only; include/hjbdp.h is the public ABI): the object,
// its refusals, the upload and the chunk loop.  Defined in rollout.hip; rollout_channels.hip and rollout_campaign_host.hip are the
// other readers.
#pragma once
#include "hjbdp_host.h"
// the records an object holds: DRollout, DAttitude, DNoise, DPaChan (a unit includes the other kernel headers whose launch it calls)
#include "kernels_rollout.h"
#include "kernels_rollout_attitude.h"
#include "kernels_rollout_noisy.h"
#include "kernels_rollout_pos_att.h"
#include "hjbdp_lookahead.h"
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
    // the noise node set (hjb_rollout_set_noise): N.n_nodes > 0 while one is set; read by hjb_rollout_run_noisy alone
    DNoise N{};
    std::shared_ptr<DevData> noise;     // N.tab: thresholds, then the masked axes' offsets
    // the value planes (hjb_rollout_set_values): val_planes > 0 while some are set; read by hjb_rollout_run_greedy alone
    std::shared_ptr<DevData> values;
    const void *dvalues = nullptr;      // [nS, val_planes] column-major, float or double
    int val_planes = 0, val_bytes = 8;
    // the lookahead node set (hjb_rollout_set_lookahead): L.n_nodes > 0 while one is set; read by hjb_rollout_run_lookahead alone
    hjb::LookSet L{};
    std::shared_ptr<DevData> look;      // L.tab: the weights, then the masked axes' offsets
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

// K17 and K21 renormalise the quaternion X0[3..6] of a 7-state column after the first step: all zeros would be 0/0
int check_quaternions(Rollout *ro, const char *pre, int64_t n_traj, const double *X0);

// The attitude loops' constants from the principal inertias: h, J and the Euler coefficients (q and r zero)
DAttitude euler_attitude(double J1, double J2, double J3, double h);

// `bytes` at src on the device (the current one), owned by dd: at least 16 bytes are allocated, nothing is copied for none
int upload(Rollout *ro, DevData &dd, const void *src, size_t bytes, const void **out);

// The chunk loop the run functions share.  A run function fills a ChunkPlan; run_chunks calls its launch once per chunk of at
// most Rollout::chunk trajectories with that chunk's device buffers.
constexpr int kMaxPaths = 5, kMaxInputs = 3;

struct ChunkPlan {
    const char *who;                // the entry point, for the error text
    int W;                          // doubles of state per trajectory
    int32_t n_steps;
    const int32_t *plane_of_step;   // null for a loop without a policy (hjb_attitude_linear_response): nothing is uploaded then
    int64_t n_traj;
    const double *X0;
    double *X_final;
    // per-step outputs, [n_traj, rows * stages] on the host; a null host pointer is an output not asked for
    struct Path { double *host; int rows, stages; } path[kMaxPaths] = {};
    double *cost = nullptr;         // [n_traj], optional
    double *device_ms = nullptr;    // optional: the sum of the launches' event times
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

}  // namespace hjbhost
