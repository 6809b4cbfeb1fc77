// hjbdp_host.h - what the host-side translation units of libhjbdp share (internal; include/hjbdp.h is the public ABI):
// the handle, error reporting, the process-wide locks and switches, and the entry points one unit offers the others.
//   hjbdp_setup.hip    process-wide state, device allocation, the problem upload, hjb_create's work as a list of steps, work buffers, probe
//   hjbdp_tables.hip   the (cell, weight) tables: domains, builds, rebuild, hash; eligibility of variants 5 / 6; K9's examination and launch
//   hjbdp_packed.hip   variant 1's analysis, variants 2 / 4 (outer terms, axis tables, contraction mode), the DNested upload, K15's set-up
//   hjbdp_colsweep.hip variant 7's host side: plan, XCD map, DPP test, cooperative plan, launch record, split rule
//   hjbdp_choose.hip   which variant serves, in which form and geometry (Handle::L), and the stage launch
//   hjbdp_api.hip      hjb_create .. hjb_backup_stage, options, probe, policy lookup (the single-device C ABI)
//   hjbdp_solve.hip    hjb_solve (one handle's backward sweep; hjbdp_sweep.h: the monitor rule, its schedule, the graph split)
//   hjbdp_evaluate.hip hjb_evaluate_stage, hjb_evaluate_stage_device, hjb_evaluate (the cost of a given policy on the grid)
//   hjbdp_disturb.hip  hjb_set_disturbance, hjb_set_control_disturbance (the disturbance a handle's stages carry: kernel variant 8)
//   hjbdp_batch.hip    hjb_solve_batch (several sweeps of one kernel shape, one launch per stage)
//   hjbdp_builder.hip  the flat builder API (MATLAB loadlibrary / calllib)
//   hjbdp_slab.hip     one device's slab of a partitioned grid: its handles, strip streams, and the enqueue of one stage (hjbdp_slab.h: the arithmetic)
//   hjbdp_multi.hip    hjb_create_multi / hjb_solve_multi (one process, several GPUs): the slabs, the halo copies, the stage loop
//   hjbdp_rank.hip     hjb_rank_* (one process per GPU: one slab) and the RCCL transport inside the library
//   hjbdp_devmem.hip   device-buffer helpers
//   rollout.hip, rollout_channels.hip (rollout_host.h)   hjb_rollout_*: closed-loop rollouts of stored policies (error reporting and locks only)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/hjbdp.h"
#include "hjbdp_dev.h"
#include "hjbdp_launch.h"
#include "hjbdp_slab.h"
#include "hjbdp_sweep.h"
#include "kernels_generic.h"
#include "kernels_nested.h"
#include "kernels_packed.h"
#include "kernels_packed2.h"
#include "kernels_uniwin.h"
#include "kernels_ctrlsplit.h"
#include "kernels_tabled.h"
#include "kernels_rowwise.h"
#include "kernels_tile2d.h"
#include "kernels_colsweep.h"
#include "kernels_colcoop.h"
#include "kernels_reduce.h"
#include "kernels_probe.h"

namespace hjbhost {
using namespace hjb;

// K15's claim counters: one set per stream a handle launches on (the first kUwSets streams; later ones take the static walk)
constexpr int kUwSets = 8;
constexpr int kUwSetWords = 8 * 16;  // one set: per XCD one 64-byte line

extern thread_local std::string g_last_error;
// fault injection for the tests, by explicit call only (hjb_test_hook; the environment never changes what the library does)
extern std::atomic<int> g_test_fail_tab64_scratch;   // "fail_tab64_scratch": the float64 table build's scratch allocation fails
extern std::atomic<int> g_test_fail_tabled_alloc;    // "fail_tabled_alloc": the (cell, t) table allocation fails
extern std::atomic<int> g_test_rccl_only_env;        // "rccl_only_env": the RCCL loader tries $HJBDP_RCCL_LIB only
extern std::atomic<int> g_test_fail_graph_capture;   // "fail_graph_capture": capture_stage_loop fails before any HIP call
// Handles may be driven from different host threads (one thread per handle).  HIP stream capture is fragile
// against "unsafe" calls made elsewhere in the process while it records (device-wide synchronisation, synchronous
// copies, allocation): a capture takes this lock exclusively, every such call takes it shared.  Kernel launches,
// graph launches and waits on a handle's own stream need no lock and overlap freely.
extern std::shared_mutex g_capture_mu;

// The launch of one stage: which kernel variant, in which form, with which geometry.  choose_launch alone fills it (launch_changed
// derives what depends on the final grid); launch_stage dispatches on it, hjb_get_info and hjb_solve_batch read it.
struct Launch {
    int variant = 0;
    int status = HJB_OK;          // variant_status of `variant`: not HJB_OK only for a float64-typed handle whose tables failed (refused)
    int grid = 1, block = 256;
    size_t lds = 0;               // dynamic LDS per workgroup
    int mode = 0;                 // variant 4: K3's contraction mode (kernels_packed2.h MODE), 7 / 8: K15 (kernels_uniwin.h)
    bool idx32 = false;           // variant 5: the 32-bit form of the table kernel (needs grid * block <= kTab32MaxThreads)
    bool lean = false;            // variant 6: the lean form (kernels_rowwise.h)
    bool j_in_lds = false;        // variant 3: the whole J buffer staged in LDS
    bool fast = false;            // variant 1: the fast inner term
    int cost_form = 0;            // variant 7: 0 general, 1 the usual shape (state terms + one control term), 2 that in float64
    bool dpp = false;             // variant 7: the one-load form
    int coop_grid = 0;            // variant 7: the cooperative form's grid (0: it does not apply); it runs where J is 16-byte aligned
};

struct Handle {
    hjb_problem prob{};  // scalar fields only (pointers are not kept)
    int device = 0;
    int dtype = HJB_F32;
    size_t esz = 4;
    int64_t n_owned = 0, nU = 0, j_elems = 0, inner = 0;
    int nplanes = 0, plane0 = 0;
    DParams hp{};                 // host copy of the device params
    DParams *dp = nullptr;        // device params
    std::vector<void *> allocs;   // every device allocation (freed in destroy): large ones and the chunks the small ones are carved from
    char *arena = nullptr;        // dev_alloc: the current chunk's free part
    size_t arena_left = 0;
    int32_t *d_status = nullptr;  // two device words: [0] a query left the slab (DParams::status), [1] the evaluation kernel met a label out of range
    // work buffers (lazy)
    void *dJ[2] = {nullptr, nullptr};
    char *d_idx = nullptr;        // argmin labels of the owned states, idx_bytes each
    int idx_bytes = 4;            // hjb_problem.idx_dtype resolved: 4 (int32), 1 (uint8) or 2 (uint16)
    bool tab64 = false;           // hjb_problem.table_dtype == HJB_TAB_F64: (cell, t) tables built in float64 from float64 terms
    bool cost64 = false;          // hjb_problem.cost_dtype == HJB_COST_F64: cost terms float64, summed in double, one rounding per backup
    DParams *dp64 = nullptr;      // ... the float64 shadow of the axes (knots, 1/dx, next-state terms) the table build reads
    double *d_partials = nullptr;  // monitor reduction scratch
    double *d_sums = nullptr;      // [2]: sum J, sum idx
    DNested hn{};                 // variant 1 (control-nested) parameters
    DNested *dn = nullptr;
    bool nested_ok = false;
    bool nested_fast = false;
    int packed_mode = 0;          // variant 2 eligibility
    // launch-bound sweeps: the ping-pong stage loop captured once into a hipGraph of kGraphStages launches
    hipStream_t stream = nullptr;
    hipGraphExec_t gexec = nullptr;
    bool gexec_tiled = false;
    bool use_graph = true;
    bool monitor_single = false;  // option "monitor_single" (see hjb_solve_opts.monitor_single)
    size_t packed_lds = 0;
    size_t packed2_lds = 0;       // variant 4 (two controls per packed op)
    void *tile_plan = nullptr;    // K9 cached form: per (state, control) stage-invariant record (k_tile2d_plan)
    int tile2d = -1;              // K9 (several stages per launch, kernels_tile2d.h): -1 not examined yet, 0 no, 1 yes
    int use_temporal = 1;         // option "temporal": 0 off, 1 when applicable, 2 required (hjb_solve fails otherwise)
    bool row_ok = false;          // variant 6 (one wave per grid row) applies
    bool row_auto = false;        // ... and is chosen automatically
    bool row_lean_ok = false;     // variant 6: the lean form applies (kernels_rowwise.h)
    bool row_lean = true;         // option "row_lean"
    int packed_pre = 0;           // variant 4 contraction mode (kernels_packed2.h MODE): 0 plain, 1 C2 shape, 2 state-only axes first
    bool window3_ok = false;      // modes 2 / 3 qualify for the three-plane window (modes 5 / 6); option "window_planes" switches
    size_t lds_pad = 0;           // extra dynamic LDS per workgroup (occupancy tuning)
    // K15 (kernels_uniwin.h, variant 4 modes 7 / 8): the window kernel for chunks that share their rate axes
    bool uniwin_ok = false;       // the structure holds and the per-point plan is built
    bool uniwin_auto = false;     // ... and few enough points leave the usual shape for it to be the automatic choice
    int uniwin_on = -1;           // option "uniwin": -1 automatic, 0 never, 1 whenever uniwin_ok
    int uniwin_slow = 0;          // points of the plan that take the slow path
    int uw_tile = 0;              // option "uw_tile": log2 tile extents lA + 8 * lB + 64 * lC (0: the default 3, 2, 2)
    int uw_claim = 1;             // option "uw_claim": 1 = the chunk walk's positions are claimed from per-XCD counters, 0 = fixed stride
    int uw_block = 256;           // option "uw_block": states per chunk = threads per workgroup (256 or 64)
    size_t uw_lds = 0;
    DUniwin huw{};                // huw.counters: the first of kUwSets counter sets (8 x one 64-byte line each)
    DUniwin *duw = nullptr;       // kUwSets + 1 device copies of huw: copy k claims from counter set k, the last one walks statically
    hipStream_t uw_streams[kUwSets] = {};    // the stream each counter set serves (launches on one stream are ordered)
    int uw_nstreams = 0;
    bool tabled_ok = false;       // variant 5: per-axis (cell, t) tables for every axis (built on first use)
    bool tabled_i32 = false;      // ... and every index of it fits 31 bits: the 32-bit form of the kernel runs (kernels_tabled.h)
    bool tabled_i32_on = true;    // option "tabled_i32" (0: the 64-bit form anyway - A/B timing, tests)
    uint32_t dom_mask[HJB_MAX_D] = {0};
    int64_t dom_entries[HJB_MAX_D] = {0};
    DTabled htb{};
    DTabled *dtb = nullptr;
    size_t nested_lds = 0;
    // every stage-invariant (cell, weight) table of this handle: rebuilt by option "prep_mfma" (timing / equality tests)
    struct PrepRec { int axis; int kind; const int32_t *dsz_d; std::vector<int32_t> dsz; int64_t n; void *tab; };
    std::vector<PrepRec> preps;
    bool inline_axis0 = true;     // allow mode 1's axis 0 without a table (see build)
    bool axis0_inline = false;    // ... in effect: N.at[0].tab is null
    uint32_t axis0_dom = 0;       // its broadcast domain and entry count, should the table be wanted after all
    int64_t axis0_nent = 0;
    int prep_mfma = 0;            // 1: tables were built with v_mfma_f32_32x32x2_f32 where the axis' terms allow it
    int prep_mfma_axes = 0;       // ... number of tables the MFMA form applied to in the last rebuild
    double prep_us = 0;           // device time of the last rebuild of all tables
    int cs_state = -1;            // variant 7 (column sweep, kernels_colsweep.h): -1 not examined, 0 does not apply, 1 plan built
    DColSweep hcs{};
    DColSweep *dcs = nullptr;
    int cs_xcd_mod = 0;           // option "cs_xcd_mod": 0 = automatic (see colsweep_map)
    int cs_dpp = 1;               // option "cs_dpp": allow the DPP form of variant 7 when the axis-0 cells permit it
    int cs_rows_mid = 0;          // corner rows per step the mid-grid column needs (get_option "cs_rows")
    int cs_xcd_axis = 0;          // option "cs_xcd_axis": 0 = the XCDs split the group axis, 1 = the window axis
    int cs_split = 0;             // option "cs_split": parts a column is swept in (0 = automatic, see colsweep_split)
    int cs_coop = 0;              // option "cs_coop": allow the cooperative form (kernels_colcoop.h) where it applies
    std::vector<double> cs_cu64;  // cost_dtype F64: the control term of the cost in float64, per control (plan building)
    int cs_coop_why = 0;          // why it does not: 1 groups, 2 axis 1 sees the window axis, 3 n0 / storage, 4 cells, 5 window knots, 6 axis-0 knots
    int cs_coop_epl = 0;          // ... it applies: elements per staging load (0 = does not apply)
    bool cs_dpp_ok = false;       // the axis-0 cells permit the DPP form (colsweep_dpp_ok)
    int forced_variant = -1;      // option "variant"
    // the fixed-label stage (kernels_evaluate.h, hjb_evaluate*)
    int eval_tables = -1;         // option "eval_tables": -1 the (cell, t) tables where the handle can hold them, 0 terms summed on the fly, 1 tables
    bool eval_i32 = true;         // option "eval_i32": 0 = the 64-bit form of the evaluation kernel whatever the sizes (A/B timing, tests)
    bool eval_m24 = true;         // option "eval_m24": 0 = the 32-bit form with 32-bit index products whatever the sizes (A/B timing, tests)
    int eval_grid = 0;            // option "eval_grid": workgroups per launch of the grid-stride evaluation kernel (0 = one per 256 states)
    // the disturbance (hjb_set_disturbance; kernels_disturb.h, variant 8): dist_nodes > 0 while one is set
    int dist_nodes = 0;
    int dist_mode = HJB_DIST_EXPECT;
    uint32_t dist_axes = 0;       // bit a: some node offsets axis a (option "dist_axes")
    bool dist_i32 = true;         // option "dist_i32": 0 = the 64-bit form of the kernel whatever the sizes (A/B timing, tests)
    void *d_dist = nullptr;       // the DDisturb block on the device (allocated by the first call, rewritten by later ones)
    // ... per control (hjb_set_control_disturbance; kernels_ctrldist.h): the nodes' offsets come from a table behind the block
    bool dist_ctrl = false;       // option "dist_ctrl" (read-only): the disturbance in effect is the per-control one
    void *d_dist_tab = nullptr;   // [nU in visiting order][n_nodes][D] in the query type: rewritten in place, reallocated when it grows
    size_t dist_tab_bytes = 0;    // its capacity
    Launch L;
    int halo_need_lo = 0, halo_need_hi = 0;
    std::string err;
};

int fail(Handle *h, int code, const char *fmt, ...);

// Work of hjb_create / hjb_solve's set-up (table builds, plans, memsets) is issued on the NULL stream; a handle's sweep runs on its own
// non-blocking stream.  Waiting for the set-up is a wait on the null stream - NOT hipDeviceSynchronize, which also waits for every other
// handle's sweep in flight (independent channels solved side by side from several host threads, hjbdp.core.solve_many, ran one after
// the other for it).
inline hipError_t sync_setup() { return hipStreamSynchronize(nullptr); }

#define HIP_TRY(h, expr)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(h, HJB_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                   \
    } while (0)

int dev_alloc(Handle *h, size_t bytes, void **out);
template <typename X>           // ... into a typed pointer (assigned on success only)
int dev_alloc(Handle *h, size_t bytes, X **out) {
    void *d = nullptr;
    const int st = dev_alloc(h, bytes, &d);
    if (!st) *out = (X *)d;
    return st;
}
template <typename T, typename X>
int upload(Handle *h, const std::vector<T> &v, X **out) {
    void *d = nullptr;
    const int ast = dev_alloc(h, std::max<size_t>(v.size(), 1) * sizeof(T), &d);
    if (ast) return ast;
    if (!v.empty()) HIP_TRY(h, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (X *)d;
    return HJB_OK;
}

// What one call of a sweep driver holds on the device beside the handle's own buffers: its scratch buffers, its two timing events
// and, where used, a graph exec.  Declared AFTER the caller's shared hold of g_capture_mu: the destructor frees everything under
// that hold (hipFree is one of the calls a stream capture elsewhere in the process must not see), or under one of its own while
// the caller's is released.
using SharedHold = std::shared_lock<std::shared_mutex>;
struct HoldUnlessHeld {                  // a shared hold for a scope, unless the caller's `held` owns one (no second one on a thread)
    SharedHold own{g_capture_mu, std::defer_lock};
    explicit HoldUnlessHeld(const SharedHold &held) { if (!held.owns_lock()) own.lock(); }
};
struct SweepScratch {
    Handle *h;
    const SharedHold &held;
    std::vector<void *> bufs;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipGraphExec_t gexec = nullptr;
    SweepScratch(Handle *h_, const SharedHold &held_) : h(h_), held(held_) {}
    SweepScratch(const SweepScratch &) = delete;
    ~SweepScratch();
    void drop_graph();                   // gexec destroyed, under the same rule
    // a buffer of this call (zero: filled with zeros) -> HJB_E_NOMEM with the caller's message, HJB_E_DEVICE if the fill failed
    template <typename X, typename... A>
    int alloc(size_t bytes, bool zero, X **out, const char *fmt, A... a) {
        void *d = nullptr;
        if (hipMalloc(&d, bytes) != hipSuccess) return fail(h, HJB_E_NOMEM, fmt, a...);
        bufs.push_back(d);
        *out = (X *)d;
        if (zero) HIP_TRY(h, hipMemset(d, 0, bytes));
        return HJB_OK;
    }
};
// kGraphStages ping-pong launches recorded on `stream` into a graph exec: takes g_capture_mu exclusively (the caller holds it in no
// form), begins the capture, runs body() - the launches, -> a status -, always ends the capture, instantiates into *out.  Frees
// nothing of the caller's and has released the lock when it returns; on failure *out is untouched and the error recorded.
int capture_stage_loop(Handle *h, hipStream_t stream, const std::function<int()> &body, hipGraphExec_t *out);

// hjbdp_setup.hip
int64_t term_elems(const hjb_problem *p, uint32_t mask);
inline int first_term(const hjb_term *t, int lo, int hi, uint32_t bits) {      // the first of terms [lo, hi) that depends on a dim of `bits`
    int k = lo;                                                                 // (none: max(lo, hi))
    while (k < hi && !(t[k].mask & bits)) ++k;
    return k;
}
int build_handle(Handle *h, const hjb_problem *p);       // upload + analysis of a validated problem (float32 / float64 arithmetic by p->dtype)
void halo_of_problem(const hjb_problem *p, bool tab64, int *lo, int *hi);     // the halo the last axis' terms imply
int ensure_work(Handle *h);
int check_status(Handle *h, hipStream_t st);
int make_probe(Handle *h, const hjb_probe *pb, DProbe *out);
int launch_probe(Handle *h, const DProbe &pr, const void *dJn, hipStream_t st);

// hjbdp_tables.hip
// An axis' broadcast domain: the dims (states, then controls) its next-state terms depend on, dense and column-major over the grid
// this handle sweeps.  dsz: each dim's size (1 outside the domain), stride: its entry stride (0 outside).
struct AxisDomain {
    uint32_t mask = 0;
    int64_t entries = 1;
    std::vector<int32_t> dsz;
    int32_t stride[HJB_MAX_G] = {0};
    bool has(int d) const { return (mask >> d) & 1u; }
};
uint32_t axis_mask(const hjb_problem *p, int a);              // union of the masks of axis a's next-state terms
AxisDomain axis_domain(const Handle *h, uint32_t mask);
inline int prep_grid(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 65536); }      // 256-thread blocks of a grid-stride kernel over n items
int build_axis_table(Handle *h, int a, const AxisDomain &dom, bool wait);     // variants 2 / 4: axis a's table allocated, launched, registered
int ensure_axis0_table(Handle *h);
int ensure_tabled(Handle *h);
void analyse_tabled(Handle *h, const hjb_problem *p, size_t entry_bytes);     // variants 5 / 6 eligibility (build_handle's step)
int rebuild_tables(Handle *h, bool mfma);
int table_hash(Handle *h, uint64_t *out);
int examine_tile2d(Handle *h);
int launch_tile2d(Handle *h, const void *dJn, void *dJo, void *didx, int K, hipStream_t st);

// hjbdp_packed.hip (analyse_nested .. setup_uniwin: build_handle's steps, in its order)
void analyse_nested(Handle *h, const hjb_problem *p, size_t elem_bytes);
void analyse_packed(Handle *h, const hjb_problem *p);
int build_packed_tables(Handle *h, const hjb_problem *p);
int upload_nested(Handle *h);
int setup_uniwin(Handle *h, const hjb_problem *p);
int uniwin_options(Handle *h);       // K15's tiling from the options, uploaded (the device is synchronised first)
inline bool uniwin_active(const Handle *h) {
    return h->uniwin_ok && (h->packed_pre == 5 || h->packed_pre == 6) && (h->uniwin_on == 1 || (h->uniwin_on < 0 && h->uniwin_auto));
}

// hjbdp_colsweep.hip
int ensure_colsweep(Handle *h);                // variant 7's eligibility and plan, examined once (Handle::cs_state)
int colsweep_options(Handle *h, bool remap);   // variant 7's launch-time fields from the options, uploaded (remap: the XCD map too)
bool colsweep_usual_cost(const Handle *h);     // state terms + one control term

// hjbdp_choose.hip
int variant_status(Handle *h, int v, const char **why);   // what variant v needs of the handle (builds what it reads)
void choose_launch(Handle *h);       // the variant, its form and geometry -> Handle::L
void launch_changed(Handle *h);      // after a change to Handle::L: what depends on the grid; the captured graph is dropped
int launch_stage(Handle *h, const void *dJn, void *dJo, void *didx, hipStream_t st);
// The fixed-label stage.  prepare_evaluate: whether the handle is served and from which source of cells and weights; a handle's FIRST
// evaluation builds the (cell, t) tables it reads if no stage kernel has yet - allocation and a wait on the null stream, so that
// first call must not sit inside a stream capture (include/hjbdp.h says so); later calls find them built and do no such work.
// launch_evaluate: one stage (dJn, dlabels -> dJo) on st; it calls prepare_evaluate itself.
// eval_grid_of / eval_runs_i32 / eval_runs_m24: the launch size and which index form of the kernel runs - the one statement of each.
int prepare_evaluate(Handle *h, bool *tabled);
int launch_evaluate(Handle *h, const void *dJn, const void *dlabels, void *dJo, hipStream_t st);
// one workgroup per 256 states; beyond 2^22 workgroups (2^30 states) equally long grid-stride spans; option "eval_grid" overrides
inline int64_t eval_grid_of(const Handle *h) {
    return h->eval_grid > 0 ? h->eval_grid : std::max<int64_t>(1, hjb::launch_spans((h->n_owned + 255) / 256, (int64_t)1 << 22));
}
// the 32-bit form: owned states and the haloed J below 2^31 - 2^26 (kTab32Lim) and a grid-stride step of at most 2^31, so that the
// step on top of the last index stays below 2^32; every axis table is below 2^31 entries (part of tabled_ok), every term and cost
// table below 2^31 elements (hjb_create)
inline bool eval_runs_i32(const Handle *h) {
    return h->eval_i32 && h->n_owned < kTab32Lim && h->j_elems < kTab32Lim && eval_grid_of(h) * 256 <= ((int64_t)1 << 31);
}
// variant 8's index form follows the same predicate (its strides are smaller: at most 2^20 workgroups, or eval_grid_of for labels)
inline bool dist_runs_i32(const Handle *h) { return h->dist_i32 && eval_runs_i32(h); }
// the 32-bit form with 24-bit index products (hjbdp_choose.hip): eval_runs_i32 and every factor the kernel multiplies below 2^24.
// tabled: the source of cells and weights the launch reads (prepare_evaluate) - tables and terms have strides of their own.
// eval_form: what the next launch runs from the source in effect (option "eval_form"): 0 64-bit, 1 32-bit, 2 32-bit with 24-bit products
bool eval_runs_m24(const Handle *h, bool tabled);
int eval_form(const Handle *h);
// the handle's part of a stage launch: stream, typing, parameter records, buffers (grid, block, LDS and the form are the caller's)
inline StageArgs stage_args(const Handle *h, const void *dJn, void *dJo, void *didx, hipStream_t st) {
    StageArgs a;
    a.st = st; a.dtype = h->dtype; a.D = h->hp.D;
    a.dp = h->dp; a.dn = h->dn; a.dtb = h->dtb; a.dcs = h->dcs;
    a.Jn = dJn; a.Jo = dJo; a.idx = didx;
    return a;
}

// First element of a term / table array that is not finite (-1: all finite).  The kernels' contract covers finite data only
// (DESIGN.md section 2): a NaN in a table is refused where it enters, with its place named, not found in J 2000 stages later.
int64_t first_nonfinite(const void *data, int64_t n, bool f64);
constexpr int64_t kMaxStates = (int64_t)1 << 40;     // more grid points than any device of this generation can hold one byte for

// hjbdp_api.hip: everything hjb_create checks or derives WITHOUT touching a device (the partitioners use it)
int analyse_problem(const hjb_problem *p, int *idx_bytes_out, int64_t *n_states_out, int *halo_lo, int *halo_hi);

// hjbdp_slab.hip: one device's slab of a grid partitioned along its last state axis - what hjb_solve_multi keeps per device and
// hjb_rank_* per process.  The numbers come from hjbdp_slab.h.
// What a partitioner learns of the whole problem WITHOUT a whole-grid handle or whole-grid tables (a problem whose slabs fit must
// not be refused because the whole grid would not): the halo the last axis' terms imply, and the sizes of a plane.
struct SlabGrid {
    int need_lo = 0, need_hi = 0, nl = 0, dtype = HJB_F32;
    int64_t inner = 0;            // states per plane of the last axis
    size_t esz = 4, isz = 4;      // bytes per J element / per argmin label
};
int slab_grid(const hjb_problem *p, SlabGrid *g);      // p->D is valid (the caller's check); analyse_problem's status
struct Slab {
    int device = 0, begin = 0, end = 0, hlo = 0, hhi = 0;
    SlabSplit cut{};                                   // the interior / strip arithmetic (cut.split: part[0] exists)
    Handle *whole = nullptr;                           // sees planes [begin - hlo, end + hhi)
    Handle *part[3] = {nullptr, nullptr, nullptr};     // interior, low strip, high strip over the same buffers (null: no such part)
    size_t plane_b = 0, label_plane_b = 0;             // bytes of one plane of J / of the labels
    hipStream_t ss[2] = {nullptr, nullptr};            // the two boundary strips run beside the interior
    hipEvent_t fork = nullptr, sdone[2] = {nullptr, nullptr};
    Handle *lead() const { return part[0] ? part[0] : whole; }      // the handle whose kernel choice stands for the slab's
};
// Slab k of n_slabs on `device`: the handles (slab fields set when n_slabs > 1), the strip streams and events.  split: divide it
// where hjbdp_slab.h allows.  On failure nothing is left behind and g_last_error says why.
int slab_create(Slab *S, const hjb_problem *p, const SlabGrid &g, int device, int k, int n_slabs, bool split);
void slab_destroy(Slab *S);      // (the caller has made the device idle)
// f(handle) for `whole` and every part, until one fails: -> its status, *failed = that handle
template <typename F>
int slab_each_handle(const Slab &S, Handle **failed, F f) {
    Handle *hs[4] = {S.whole, S.part[0], S.part[1], S.part[2]};
    for (Handle *h : hs)
        if (h) {
            const int st = f(h);
            if (st) { *failed = h; return st; }
        }
    return HJB_OK;
}
// One stage of the slab, enqueued: J_in -> J_out (the slab's haloed buffers), idx = the owned states' labels (may be null).
// `halo`: the event behind which J_in's halo planes are in place, recorded by the caller BEFORE this call (null: nothing to
// wait for).  Without a split: `cs` waits for it, then one launch.  With one, the strips run on streams of their own beside the
// interior - each launch of the column-sweep kernel lasts at least one column (~0.2 ms); in line behind the interior two strips
// would cost more than the transfers hide.  A strip starts behind everything cs held at the call (event `fork`) and behind
// `halo`, and records sdone[k]; when the call returns cs has waited for both.  strips_first: the strips are enqueued before the
// interior (their halos are there already).  The current device is S.device.  On failure *err and g_last_error say why.
int slab_enqueue_stage(Slab &S, const void *J_in, void *J_out, void *idx, hipStream_t cs, hipEvent_t halo, bool strips_first, std::string *err);

}  // namespace hjbhost

// hjbdp_builder.hip: the flat builder (hjb_problem_new ...) and its problem with the pointers bound
struct hjb_builder_s {
    hjb_problem p{};
    std::vector<std::vector<double>> knots;
    std::vector<std::vector<unsigned char>> blobs;   // owned copies of every term / model table
    std::string err;
};
extern "C" {
int builder_bind(hjb_builder b, hjb_problem *out);
int bfail(hjb_builder b, int code, const char *fmt, ...);
}
