/* hjbdp.h - C ABI of libhjbdp: the Bellman-backup hot path of grid-based HJB
 * dynamic programming on AMD MI355X (gfx950).
 *
 * The reference (abdolrezat/Optimal-Control-Dynamic-Programming, pure MATLAB) has
 * no FFI seam; the seam this library replaces is the per-stage statement every
 * solver repeats inside its stage loop
 *
 *     [F.Values, idx] = min( J_stage + F(x_next_1,...,x_next_D), [], ctrl_dim )
 *
 *   test/Dynamic_Solver.m:207-210           (J_state_M, called from run :86-102)
 *   position-control/Solver_position.m:135-137   (simplified_run :132-141)
 *   attitude-control/Solver_attitude.m:239-241   (simplified_run :236-247)
 *   attitude-control/Solver_attitude.m:400-409   (calculate_J_U_opt_state_M, run :280-287)
 *   pos-att/Solver_pos_att.m:272                 (calculate_one_channel_U_Opt :270-286)
 *
 * plus the loop around it (hjb_solve) including the pos-att early-stop monitor
 * (Solver_pos_att.m:268-285).  F is griddedInterpolant(...,'linear'): N-linear
 * interpolation with linear extrapolation; min returns the first minimal index.
 *
 * Conventions (MATLAB's): all arrays COLUMN-MAJOR, first index fastest; grid
 * dims 0..D-1 are state axes, D..D+C-1 control axes; argmin labels enumerate the
 * control dims column-major (ndgrid order) and are index_base-based.
 *
 * Plain C, caller-owned host pointers, no callbacks except the optional
 * progress function; never throws.  A MATLAB host binds this header with
 * loadlibrary/calllib; tests bind it with ctypes.
 */
#ifndef HJBDP_H
#define HJBDP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HJB_MAX_D 6      /* state dims   (Solver_attitude.run: 6)            */
#define HJB_MAX_C 3      /* control dims (Solver_attitude.run: U1,U2,U3)     */
#define HJB_MAX_G 9      /* D + C        (reshape_states: dims 1..9)         */
#define HJB_MAX_TERMS 12 /* broadcast terms per quantity (attitude cost: 9)      */

/* status codes */
#define HJB_OK 0
#define HJB_E_INVALID 1      /* bad argument / inconsistent problem           */
#define HJB_E_UNSUPPORTED 2  /* valid but not supported (D, C, dtype)         */
#define HJB_E_DEVICE 3       /* HIP error; text via hjb_last_error            */
#define HJB_E_NOMEM 4
#define HJB_E_HALO 5         /* a query left the slab's halo (multi-GPU)      */

#define HJB_F32 0
#define HJB_F64 1
#define HJB_F16S 2   /* float32 arithmetic, tables and knots; J buffers (terminal, J_final, J_stages,
                        device J) stored as IEEE binary16, rounded to nearest even on store -
                        halves the cost-to-go footprint (288 GB sizing of the 6-D grids)   */

/* One broadcast term of an ordered sum  q = ((t0 + t1) + t2) + ...
 * This is MATLAB implicit expansion of vectors/arrays reshaped onto the
 * D+C grid dims (Solver_attitude.m:717-742 reshape_states; Solver_pos_att.m
 * :307-314, :791-801): bit d of mask set <=> the term varies along grid dim d.
 * data: host array of the problem's dtype, column-major over the masked dims
 * in increasing dim order. */
typedef struct hjb_term {
    uint32_t mask;
    uint32_t reserved;
    const void *data;
} hjb_term;

typedef struct hjb_problem {
    int32_t D;                      /* number of state axes, 1..HJB_MAX_D      */
    int32_t C;                      /* number of control axes, 1..HJB_MAX_C    */
    int32_t n[HJB_MAX_D];           /* state grid sizes (>= 2)                 */
    int32_t m[HJB_MAX_C];           /* control grid sizes (>= 1)               */
    int32_t dtype;                  /* HJB_F32 / HJB_F64 / HJB_F16S: arithmetic type of J,
                                       tables, knots and weights               */
    int32_t index_base;             /* 0 or 1 (MATLAB) for argmin labels       */
    const double *knots[HJB_MAX_D]; /* grid vectors, strictly increasing, may be
                                       non-uniform (Solver_pos_att.m:906-918);
                                       rounded to dtype inside                 */
    /* x_next_a = ordered sum of terms (a_D_M Dynamic_Solver.m:184-188;
       next_stage_states_simplified Solver_pos_att.m:299-328; ...)             */
    int32_t n_next_terms[HJB_MAX_D];
    hjb_term next_terms[HJB_MAX_D][HJB_MAX_TERMS];
    /* stage cost g = ordered sum of terms (g_D Dynamic_Solver.m:196-200;
       J_current_reshaped Solver_pos_att.m:784-802; ...)                       */
    int32_t n_cost_terms;
    int32_t idx_dtype;              /* storage type of the argmin labels (idx_final, idx_stages, d_idx_out):
                                       HJB_IDX_I32 (0, default), HJB_IDX_U8, HJB_IDX_U16, or HJB_IDX_AUTO = the narrowest
                                       that holds nU - 1 + index_base (MATLAB's U_Optimal_id of Solver_pos_att.m:272
                                       carries 9 distinct values: one byte per state instead of four); the width in
                                       effect is hjb_info.idx_bytes */
    hjb_term cost_terms[HJB_MAX_TERMS];
    /* Slab decomposition along the LAST state axis (multi-GPU; all four zero =
       whole grid).  The handle owns planes [slab_begin, slab_end) and every J
       buffer it is given covers planes [slab_begin-halo_lo, slab_end+halo_hi). */
    int32_t slab_begin, slab_end, halo_lo, halo_hi;
    /* Optional on-the-fly model of the LEADING state axes (those whose next value does not depend on the
       control).  HJB_MODEL_NONE: every axis is described by next_terms.  HJB_MODEL_QUAT_EULER321 (D == 6, C == 3):
       axes 0,1,2 = (yaw, pitch, roll), axes 3,4,5 = (w1, w2, w3); n_next_terms[0..2] must be 0 and the next angles
       are computed per state as attitude-control/Solver_attitude.m:449-489 does (Euler step of the quaternion
       kinematics with step model_h, renormalise, back to Euler angles) from model_tables[0..3] = the quaternion
       components x4,x5,x6,x7 of the grid angles (Solver_attitude.m:419-421; arrays over (n[0],n[1],n[2]),
       column-major, problem dtype HJB_F32/HJB_F16S) and the knots of axes 3..5.  This replaces the three
       nS-sized next-angle tables, which do not fit at 51^6.  atan2/asin use the library's own
       fixed polynomial forms, so that results are reproducible bit for bit across CPUs/GPUs.
       The pitch argument s = -2 (x6 x4 - x7 x5) is clamped to [-1, 1] before the asin (the clamp is ours, the
       reference would go complex: at pitch +-90 degrees the rounded quaternion gives |s| = 1 + 1..2 ulp), so a
       grid with a pitch knot at +-pi/2 gives next pitch +-float(pi/2), never NaN; where |s| <= 1 nothing changes.
       The atan2 reads the signs of its arguments with `< 0`, so a zero of either sign counts as positive: it
       returns +pi at (y = -0, x < 0) where libm returns -pi, and 0 at (y = +-0, x = -0) where libm returns
       +-pi, and +0 at (y = -0, x >= 0) where libm returns -0.  Everywhere else it is within 4 ulp of libm.  The tables must be finite and
       no entry the zero quaternion (0 / 0 is the caller's error). */
    int32_t model;
    int32_t table_dtype;            /* HJB_TAB_DEFAULT (0): next-state terms are arrays of the problem dtype and the
                                       queries are formed, located and weighted in it.  HJB_TAB_F64 (dtype HJB_F32 /
                                       HJB_F16S only): the data of every next_terms entry are float64 - the reference's
                                       pos-att typing (Solver_pos_att.m:299-327 keeps x_next .. w_next in double while
                                       F_gI.Values is single, :264-265): each query is summed in double, its cell is found
                                       on the float64 knots, its weight (q - k[c]) * (1 / (k[c+1] - k[c])) is formed in
                                       double and rounded to float32 ONCE; the blend and the cost stay float32.  The
                                       (cell, weight) tables are stage-invariant, so this costs nothing per stage; only
                                       the table-driven stage kernels (variants 5, 6, 7 and the multi-stage 2-D kernel)
                                       serve such a problem.  cost_terms stay arrays of the problem dtype. */
    double model_h;
    const void *model_tables[4];
    int32_t cost_dtype;             /* HJB_COST_DEFAULT (0): cost_terms are arrays of the problem dtype, summed in it.
                                       HJB_COST_F64 (dtype HJB_F32 / HJB_F16S, no state model): the data of every
                                       cost_terms entry are float64 and the stage cost of a (state, control) is the ordered
                                       sum of the terms IN DOUBLE, rounded to float32 ONCE - the reference's
                                       J_current_M = single(Qx*x.^2 + Qv*v.^2 + Qw*w.^2 + Qt*t.^2 + (R*f1.^2 + ...))
                                       (Solver_pos_att.m:800-801: a double expression under implicit expansion, one cast)
                                       without the [n_x,n_v,n_t,n_w,nU] array: bit-identical to passing that array as one
                                       term, at any grid size.  The state part is summed once per state, each control adds
                                       its part in double and rounds.  Served by the table-driven kernel (variant 5) and
                                       the column sweep (variant 7, state terms + one control term); ~10 % slower than
                                       float32 terms on C4. */
    int32_t reserved_;
} hjb_problem;

#define HJB_IDX_I32 0
#define HJB_IDX_U8 1
#define HJB_IDX_U16 2
#define HJB_IDX_AUTO 3

#define HJB_TAB_DEFAULT 0
#define HJB_TAB_F64 1

#define HJB_COST_DEFAULT 0
#define HJB_COST_F64 1

#define HJB_MODEL_NONE 0
#define HJB_MODEL_QUAT_EULER321 1

typedef struct hjb_handle_s *hjb_handle;

/* optional progress callback, replaces fprintf/waitbar in the stage loops
 * (Dynamic_Solver.m:101, Solver_pos_att.m:278): called at monitor points (and, with
 * hjb_solve_opts.progress_every_stage, after every stage) with the reference's k_s,
 * e = d(sum J), e2 = d(sum idx), elapsed seconds. */
typedef void (*hjb_progress_fn)(void *user, int32_t k_s, double e, double e2, double seconds);

/* Optional probe block = the reference's debug taps (test/Dynamic_Solver.m:212-219, `checkstagesXJF`): per stage the
 * reference copies the fixed sub-block (50:55, 52:57, 105) of J_current_state, X_next_M1, X_next_M2 (and, commented
 * out, of J_F_next) into *_check(:,:,k).  Here: any rectangular sub-block of states [lo, hi) (0-based, half open -
 * 50:55 is lo 49, hi 55) at ONE control (0-based index per control dim - 105 is 104).  With B = prod(hi - lo) block
 * states in column-major order, plane k_s - 1 of each output holds stage k_s (as J_stages does):
 *   g        [B, n_stages]     the stage cost g(x, u)                      (J_current_state_check)
 *   x_next   [B, D, n_stages]  the next-state coordinate of every axis     (X_next_M1_check, X_next_M2_check, ...)
 *   j_interp [B, n_stages]     J_{k+1} interpolated at x_next              (J_F_next_check)
 * all in the problem's arithmetic dtype (float for HJB_F16S); any of the three may be NULL. */
typedef struct hjb_probe {
    int32_t lo[HJB_MAX_D], hi[HJB_MAX_D];
    int32_t control[HJB_MAX_C];
    int32_t reserved;
    void *g;
    void *x_next;
    void *j_interp;
} hjb_probe;

typedef struct hjb_solve_opts {
    int32_t n_stages;        /* number of backups: N-1 (Dynamic_Solver.m:86), N_stage-1 */
    int32_t monitor_period;  /* 0 = off; 50 in Solver_pos_att.m:273                     */
    double monitor_tol;      /* 1e-2 in Solver_pos_att.m:269.  By default the two sums are float64 sums (fixed
                                reduction tree, reproducible); MATLAB's sum() of the single array F.Values is a
                                single-precision sum, so |e| < tol can first hold at a different monitor point there:
                                see monitor_single below */
    const void *terminal;    /* J_N [nS] dtype, NULL = zeros (Dynamic_Solver.m:83-84)   */
    void *J_final;           /* out [nS] dtype: J of the last computed stage (may be NULL) */
    void *idx_final;         /* out [nS] labels of hjb_problem.idx_dtype (int32 by default): argmin of the last
                                computed stage                                          */
    void *J_stages;          /* out [nS * n_stages] or NULL: stage with reference index
                                k_s (1-based, counting down from n_stages) is written
                                to plane k_s-1  (test_coder.m:32 J_star(:,:,k_s))       */
    void *idx_stages;        /* out [nS * n_stages] labels or NULL (Dynamic_Solver.m:100) */
    hjb_progress_fn progress;
    void *progress_user;
    const hjb_probe *probe;  /* NULL = no debug taps (Dynamic_Solver.m:212-219)                    */
    int32_t progress_every_stage; /* 0: progress is called at monitor points only; 1: after every stage (the reference
                                     prints per stage, Dynamic_Solver.m:101; e, e2 are then 0 between monitor points) */
    int32_t monitor_single;  /* 1: the monitor's sum of J is accumulated in float32, as MATLAB's sum() of the single
                                array F_gI.Values is (Solver_pos_att.m:274; dtype HJB_F32 / HJB_F16S, one device).
                                MATLAB's own summation order is not documented; the order used here is the fixed
                                tree stated in csrc/kernels_reduce.h, restated by the oracle.  The label sum stays
                                exact (U_Optimal_id is a double array there).  The difference e = fsum50 - fsum50_prev
                                and the test abs(e) < tol are then single-precision too (:276-282; MATLAB casts the
                                double tol to single).  0: float64 sums, float64 difference and test */
} hjb_solve_opts;

typedef struct hjb_result {
    int32_t stages_done;     /* < n_stages if the monitor stopped the sweep             */
    int32_t stopped_early;
    double sweep_ms;         /* device time of the stage loop (HIP events)              */
    double last_e, last_e2;  /* monitor deltas at the last monitor point                */
} hjb_result;

typedef struct hjb_info {
    int64_t n_states;        /* states this handle owns                                 */
    int64_t n_controls;
    int64_t j_elems;         /* elements of a J buffer (owned + halo planes)            */
    int32_t kernel_variant;  /* which stage kernel hjb_create selected                  */
    int32_t lds_bytes;
    int32_t block, grid;
    int32_t halo_needed_lo;  /* conservative halo the tables imply (planes)             */
    int32_t halo_needed_hi;
    int32_t idx_bytes;       /* bytes per stored argmin label: 4, 1 or 2 (hjb_problem.idx_dtype resolved) */
    int32_t table_dtype;     /* HJB_TAB_* in effect                                     */
    int32_t cost_dtype;      /* HJB_COST_* in effect                                    */
    int32_t reserved_;
} hjb_info;

const char *hjb_version(void);
const char *hjb_status_string(int32_t status);
/* number of visible HIP devices, or 0 */
int32_t hjb_device_count(void);
/* Fault injection for the test suite (NOT for production hosts): an explicit in-process call - the library never reads
 * the environment to change behaviour.  Keys: "fail_tab64_scratch" (value != 0: the float64 table build's scratch
 * allocation fails, so that hjb_create's refusal of an unservable HJB_TAB_F64 problem can be tested),
 * "fail_tabled_alloc" (the (cell, t) table allocation of the table-driven kernels fails: HJB_COST_F64's refusal),
 * "rccl_only_env" (the RCCL loader tries $HJBDP_RCCL_LIB only: a host without librccl),
 * "fail_graph_capture" (host side only: the stage-loop graph capture of hjb_solve / hjb_solve_batch fails before any HIP
 * call with HJB_E_DEVICE and "(test hook)" in the text; the handles stay usable). */
int32_t hjb_test_hook(const char *key, int64_t value);

/* Threading: a handle is not thread-safe - drive each handle from one host thread.  DIFFERENT handles may be
 * driven from different threads at the same time (each hjb_solve runs on its handle's own HIP stream): this is how
 * the independent channels of the spacecraft solvers run side by side.  The library serialises only what HIP
 * cannot overlap safely (stream capture against allocation / synchronous copies); hjb_create and hjb_solve wait for
 * their own set-up (issued on the null stream), never for the whole device, so a handle does not wait for another
 * handle's sweep.  (Measured, round 5: an MI355X runs two such launch chains at full rate; a third waits.)
 *
 * Validate the problem, copy tables and knots to `device`, pick a kernel. */
int32_t hjb_create(const hjb_problem *problem, int32_t device, hjb_handle *out);
int32_t hjb_destroy(hjb_handle h);
/* text of the last error on this handle (h may be NULL: last create error) */
const char *hjb_last_error(hjb_handle h);
int32_t hjb_get_info(hjb_handle h, hjb_info *info);
/* tuning/testing knobs: "variant" (-1 automatic, 0..7 force a stage kernel; HJB_E_UNSUPPORTED when it does not
 * apply), "graph" (0/1: hipGraph replay inside hjb_solve), "temporal" (several stages per launch inside hjb_solve
 * for local 2-D problems, kernels_tile2d.h: 0 off, 1 when applicable [default], 2 required), "row_lean" (0/1: lean form of
 * stage kernel 6), "lds_pad" (extra dynamic LDS bytes per workgroup: occupancy experiments), "monitor_single" (0/1:
 * hjb_solve_opts.monitor_single for callers of hjb_solve_flat); read-only: "idx_bytes" */
int32_t hjb_set_option(hjb_handle h, const char *key, int64_t value);
/* "prep_mfma" (set): rebuild the handle's stage-invariant (cell, weight) tables - 1: with v_mfma_f32_32x32x2_f32 where an
 * axis' next-state sum splits into (all terms but the last) + (last term) over disjoint grid dims (the affine A x + B u
 * of every reference solver; csrc/kernels_prep_mfma.h), 0: with the vector kernels.  Bit-identical tables either way;
 * get: "prep_mfma", "prep_mfma_tables", "prep_tables", "prep_ns" (device time of the last rebuild), "table_hash",
 * "packed2_mode" (variant 4's contraction mode, csrc/kernels_packed2.h: 0 plain, 1 / 4 the C2 shape with / without the axis-0
 * table, 2 / 3 the per-state window of the attitude shapes with four last-axis planes, 5 / 6 with three - chosen when the inner
 * control moves the last axis by less than its narrowest cell per step; -1 when variant 4 does not apply).  Settable:
 * "window_planes" (3 or 4: switch a handle that qualifies between modes 5 / 6 and 2 / 3; same results, tests and timing).
 * read a knob back, plus what the column-sweep kernel (variant 7) settled on: "cs_dpp" (1: one load per corner row, the
 * upper axis-0 neighbour taken from the next lane), "cs_groups", "cs_group_axis", "cs_rows" (corner rows per step of the
 * mid-grid column), "cs_cost_form" (0 general, 1 state terms + one control term, 2 the same summed in float64; -1 when
 * another variant runs), "cs_coop" (1: the cooperative form is in effect), "cs_coop_why" (why it does not apply: 0 applies,
 * 1 groups, 2 axis 1 sees the window axis, 3 n0 / storage, 4 cells, 5 window knots, 6 axis-0 knots).  Settable (testing,
 * tuning): "cs_dpp", "cs_coop" (1: eight neighbouring columns share their corner rows through LDS, kernels_colcoop.h;
 * off by default - slower on C4), "cs_xcd_mod" (residue modulus of the column -> XCD assignment: 0/1 contiguous ranges,
 * -1 the group spacing), "cs_xcd_axis" (0: the XCDs split the group axis [default], 1: the window axis), "cs_split" (parts
 * a column is swept in - each by a wave of its own, priming where it starts; 0 = automatic: more parts for launches with
 * few columns, e.g. the boundary strips of a multi-GPU slab; reads back the value in effect).  Variant 5: "tabled_i32"
 * (1 [default where every index of the problem fits 31 bits]: the table kernel's 32-bit form, 0: its general 64-bit form;
 * reads back the form a launch would take).  "grid" (get: workgroups per launch; set, timing experiments on the grid-stride
 * kernels only: the library's own choice walks a grid larger than the launch in equally long spans - until the next option that
 * re-chooses the launch).  "block" (set, variant 3: 256 / 512 / 1024 threads per workgroup = 64 x the states it sweeps side by
 * side; 512 by default where J is staged in LDS.  Variant 8: 64 / 128 / 256, same bits - its min form strides by the launch). */
int32_t hjb_get_option(hjb_handle h, const char *key, int64_t *value);

/* ONE backup, host buffers (exactly the MATLAB statement above):
 * J_next [j_elems] -> J_out [j_elems] (owned planes written), idx_out [n_states]. */
int32_t hjb_backup_stage(hjb_handle h, const void *J_next, void *J_out, void *idx_out);
/* ONE backup on device buffers, asynchronous on `stream` (a hipStream_t; NULL =
 * default stream).  For host-driven loops and multi-GPU halo exchange.
 * Streams: one handle may have launches in flight on several streams at once (from its one host thread), also beside a
 * hjb_solve on the handle's own stream; the caller owns the ordering of the buffers it passes.  The device state a launch
 * writes is per stream: the claim counters of kernel 15's chunk walk are kept per stream for the first 8 streams a handle
 * sees, and launches on further streams take the walk's static form (the same results).  The halo flag
 * (hjb_check_device_status) is shared: a fault on any stream is reported by the next check on any of them. */
int32_t hjb_backup_stage_device(hjb_handle h, const void *dJ_next, void *dJ_out,
                                void *d_idx_out, void *stream);
/* Non-zero if a previous device-side backup hit HJB_E_HALO (synchronises). */
int32_t hjb_check_device_status(hjb_handle h, void *stream);

/* ---- device-buffer helpers --------------------------------------------------------------------------------------
 * hjb_backup_stage_device works on device buffers the CALLER owns.  A host without a HIP binding of its own (MATLAB
 * through calllib, plain C) gets them here - enough to drive a grid that never exists in host memory (C3: 51^6 states,
 * 70 GB per buffer).  Pointers returned by hjb_device_malloc are ordinary HIP device pointers (hipMalloc). */
#define HJB_COPY_H2D 0
#define HJB_COPY_D2H 1
#define HJB_COPY_D2D 2
int32_t hjb_device_malloc(int32_t device, int64_t bytes, void **out);
int32_t hjb_device_free(int32_t device, void *p);
int32_t hjb_device_mem_info(int32_t device, int64_t *free_bytes, int64_t *total_bytes);
int32_t hjb_device_copy(int32_t device, void *dst, const void *src, int64_t bytes, int32_t kind);   /* synchronous */
/* dJ[s] = ((v0[i0] + v1[i1]) + v2[i2]) + ...  over the handle's whole grid: one add of the arithmetic type per axis,
 * axis 0 first, stored in the handle's J storage type.  vecs[a]: HOST vector of n[a] elements of the arithmetic type
 * (float for HJB_F32 / HJB_F16S).  A separable terminal cost for grids too large to build on the host.  On a SLAB handle dJ is
 * the slab's haloed buffer and is filled with the planes [slab_begin - halo_lo, slab_end + halo_hi) of that global function. */
int32_t hjb_device_fill_separable(hjb_handle h, const void *const *vecs, void *dJ, void *stream);
/* out[i] = d_src[sel[i]] for elements of elem_bytes (1, 2, 4, 8) bytes: sample a device-resident J or label array */
int32_t hjb_device_gather(int32_t device, const void *d_src, int32_t elem_bytes, const int64_t *sel, int64_t n_sel, void *out);

/* The whole backward sweep (the `for k` loops of the reference). */
int32_t hjb_solve(hjb_handle h, const hjb_solve_opts *opts, hjb_result *result);
/* n independent problems of ONE kernel shape swept side by side with ONE launch per stage for all of them: the four channels of
 * Solver_pos_att.simplified_run (pos-att/Solver_pos_att.m:197-242: 2.7e5 states each - a stage kernel of one channel is a launch
 * boundary plus one wave's chain of round trips, and of four such chains on four streams the device runs two at full rate).
 * Every problem keeps its own terminal cost, outputs, monitor sums / difference / stop decision (a stopped problem drops out of
 * the launches that follow) and progress callback; its results equal hjb_solve's bit for bit.  Conditions (else
 * HJB_E_UNSUPPORTED, and the caller sweeps the problems with hjb_solve on threads of their own): n <= 8, one device, one n_stages
 * and one monitor_period for all, no per-stage outputs / probe / per-stage progress, and every handle on ONE of
 *   - the column-sweep kernel in its usual form (float32 J, state cost terms + one control term, the one-load form), one group
 *     axis and one cost typing; the columns are cut into parts for the whole batch unless option "cs_split" is set;
 *   - the table kernel's 32-bit form (kernel_variant 5, every index below 2^31), one dtype and one D <= 4.  Worth it while all the
 *     problems' states are resident at once (<= ~5e5 states in all: a launch-bound stage); larger ones overlap better as chains
 *     of their own (profiles/r06_batch_attitude.log). */
int32_t hjb_solve_batch(int32_t n, const hjb_handle *handles, const hjb_solve_opts *const *opts, hjb_result *const *results);

/* Batched evaluation of a gridded function at nq points - what the reference does with the
 * sweep's results: griddedInterpolant({grid vectors}, U_vector(U_idx), 'nearest') policy lookups
 * (Solver_position.m:144-146, Solver_pos_att.m:851-861, :404-449) and 'linear' lookups of
 * u_star(:,:,k) / J (Dynamic_Solver.m:132-135).  values: [n_1..n_D] column-major, dtype;
 * queries: [D x nq] column-major (point i = queries[D*i .. D*i+D-1]), dtype; out: [nq] dtype.
 * method HJB_LOOKUP_LINEAR: N-linear with linear extrapolation (same arithmetic as the sweep);
 * HJB_LOOKUP_NEAREST: per axis the nearer knot of the enclosing cell, the upper one at the midpoint.  Knots and
 * queries are rounded to dtype and every comparison is made in dtype; knots that are not strictly increasing after
 * that rounding are HJB_E_INVALID (decided before any device work). */
#define HJB_LOOKUP_NEAREST 0
#define HJB_LOOKUP_LINEAR 1
int32_t hjb_policy_lookup(int32_t device, int32_t dtype, int32_t D, const int32_t *n, const double *const *knots,
                          const void *values, int64_t nq, const void *queries, int32_t method, void *out);

/* One stage of the probe block from a host J_next (for host-driven stage loops): same outputs as hjb_probe, one
 * plane each (g [B], x_next [B, D], j_interp [B]).  J_next may be NULL when j_interp is NULL. */
int32_t hjb_probe_stage(hjb_handle h, const void *J_next, const hjb_probe *probe);

/* ---- the cost of a GIVEN policy on the grid (the fixed-label stage and its sweep) ---------------------------------------------
 *   J_k(x) = g(x, u_k(x)) + F_{k+1}(x_next(x, u_k(x)))          (no min: u_k is given)
 * `labels` are argmin labels as hjb_backup_stage / hjb_solve write them: one per OWNED state, of the handle's idx_dtype
 * (hjb_info.idx_bytes wide), in [index_base, index_base + n_controls), column-major over the control dims (control dim 0 fastest).
 * For every state the value is bit-identical to the candidate the backup kernels compare for that control, under every typing
 * (HJB_F32 / _F64 / _F16S, HJB_TAB_F64, HJB_COST_F64), so hjb_evaluate_stage on hjb_backup_stage's own labels returns its J.
 * Uses: the cost of the stationary controller the reference flies (the last stage's labels kept by simplified_run), a policy
 * judged under another handle's cost terms.  A handle with a state model (HJB_MODEL_QUAT_EULER321) is HJB_E_UNSUPPORTED.
 * hjb_evaluate_stage: host buffers, J_next and J_out [j_elems] in the (haloed) J layout (the owned planes are written; halo planes
 * of J_out repeat J_next), labels [n_states].  hjb_evaluate_stage_device: the same on device buffers, asynchronous on `stream`
 * (the stream rules of hjb_backup_stage_device); dJ_out's halo planes are not touched.  A handle's first evaluation builds the
 * (cell, weight) tables it reads if no stage kernel has yet (synchronous, on the null stream): call it once before a stream capture.
 * hjb_evaluate: the sweep of a fixed policy on a whole-grid handle (the handles hjb_solve accepts): n_stages >= 1 evaluations
 * from `terminal` (NULL = zeros).  labels_per_stage 0: labels [nS], one stationary policy used at every stage; 1: labels
 * [nS * n_stages], the stage with reference index k_s reads plane k_s - 1 (what hjb_solve's idx_stages holds).  J_final [nS] and
 * J_stages [nS * n_stages] (plane k_s - 1) may be NULL; sweep_ms (may be NULL) = device time of the loop.
 * HJB_E_INVALID, decided before any device work: a null handle, J_next, labels or J_out; n_stages < 1; labels_per_stage not 0 or
 * 1; and, for the two host-buffer calls, ANY label out of range anywhere in the array (the outputs are then left untouched).
 * The device-buffer call cannot look first: for a label out of range the kernel reads nothing, stores NaN for that state (every
 * other state gets its value) and raises a flag of its own, which the next hjb_check_device_status reports as HJB_E_INVALID
 * (once: reporting clears it; a left slab, HJB_E_HALO, is reported first when both are raised).
 * Options (hjb_set_option): "eval_grid" workgroups per launch (0 = one per 256 states; the kernel strides), "eval_tables" the
 * source of cells and weights: -1 the handle's (cell, weight) tables where they fit, 0 the terms summed in the kernel, 1 tables;
 * "eval_i32" 0 runs the kernel's 64-bit form even where every index fits 31 bits, "eval_m24" 0 its 32-bit form without 24-bit
 * index products even where every factor fits 24 bits (same bits either way; timing experiments, tests).  hjb_get_option
 * "eval_form" (read-only: setting it is HJB_E_INVALID) is the form the next launch runs from the source in effect: 0 64-bit,
 * 1 32-bit, 2 32-bit with 24-bit index products. */
int32_t hjb_evaluate_stage(hjb_handle h, const void *J_next, const void *labels, void *J_out);
int32_t hjb_evaluate_stage_device(hjb_handle h, const void *dJ_next, const void *d_labels, void *dJ_out, void *stream);
int32_t hjb_evaluate(hjb_handle h, int32_t n_stages, const void *terminal, const void *labels, int32_t labels_per_stage,
                     void *J_final, void *J_stages, double *sweep_ms);

/* ---- a disturbance in the backup: expected-value and worst-case stages (kernel variant 8) ----------------------------------------
 *   J_k(x) = min_u  g(x, u) + E_w[ F_{k+1}(x_next(x, u) + d_w) ]          (HJB_DIST_EXPECT: sum_w p_w (.))
 *   J_k(x) = min_u  g(x, u) + max_w F_{k+1}(x_next(x, u) + d_w)           (HJB_DIST_WORST)
 * The stochastic and minimax backups of the textbooks (Kirk; Bertsekas) over n_nodes additive offsets of the next state, the same
 * for every (state, control).  The setting lives on the handle: while it is set EVERY entry point that launches a stage -
 * hjb_backup_stage(_device), hjb_solve, hjb_solve_flat, hjb_evaluate_stage(_device), hjb_evaluate - serves the disturbed problem on
 * kernel variant 8 (hjb_info.kernel_variant reads 8) and no other variant serves the handle.  n_nodes == 0 detaches: the handle goes
 * back to the launch it had and gives the same bits as before.  A handle on which the call was never made is not affected at all.
 * offsets: [D, n_nodes] column-major (node w's offset of axis a at offsets[a + D * w]); weights: [n_nodes], HJB_DIST_EXPECT only,
 * NULL = 1 / n_nodes each.  T is the arithmetic type (float for HJB_F32 / HJB_F16S, double for HJB_F64), TQ the query type (double
 * under HJB_TAB_F64, else T).  Offsets are rounded once to TQ at the call, weights once to T; the NULL default is (T)(1.0 / n_nodes).
 * For each (state, control), visited in the generic kernel's order (control dim 0 slowest, first minimum wins, label written
 * column-major plus index_base):
 *   1. q_a = the ordered term sum of axis a in TQ, as in every kernel; for node w  q_aw = (TQ)(q_a + d[a][w]).  An axis whose
 *      offsets are all exactly zero is not offset at all: its query, cell and weight are formed once per control and shared by
 *      the nodes.  Option "dist_axes" (read-only) is the mask of the offset axes.
 *   2. cell and weight of q_aw as everywhere: the exact cell search, t = (q - k[c]) * (1 / dx[c]) formed in TQ and rounded to float
 *      once under HJB_TAB_F64; linear extrapolation outside the grid.
 *   3. v_w = the N-linear blend of J_{k+1}: the fma cascade, axis 0 first.
 *   4. HJB_DIST_EXPECT: acc = (T)(p_0 * v_0), then acc = fma(p_w, v_w, acc) for w = 1 .. n_nodes - 1 in node order.
 *      HJB_DIST_WORST:  acc = v_0, then acc = v_w > acc ? v_w : acc (the first maximum; a NaN never replaces).
 *   5. candidate = (T)(g + acc), g formed as everywhere (HJB_COST_F64: state part summed once in double, each control adds its
 *      part and rounds once).
 * With labels given (hjb_evaluate*) the same kernel forms that one candidate and takes no min; a label out of range follows the
 * rules above (NaN for that state, the flag hjb_check_device_status reports; the host-buffer calls look first).
 * Consequences: with ONE node, offset 0 and weight 1, in either mode, J and labels equal the undisturbed backup's bit for bit under
 * every typing; hjb_evaluate_stage on the disturbed backup's own labels returns its J bit for bit, and on ANY labels values >= it.
 * Refused before any device work, the handle left as it was (text: hjb_last_error) - HJB_E_INVALID: a null handle; a mode other than
 * the two; n_nodes < 0 or > HJB_DIST_MAX_NODES; null offsets with n_nodes > 0; an offset that is not finite; a weight that is not
 * finite or is negative; weights given with HJB_DIST_WORST.  HJB_E_UNSUPPORTED: a slab handle (any slab field non-zero: an offset
 * last axis changes the halo), a handle with a state model.  While a disturbance is set: hjb_solve with a probe, hjb_solve_batch
 * with such a handle among its members and option "temporal" = 2 are HJB_E_UNSUPPORTED ("temporal" = 1 runs plain stages);
 * option "graph" works as ever.  The multi-GPU objects take no disturbance.
 * Options: read-only "dist_nodes", "dist_mode", "dist_axes", "dist_form" (the index form the next launch runs: 0 64-bit, 1 32-bit,
 * where "eval_form" would be at least 1); settable "dist_i32" (0: the 64-bit form whatever the sizes; same bits - timing, tests). */
#define HJB_DIST_EXPECT 0
#define HJB_DIST_WORST 1
#define HJB_DIST_MAX_NODES 128
int32_t hjb_set_disturbance(hjb_handle h, int32_t mode, int32_t n_nodes, const double *offsets, const double *weights);

/* ---- a control-dependent disturbance in the backup (kernel variant 8, per-control form: K32) --------------------------------------
 *   J_k(x) = min_u  g(x, u) + E_w / max_w F_{k+1}(x_next(x, u) + d_w(u))
 * The node set depends on the candidate control: actuator noise, x+ = A x + B (u (1 + eps_w)), has d_w(u) = B u eps_w - "no
 * control" is noise-free, a large control is uncertain, and the optimal policy becomes cautious.  Additive nodes cannot say that.
 * Same modes, weights, rounding rules and consequences as hjb_set_disturbance above; only step 1 of its contract changes:
 *   1. for node w of the candidate with 0-based column-major control label l (the number the stage writes, minus index_base)
 *      q_aw = (TQ)(q_a + d[a][w][l]).
 * offsets: [D, n_nodes, n_controls] column-major - offsets[a + D * (w + n_nodes * l)] - each entry rounded once to TQ at the call.
 * n_controls must equal the handle's nU (it is there so that a table of the wrong size is refused instead of read past).
 * Steps 2 - 5 are hjb_set_disturbance's word for word: cell and weight, the fma cascade, acc = (T)(p_0 v_0) then fma(p_w, v_w, acc)
 * or the first maximum, candidate (T)(g + acc).  Every node is evaluated for every control, also for a control whose offsets are
 * all zero: the bits are defined by the contract, not by a shortcut.  The offset-axis mask ("dist_axes") has bit a set iff some
 * (w, l) entry of row a is not zero; an axis outside the mask is located once per control, as there.
 * The setting is of the same kind as hjb_set_disturbance's and lives in the same place: every entry that launches a stage serves it
 * (hjb_backup_stage(_device), hjb_solve, hjb_solve_flat, hjb_evaluate_stage(_device), hjb_evaluate), hjb_info.kernel_variant reads
 * 8, the two setters replace each other, and n_nodes == 0 through either detaches (n_controls is then not looked at): the handle
 * returns to the launch and the bits it had.
 * Consequences: (i) a table that is constant along l gives J and labels bit for bit those of hjb_set_disturbance with that node set,
 * under every typing; (ii) one zero node is the undisturbed backup; (iii) for any fixed label l0 the candidate equals
 * hjb_set_disturbance's candidate under the node set offsets[:, :, l0]; (iv) the fixed-label form (hjb_evaluate*) shares the min
 * form's candidates: its own labels return its J, any labels values >= it, a label out of range NaN and the flag.
 * Refused before any device work, the handle left as it was: everything hjb_set_disturbance refuses; HJB_E_INVALID: n_controls < 0
 * or, with n_nodes > 0, n_controls != nU; HJB_E_UNSUPPORTED: D * n_nodes * nU > 2^26 entries (the table stays within 512 MiB and its
 * index within 32 bits).  While it is set the same three refusals hold: a probe in hjb_solve, membership in hjb_solve_batch,
 * option "temporal" = 2.
 * Options: read-only "dist_ctrl" (1 while the disturbance in effect is this one, else 0); "dist_nodes", "dist_mode", "dist_axes",
 * "dist_form" and "dist_i32" as above.  Flying under such noise: hjb_rollout_run_actuator (kernel K33, below). */
#define HJB_CTRL_DIST_MAX_ENTRIES 67108864 /* 2^26 */
int32_t hjb_set_control_disturbance(hjb_handle h, int32_t mode, int32_t n_nodes, int32_t n_controls, const double *offsets,
                                    const double *weights);

/* ---- batched closed-loop rollouts of a stored policy (test/Dynamic_Solver.m:108-181 get_optimal_path, 'Nssu' and 'ssu') ----
 * A rollout object holds a per-stage policy on one device: the grid (D <= 6 axes, knots concatenated axis 0 first), the
 * labels of n_planes stages ([nS, n_planes] column-major in HJB_IDX_I32 / _U8 / _U16: hjb_solve's idx_stages layout) and the
 * control table u_table [n_labels, n_u] (column-major, n_u <= HJB_ROLLOUT_MAX_U).  Every label must lie in
 * [index_base, index_base + n_labels); the whole array is checked in hjb_rollout_create before any device work.
 * hjb_rollout_set_model gives the fixed-step affine closed loop x+ = A x + B u + c with stage cost x'diag(q)x + u'diag(r)u
 * (A [D, D], B [D, n_u] column-major; c, q, r may be NULL: no offset, zero weights).  hjb_rollout_run steps n_traj
 * trajectories n_steps times, one GPU thread each, all in double:
 *   p = plane_of_step[k];  u_j = policy lookup of u_table[labels[:, p] - index_base, j] at x (HJB_LOOKUP_NEAREST / _LINEAR:
 *       bit-identical to hjb_policy_lookup in double on those dense values);
 *   cost += ((q0*(x0*x0) + q1*(x1*x1)) + ...) + r0*(u0*u0) + ...;
 *   x+_a = ((A[a,0]*x0 + A[a,1]*x1) + ...) + B[a,0]*u0 + ... + c_a   (left to right, each product rounded).
 * X0, X_final: [D, n_traj]; X_path [n_traj, D, n_steps+1] and U_path [n_traj, n_u, n_steps] (NULL: not kept); device_ms: the
 * kernels' time.  Option "chunk" (default 1 << 20): trajectories per launch, which bounds the device memory of a run.
 * Option "lds" (default 1): 1 stages knots, 1/dx and u_table in LDS when they fit 32 KiB, 0 never stages (every run function of
 * the object then reads them from global memory: same bits; tests, timing experiments); any other value is HJB_E_INVALID.
 * One call at a time per object; different objects may run from different threads.  The handle is spelled void * (no typedef).
 * hjb_rollout_last_error(NULL): the text of the calling thread's last failure (create's refusals). */
#define HJB_ROLLOUT_MAX_U 4
int32_t hjb_rollout_create(int32_t device, int32_t D, const int32_t *n, const double *knots, int32_t idx_dtype,
                           int32_t index_base, int32_t n_planes, const void *labels, int32_t n_labels, int32_t n_u,
                           const double *u_table, void **rollout_out);
int32_t hjb_rollout_set_model(void *rollout, const double *A, const double *B, const double *c, const double *q,
                              const double *r);
int32_t hjb_rollout_set_option(void *rollout, const char *key, int64_t value);
int32_t hjb_rollout_run(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                        const double *X0, double *X_final, double *cost, double *X_path, double *U_path, double *device_ms);
int32_t hjb_rollout_destroy(void *rollout);
const char *hjb_rollout_last_error(void *rollout);

/* ---- noisy rollouts: the affine loop under sampled additive process noise (kernel K25) --------------------------------------
 *   x+ = A x + B u + c + d_w,   node w of a finite set (d_w, p_w) drawn per trajectory and step
 * - the model class of hjb_set_disturbance's additive next-state offsets, with the same layout (offsets [D, n_nodes] column-major,
 * weights [n_nodes] or NULL = equal) and the same limit HJB_DIST_MAX_NODES, so one node set serves both: design under it
 * (hjb_solve on a disturbed handle), price the policy under it (hjb_evaluate on that handle), fly it under it (here), compare.
 * hjb_rollout_set_noise gives the object a node set (n_nodes == 0 detaches).  The noise is a property of the object, independent
 * of the model; ONLY hjb_rollout_run_noisy reads it: hjb_rollout_run and every other run function of an object that holds noise
 * give the bits they gave before.  hjb_rollout_run_noisy is hjb_rollout_run (the affine model, the same arguments, the same
 * arithmetic in the same order) with, per step k after the affine update acc_a:
 *   w = the drawn node (below);  x+_a = acc_a + d[a][w] for every axis a of the offset mask - the axes with at least one offset
 *   that is not +-0; an axis outside the mask is not touched, not even by adding 0.0.
 * So with ONE node of zero offsets it equals hjb_rollout_run bit for bit.  W_path [n_traj, n_steps] (NULL: not kept): the drawn
 * node of every step, as a double.  The cost is the cost of the states actually visited.
 * The random stream and the sampler (csrc/hjbdp_noise.h, shared by the kernel and the two host twins below):
 *   generator   Philox4x32-10: multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds;
 *   addressing  counter-based, no state between calls: the stream of a trajectory is s = first_stream + i, a uint64, i the
 *               trajectory's index in the CALL (not in the chunk: option "chunk" does not change a bit); step k reads word k & 3
 *               of Philox(counter = (lo32 s, hi32 s, k >> 2, 0), key = (lo32 seed, hi32 seed)): one Philox call per four steps.
 *               One run of 2n trajectories equals two runs of n at first_stream and first_stream + n;
 *   thresholds  W - 1 doubles built once on the host, T[w] = floor(2^32 * (S_w / S_{W-1})), S_w = p_0 + ... + p_w summed left
 *               to right in double (NULL weights: p_w = 1.0 each); the drawn node is the number of w in [0, W-2] with
 *               T[w] <= (double)word.  Doubles keep T = 2^32 representable, so a trailing zero-weight node is never drawn; a
 *               zero-weight node anywhere is never drawn; W = 1 draws node 0.  Probabilities resolve to 2^-32.
 * hjb_rollout_noise_table writes the W - 1 thresholds of a weight vector; hjb_rollout_noise_draw writes the nodes n_traj streams
 * draw over n_steps steps (nodes [n_traj, n_steps], trajectory fastest) from thresholds in [0, 2^32] that do not decrease.  Both
 * run without a device and call the functions the kernel calls.
 * Refused before any device work, outputs untouched (text: hjb_rollout_last_error) - HJB_E_INVALID: a null handle; n_nodes outside
 * 0..HJB_DIST_MAX_NODES; null offsets with n_nodes > 0; an offset that is not finite; a weight that is not finite or is negative,
 * or weights that sum to 0; hjb_rollout_run_noisy with no noise set or with a model other than the affine one, and everything
 * hjb_rollout_run refuses; first_stream < 0 or first_stream + n_traj overflowing.  In the LDS form the node block (thresholds,
 * then the masked axes' offsets) is staged behind knots, 1/dx and u_table; the 32 KiB rule of option "lds" applies to the sum.
 * Noise that depends on the control (actuator noise): hjb_rollout_run_actuator (kernel K33, below).
 * Out of scope: noise that depends on the state, and continuous distributions (discretise them into nodes: the Gauss-Hermite and
 * box helpers of the host packages). */
int32_t hjb_rollout_set_noise(void *rollout, int32_t n_nodes, const double *offsets, const double *weights);
int32_t hjb_rollout_run_noisy(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                              const double *X0, uint64_t seed, int64_t first_stream, double *X_final, double *cost, double *X_path,
                              double *U_path, double *W_path, double *device_ms);
int32_t hjb_rollout_noise_table(int32_t n_nodes, const double *weights, double *thresholds);
int32_t hjb_rollout_noise_draw(uint64_t seed, int64_t first_stream, int64_t n_traj, int32_t n_steps, int32_t n_nodes,
                               const double *thresholds, int32_t *nodes);

/* ---- noisy campaigns: per-start cost statistics of the noisy loop, reduced on the device (kernel K28) ----------------------------
 * hjb_rollout_run_campaign flies n_starts starts n_samples (M) times each under the node set of hjb_rollout_set_noise, with the
 * stored-label controller of hjb_rollout_run_noisy, and returns one record of HJB_CAMPAIGN_NSTAT doubles per start.  No array of
 * the call, on the host or on the device, has a dimension of n_starts * M: the device memory of a call is bounded by option
 * "chunk" (the lanes of a launch; 8 doubles per block of a launch) and by n_starts ([D + 1 + 8, n_starts] doubles).
 * Trajectories.  Sample m of start s is hjb_rollout_run_noisy's trajectory from X0[:, s] on stream first_stream + s*M + m of
 *   `seed`: its cost c, its final state xf and its visited states are the bits hjb_rollout_run_noisy gives for an X0 with every
 *   start repeated M times.  Option "chunk" changes no bit.
 * Slot values of a sample.  v0 = c;  v1 = c*c, rounded;  v2 = c;  v3 = c;
 *   e = 1 iff threshold is given and c > threshold[s];
 *   l = 1 iff some visited state x_k, k = 0..n_steps, has an axis with !(knots_a[0] <= x_a && x_a <= knots_a[n_a-1]) - evaluated
 *       on the states as flown; a NaN counts as left;
 *   t = 1 iff tol is given and |xf_a| <= tol_a on every axis;   v7 = t ? c : +0.0.
 * Padding.  A padding slot holds v0 = v1 = v7 = +0.0, v2 = +inf, v3 = -inf and counts 0; it flies nothing and draws nothing.
 * Reduction order, independent of the launch layout (csrc/hjbdp_campaign.h, shared by the kernel and the host reduce):
 *   G = min(64, smallest power of two >= M).  The samples of a start form blocks of G consecutive samples; the last block is
 *   padded.  A block's partial is the adjacent-pair tree over its G slots: at level L, element i (a multiple of 2^(L+1)) becomes
 *   op(v[i], v[i + 2^L]) - sums: a + b;  min: b < a ? b : a;  max: b > a ? b : a.  The start's value is the block partials folded
 *   left to right in block order: acc = p_0, then acc = op(acc, p_b).  Counts are exact integers.  NaNs follow from these rules
 *   with no special case.
 * Output.  stats [HJB_CAMPAIGN_NSTAT = 8, n_starts] column-major: 0 sum, 1 sum of squares, 2 min, 3 max, 4 n_exceed, 5 n_left,
 *   6 n_settled (the three counts as doubles), 7 sum over the settled samples.  threshold [n_starts] or NULL; tol [D] or NULL.
 * hjb_rollout_campaign_reduce runs the same reduction on the CPU with no device, on per-trajectory arrays such as
 * hjb_rollout_run_noisy returns (trajectory s*M + m is sample m of start s): cost [n_starts*M], X_final [D, n_starts*M] or NULL
 * (required with tol), left [n_starts*M] uint8 (non-zero: left the grid) or NULL (n_left = 0).
 * Refused before any device work, outputs untouched (text: hjb_rollout_last_error) - HJB_E_INVALID: everything
 * hjb_rollout_run_noisy refuses (n_starts in the place of n_traj; no noise set; another model set); null stats; n_samples < 1;
 * n_starts * n_samples or first_stream + n_starts * n_samples overflowing int64; a threshold entry that is NaN; a tol entry that
 * is NaN or negative.
 * The campaign of the lookahead controller is hjb_rollout_run_lookahead_campaign (kernel K29, below): the same statistics on the
 * same streams; csrc/hjbdp_campaign.h serves both.
 * The histogram of a start's costs beside these statistics, and the quantiles it gives: hjb_rollout_run_campaign_hist (kernel
 * K30, below).
 * Out of scope: campaigns of the integrated plants. */
#define HJB_CAMPAIGN_NSTAT 8
int32_t hjb_rollout_run_campaign(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_starts,
                                 int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream, const double *threshold,
                                 const double *tol, double *stats, double *device_ms);
int32_t hjb_rollout_campaign_reduce(int64_t n_starts, int64_t n_samples, int32_t D, const double *cost, const double *X_final,
                                    const uint8_t *left, const double *threshold, const double *tol, double *stats);

/* ---- actuator-noise rollouts and campaigns: the affine loop under sampled control-dependent noise (kernels K33, K34) -------------
 *   x+ = A x + B (u (1 + eps_w)) + c + base_w,   node w of a finite set (eps_w, base_w, p_w) drawn per trajectory and step
 * - the model class of hjb_set_control_disturbance's actuator table (hjbdp.actuator_nodes: d_w(u) = B (u eps_w) + base_w), so one
 * node set serves the design (hjb_solve on such a handle), the price (hjb_evaluate) and the flight (here).  Everything in double,
 * one thread per trajectory, the affine model of hjb_rollout_set_model only.
 * hjb_rollout_set_actuator_noise gives the object an actuator node set (n_nodes == 0 detaches): eps [n_u, n_nodes] column-major
 * (eps[j + n_u * w]: the relative error of input j at node w), base [D, n_nodes] column-major or NULL (an additive node set on the
 * same nodes), weights [n_nodes] or NULL with hjb_rollout_set_noise's meaning, at most HJB_DIST_MAX_NODES nodes.  The set is a
 * property of the object, independent of hjb_rollout_set_noise's set and of the model; ONLY the two run functions below read it:
 * every other run function of an object that holds one gives the bits it gave before.
 * hjb_rollout_run_actuator is hjb_rollout_run_noisy word for word - the lookup, g, cost += g on the COMMANDED u, the affine update
 * acc_a, and the draw of node w (the same stream first_stream + i, the same thresholds, the same two statements) - with one change.
 * In the place of x+_a = acc_a + d[a][w]:
 *   1. an input j is LIVE iff some eps[j][w] is not +-0; for every live input ue_j = u_j * eps[j][w], one rounded product, formed
 *      once per step and used by every axis;
 *   2. the noise terms of axis a, in this order: for live j ascending with B[a,j] not +-0, B[a,j] * ue_j (the product rounded); then
 *      base[a][w] if row a of base has an entry that is not +-0;
 *   3. an axis with no term: x+_a = acc_a - not touched, not even by adding 0.0;
 *   4. otherwise n_a = the first term, n_a = n_a + term left to right, x+_a = acc_a + n_a.
 * Which terms exist is a launch constant: the live-input and base-axis masks are formed by the setter, B[a,j] != 0 is read from the
 * model in effect at the run (hjb_rollout_set_model may come before or after).  U_path holds the commanded u and W_path the drawn
 * node; the delivered control u_j + ue_j is not stored.
 * Consequences: (i) eps all +-0 with a base is hjb_rollout_run_noisy under hjb_rollout_set_noise(base, weights) bit for bit; with
 * no base (or one that is all +-0) it is hjb_rollout_run bit for bit, W_path still the drawn nodes; (ii) W_path equals
 * hjb_rollout_noise_draw for the same seed, streams and weights, so an additive and an actuator flight of one seed draw the same
 * nodes (common random numbers across plants); (iii) with n_u = 1 and HJB_LOOKUP_NEAREST, one step from a grid node x of a double
 * problem whose next-state terms are A[a,0] x0, A[a,1] x1, .., B[a,0] u lands on fl(q_a + off[a, w, l]), off the table of
 * hjbdp.actuator_nodes and l the label at x: the point hjb_set_control_disturbance's backup queries for (x, l, w); (iv) on an exactly
 * posed lattice problem the promised expected and worst-case costs are the costs paid.
 * hjb_rollout_run_actuator_campaign is hjb_rollout_run_campaign's contract with hjb_rollout_run_actuator in the place of
 * hjb_rollout_run_noisy: sample m of start s flies stream first_stream + s*M + m; the slots, the padding, the blocks of G, the tree,
 * the fold and the 8 doubles per start are K28's; no array has a dimension of n_starts * n_samples; options "chunk" and "lds"
 * change no bit; the statistics are bit for bit hjb_rollout_campaign_reduce of hjb_rollout_run_actuator's own outputs.
 * Refused before any device work, outputs untouched (text: hjb_rollout_last_error) - HJB_E_INVALID: a null handle; n_nodes outside
 * 0..HJB_DIST_MAX_NODES; null eps with n_nodes > 0; an eps or base entry that is not finite (named by input or axis and node);
 * a weight that is not finite or is negative, or weights that sum to 0; the run functions with no actuator set, and everything
 * hjb_rollout_run_noisy and hjb_rollout_run_campaign refuse.  In the LDS form the node block (thresholds, the live inputs' eps rows,
 * the base axes' rows, node index fastest) is staged behind knots, 1/dx and u_table; the 32 KiB rule applies to the sum.
 * Lookahead controllers that believe and fly actuator noise: hjb_rollout_run_control_lookahead (kernels K35, K36, below).
 * Out of scope: histogram and paired campaigns on this plant; the integrated plants; a general per-label table d[a][w][l] under
 * HJB_LOOKUP_NEAREST. */
int32_t hjb_rollout_set_actuator_noise(void *rollout, int32_t n_nodes, const double *eps, const double *base, const double *weights);
int32_t hjb_rollout_run_actuator(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                 const double *X0, uint64_t seed, int64_t first_stream, double *X_final, double *cost,
                                 double *X_path, double *U_path, double *W_path, double *device_ms);
int32_t hjb_rollout_run_actuator_campaign(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step,
                                          int64_t n_starts, int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream,
                                          const double *threshold, const double *tol, double *stats, double *device_ms);

/* ---- greedy rollouts: the affine loop flown by one-step lookahead on a stored cost-to-go (kernel K26) ---------------------------
 *   u_k(x) = argmin_l  g(x, u_l) + J_{k+1}(A x + B u_l + c)   over the rows u_l of the object's u_table, at the state visited
 * - the textbook DP controller: the other half of what hjb_solve(keep_J) returns.  It reads no label (the object's labels are not
 * touched) and does not interpolate between the labels of different controls.
 * hjb_rollout_set_values gives the object value planes: values [nS, n_planes] column-major in HJB_F32 or HJB_F64, hjb_solve's
 * J_stages layout, widened to double exactly on read (n_planes == 0 detaches).  The values are a property of the object, like the
 * noise; ONLY hjb_rollout_run_greedy reads them: every other run function of an object that holds values gives the bits it gave
 * before.  hjb_rollout_run_greedy steps n_traj trajectories n_steps times under the affine model of hjb_rollout_set_model, one
 * GPU thread each, all in double, every product rounded.  Step k at the state x:
 *   1. p = value_plane_of_step[k]: a plane of values, or -1 for the zero function (a terminal cost of zeros: v = +0.0 for every
 *      candidate and nothing is read);
 *   2. the state parts, once:  gs = (q0*(x0*x0) + q1*(x1*x1)) + ...;  as_a = (A[a,0]*x0 + A[a,1]*x1) + ...;
 *   3. for label l = 0 .. n_labels-1 in this order, u_j = u_table[l, j]:
 *        g_l  = gs + r0*(u0*u0) + ...;   xn_a = as_a + B[a,0]*u0 + ... (+ c_a if given)        (hjb_rollout_run's g and x+)
 *        v_l  = the N-linear blend of plane p at xn: the cell by exact search, clamped to [0, n-2] (outside the grid the blend
 *               extrapolates linearly; NaN: cell 0), t_a = (xn_a - k[cell]) * rdx[cell], fma lerps axis 0 first, pairwise:
 *               bit-identical to hjb_policy_lookup(..., HJB_LOOKUP_LINEAR) in double on that plane;
 *        cand_l = g_l + v_l;
 *   4. best = cand_0; label l >= 1 replaces iff cand_l < best: the first minimum wins, a NaN candidate never replaces;
 *   5. the chosen label applied: cost += g_best, x = xn_best - the bits step 3 formed.
 * X0, X_final, cost, X_path, U_path: hjb_rollout_run's.  L_path [n_traj, n_steps]: the chosen label + index_base, as a double;
 * V_path [n_traj, n_steps]: best, the cost-to-go the controller believed (NULL: not kept).  Options "chunk" (no bit changes with
 * it) and "lds" (knots, 1/dx and u_table staged when they fit 32 KiB; the value planes stay in global memory) as in
 * hjb_rollout_run.  hjb_rollout_greedy_host runs the same functions (csrc/hjbdp_greedy.h) on the CPU, with no device and no
 * object: the grid and table as hjb_rollout_create takes them, the model as hjb_rollout_set_model, the values as
 * hjb_rollout_set_values; its L_path holds the 0-based label.
 * Refused before any device work, outputs untouched (text: hjb_rollout_last_error) - HJB_E_INVALID: a null handle; a dtype other
 * than the two (HJB_F16S included: convert on the host); n_planes < 0; null values with n_planes > 0; hjb_rollout_run_greedy with
 * no affine model, with another model set, or with no values unless every plane index is -1; a plane index outside
 * -1 .. n_planes-1; and everything hjb_rollout_run refuses of n_steps, n_traj, X0 and X_final.
 * Lookahead under a disturbance and a greedy flight under hjb_rollout_set_noise's sampled noise: hjb_rollout_run_lookahead below.
 * Out of scope: the integrated plants of the other models, float16 value planes. */
int32_t hjb_rollout_set_values(void *rollout, int32_t dtype, int32_t n_planes, const void *values);
int32_t hjb_rollout_run_greedy(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_traj,
                               const double *X0, double *X_final, double *cost, double *X_path, double *U_path,
                               double *L_path, double *V_path, double *device_ms);
int32_t hjb_rollout_greedy_host(int32_t D, const int32_t *n, const double *knots, int32_t n_labels, int32_t n_u,
                                const double *u_table, const double *A, const double *B, const double *c, const double *q,
                                const double *r, int32_t dtype, int32_t n_value_planes, const void *values, int32_t n_steps,
                                const int32_t *value_plane_of_step, int64_t n_traj, const double *X0, double *X_final,
                                double *cost, double *X_path, double *U_path, double *L_path, double *V_path);

/* ---- disturbance-aware greedy rollouts: E_w / max_w lookahead, on a nominal or a noisy plant (kernel K27) -----------------------
 *   u_k(x) = argmin_l  g(x, u_l) + E_w[ J_{k+1}(A x + B u_l + c + e_w) ]      (HJB_DIST_EXPECT: sum_w p_w (.); HJB_DIST_WORST: max_w)
 * - the controller that is exactly optimal for the problem hjb_set_disturbance poses, evaluated at the state actually visited:
 * hjb_rollout_run_greedy with the disturbed backup's combine inside every candidate, and optionally hjb_rollout_run_noisy's plant.
 * hjb_rollout_set_lookahead gives the object a lookahead node set, in hjb_set_disturbance's layout (offsets [D, n_nodes]
 * column-major, weights [n_nodes], HJB_DIST_EXPECT only, NULL = 1.0 / n_nodes each; n_nodes == 0 detaches).  Weights are used as
 * given: they are NOT normalised (hjb_set_disturbance's rule in its float64 typing).  The lookahead set is what the controller
 * believes; the set of hjb_rollout_set_noise is the plant.  They are two independent properties of the object and may differ:
 * flying a controller designed for one noise under another is a use, not an error.  ONLY hjb_rollout_run_lookahead reads the
 * lookahead set: every other run function of an object that holds one gives the bits it gave before.
 * hjb_rollout_run_lookahead steps n_traj trajectories n_steps times under the affine model, one GPU thread each, all in double,
 * every product rounded.  Step k at the state x (csrc/hjbdp_lookahead.h, shared by the kernel and the host twin):
 *   1. p = value_plane_of_step[k]: a plane of hjb_rollout_set_values' values, or -1 for the zero function;
 *   2. the state parts gs and as_a, once: hjb_rollout_run_greedy's;
 *   3. for label l = 0 .. n_labels-1 in this order: u, g_l and xn_a are hjb_rollout_run_greedy's operations exactly; then
 *        - an axis outside the lookahead mask (the axes with at least one lookahead offset that is not +-0): its cell and t_a are
 *          formed from xn_a once per candidate and shared by the nodes; the axis is not touched, not even by + 0.0;
 *        - per node w = 0 .. n_nodes-1 in order: q_aw = xn_a + e[a][w] on every masked axis, its cell by the exact search clamped
 *          to [0, n-2] and t = (q_aw - k[cell]) * rdx[cell]; v_w = the N-linear blend of plane p (fma lerps axis 0 first,
 *          pairwise: hjb_rollout_run_greedy's blend at that point);
 *        - HJB_DIST_EXPECT: acc = p_0 * v_0 rounded, then acc = fma(p_w, v_w, acc) in node order;
 *          HJB_DIST_WORST:  acc = v_0, then acc = v_w > acc ? v_w : acc (the first maximum wins, a NaN never replaces);
 *          plane -1: acc = +0.0 and nothing is read;
 *        - cand_l = g_l + acc;
 *   4. best = cand_0; label l >= 1 replaces iff cand_l < best (the first minimum wins, a NaN candidate never replaces);
 *   5. the chosen label applied: cost += g, x = xn - formed again from the same operands;
 *   6. fly_noise = 1 only, hjb_rollout_run_noisy's sampler with nothing changed: a Philox block when (k & 3) == 0, the drawn node
 *      w' of the hjb_rollout_set_noise set, x_a = x_a + d[a][w'] on that set's mask only.  Streams s = first_stream + i count
 *      through the call whatever option "chunk" says.
 * So with ONE lookahead node of zero offsets and weight 1 (or NULL weights) and fly_noise = 0 it equals hjb_rollout_run_greedy
 * bit for bit; one step from a grid node under hjb_set_disturbance's set returns the disturbed backup's label and (HJB_F64) value.
 * X0, X_final, cost, X_path, U_path, L_path, V_path: hjb_rollout_run_greedy's; W_path [n_traj, n_steps]: the drawn node of every
 * step, as a double (fly_noise = 1 only).  fly_noise = 0: the plant is nominal, seed and first_stream are ignored.  Options
 * "chunk" and "lds" as in hjb_rollout_run; the lookahead block [p | e] is read through scalar registers and never staged; in the
 * LDS form the flight block is staged behind knots, 1/dx and u_table, the 32 KiB rule applied to the sum.
 * hjb_rollout_lookahead_host runs the same functions on the CPU, with no device and no object: hjb_rollout_greedy_host's
 * arguments, then the lookahead set (n_nodes >= 1), then optionally the nodes to fly - nodes [n_traj, n_steps] (trajectory
 * fastest: what hjb_rollout_noise_draw writes; NULL: a nominal plant) of the n_flight_nodes flight offsets [D, n_flight_nodes]
 * column-major, added on the axes that have an offset that is not +-0.  Its L_path holds the 0-based label.
 * Refused before any device work, outputs untouched (text: hjb_rollout_last_error) - HJB_E_INVALID: a null handle; a mode other
 * than the two; n_nodes outside 0..HJB_DIST_MAX_NODES; null offsets with n_nodes > 0; an offset that is not finite; a weight that
 * is not finite or is negative; weights given with HJB_DIST_WORST; hjb_rollout_run_lookahead with no lookahead set, with fly_noise
 * other than 0 or 1, with fly_noise = 1 and no noise set, first_stream < 0 or first_stream + n_traj overflowing, with fly_noise = 0
 * and a W_path, and everything hjb_rollout_run_greedy refuses.
 * Out of scope: the integrated plants of the other models, float16 value planes, noise that depends on the control or the state. */
int32_t hjb_rollout_set_lookahead(void *rollout, int32_t mode, int32_t n_nodes, const double *offsets, const double *weights);
int32_t hjb_rollout_run_lookahead(void *rollout, int32_t fly_noise, int32_t n_steps, const int32_t *value_plane_of_step,
                                  int64_t n_traj, const double *X0, uint64_t seed, int64_t first_stream, double *X_final,
                                  double *cost, double *X_path, double *U_path, double *L_path, double *V_path, double *W_path,
                                  double *device_ms);
int32_t hjb_rollout_lookahead_host(int32_t D, const int32_t *n, const double *knots, int32_t n_labels, int32_t n_u,
                                   const double *u_table, const double *A, const double *B, const double *c, const double *q,
                                   const double *r, int32_t dtype, int32_t n_value_planes, const void *values, int32_t n_steps,
                                   const int32_t *value_plane_of_step, int64_t n_traj, const double *X0, double *X_final,
                                   double *cost, double *X_path, double *U_path, double *L_path, double *V_path, int32_t mode,
                                   int32_t n_nodes, const double *offsets, const double *weights, const int32_t *nodes,
                                   int32_t n_flight_nodes, const double *flight_offsets);

/* ---- lookahead campaigns: per-start cost statistics of the flown lookahead, reduced on the device (kernel K29) ------------------
 * hjb_rollout_run_lookahead_campaign is hjb_rollout_run_campaign for the controller of hjb_rollout_run_lookahead: n_starts starts
 * flown n_samples (M) times each, one record of HJB_CAMPAIGN_NSTAT doubles per start.  The controller is the object's value planes
 * (hjb_rollout_set_values; value_plane_of_step, -1 = the zero function) under the lookahead set of hjb_rollout_set_lookahead; the
 * plant is the node set of hjb_rollout_set_noise.  The two sets may differ; the nominal greedy controller (K26) under noise is one
 * zero lookahead node of weight 1.  There is no nominal-plant form: a campaign of a deterministic flight is M copies of one number.
 * Trajectories.  Sample m of start s is hjb_rollout_run_lookahead's trajectory with fly_noise = 1 from X0[:, s] on stream
 *   first_stream + s*M + m of `seed`: its cost c, its final state xf and its visited states are the bits hjb_rollout_run_lookahead
 *   gives for an X0 with every start repeated M times.  Options "chunk" and "lds" change no bit.
 * Common random numbers.  Sample m of start s flies the same stream under every controller: hjb_rollout_run_campaign and this call
 *   with one seed, first_stream, n_starts and M draw the same node at every step of every sample, so the per-start means of the two
 *   controllers can be differenced with the sampling noise largely cancelled.
 * The statistics, the slot values of a sample, the padding, the reduction order and the output stats [HJB_CAMPAIGN_NSTAT, n_starts]
 *   are hjb_rollout_run_campaign's (above), word for word; the left-the-grid flag is evaluated on the states as flown, after the noise.
 *   hjb_rollout_campaign_reduce of hjb_rollout_run_lookahead's per-trajectory outputs gives the same bits.
 * Device memory of a call: [D + 1 + 8, n_starts] doubles plus 8 doubles per block of a launch; launches of at most option "chunk"
 *   lanes; a start's blocks may straddle launches.  No array has a dimension of n_starts * M.  Table placement is K27's.
 * hjb_rollout_lookahead_campaign_host runs the same functions on the CPU, with no device and no object: hjb_rollout_lookahead_host's
 * problem (D .. value_plane_of_step) and lookahead set (mode, n_nodes >= 1, offsets, weights), then the flight set (n_flight_nodes
 * >= 1, flight_offsets [D, n_flight_nodes] column-major, flight_weights or NULL = equal: hjb_rollout_set_noise's arguments), then
 * the campaign's arguments.  It never holds more than one start's samples.
 * Refused before any device work, outputs untouched (text: hjb_rollout_last_error) - HJB_E_INVALID: everything
 * hjb_rollout_run_lookahead refuses with fly_noise = 1 (n_starts in the place of n_traj; no lookahead set; no noise set; another
 * model set; a plane outside the value planes); null stats; n_samples < 1; n_starts * n_samples or first_stream + n_starts *
 * n_samples overflowing int64; a threshold entry that is NaN; a tol entry that is NaN or negative.  n_starts = 0 is HJB_OK.
 * The paired-difference statistic of two controllers on these streams, computed on the device: hjb_rollout_run_campaign_pair
 * (kernel K31, below).
 * Out of scope: sharing the first step's lookahead among a start's samples, campaigns of the integrated plants,
 * float16 value planes. */
int32_t hjb_rollout_run_lookahead_campaign(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_starts,
                                           int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream,
                                           const double *threshold, const double *tol, double *stats, double *device_ms);
int32_t hjb_rollout_lookahead_campaign_host(int32_t D, const int32_t *n, const double *knots, int32_t n_labels, int32_t n_u,
                                            const double *u_table, const double *A, const double *B, const double *c, const double *q,
                                            const double *r, int32_t dtype, int32_t n_value_planes, const void *values, int32_t n_steps,
                                            const int32_t *value_plane_of_step, int32_t mode, int32_t n_nodes, const double *offsets,
                                            const double *weights, int32_t n_flight_nodes, const double *flight_offsets,
                                            const double *flight_weights, int64_t n_starts, int64_t n_samples, const double *X0,
                                            uint64_t seed, int64_t first_stream, const double *threshold, const double *tol,
                                            double *stats);

/* ---- lookahead under actuator noise: the value function of hjb_set_control_disturbance flown directly (kernels K35, K36) -----------
 *   u_k(x) = argmin_l  g(x, u_l) + E_w[ J_{k+1}(A x + B u_l + c + e_w(l)) ]     (HJB_DIST_EXPECT; HJB_DIST_WORST: max_w)
 * - hjb_rollout_run_lookahead with a node set PER CANDIDATE, the controller that is exactly optimal for the problem
 * hjb_set_control_disturbance poses, flown on a nominal plant or on hjb_rollout_run_actuator's plant, and its campaign.
 * hjb_rollout_set_control_lookahead gives the object a per-control lookahead node set: offsets [D, n_nodes, n_controls]
 * column-major, the argument hjb_set_control_disturbance takes (offsets[a + D * (w + n_nodes * l)]: axis a, node w, 0-based label
 * l); weights and mode as hjb_rollout_set_lookahead's; n_controls must equal the object's label count (n_labels of
 * hjb_rollout_create), so that a wrong table is refused instead of read past; n_nodes == 0 detaches (n_controls is then not
 * read).  The set is a property of its own: hjb_rollout_set_lookahead's set is neither read nor changed by it, and ONLY the two
 * run functions below read it - every other run function of an object that holds one gives the bits it gave before.
 * hjb_rollout_run_control_lookahead is hjb_rollout_run_lookahead's contract (steps 1 - 5 above; csrc/hjbdp_ctrl_lookahead.h, shared
 * by the kernels and the host twin) with one change, the one hjb_set_control_disturbance makes to hjb_set_disturbance's:
 *   node w of the candidate with 0-based label l: q_aw = xn_a + e[a][w][l] on the masked axes; the mask has bit a set iff some
 *   (w, l) entry of row a is not +-0; an axis outside the mask is located once per candidate and is not touched by + 0.0.
 * Every node is evaluated for every candidate, a candidate whose offsets are all zero included.  Step 6, fly_noise = 1 only, is
 * hjb_rollout_run_actuator's plant with nothing changed, on the chosen label's xn and commanded u under the set of
 * hjb_rollout_set_actuator_noise: the node w' drawn from stream first_stream + i by hjb_rollout_run_noisy's sampler, ue_j = u_j *
 * eps[j][w'] for the live inputs, the terms of every axis summed left to right, x+_a = xn_a + n_a; the cost is charged on the
 * commanded u, U_path holds it, W_path the drawn node; which terms exist is formed from the model in effect at the run.  The
 * lookahead table is what the controller believes, the actuator set is the plant: two independent properties, which may differ.
 * So a table that is constant along l is hjb_rollout_run_lookahead under offsets[:, :, 0] bit for bit (fly_noise = 0); one zero
 * node is hjb_rollout_run_greedy; one step from a grid node under hjb_set_control_disturbance's table returns that backup's label
 * and (HJB_F64) value; and on an exactly posed lattice problem the flown run equals hjb_rollout_run_actuator of the stored labels.
 * Arguments, outputs and options: hjb_rollout_run_lookahead's, word for word; fly_noise = 0 is the nominal plant, 1 the actuator
 * set.  The table [p | for l: e (n_axes x n_nodes)] is read through scalar registers and never staged; in the LDS form the actuator
 * block is staged behind knots, 1/dx and u_table, the 32 KiB rule applied to the sum.  Option "chunk" changes no bit.
 * hjb_rollout_control_lookahead_host runs the same functions on the CPU, with no device and no object: hjb_rollout_greedy_host's
 * arguments, then the per-control set (n_nodes >= 1, n_controls == n_labels), then optionally the plant - nodes [n_traj, n_steps]
 * (what hjb_rollout_noise_draw writes; NULL: a nominal plant) of the n_flight_nodes actuator nodes eps [n_u, n_flight_nodes] and
 * base [D, n_flight_nodes] (or NULL), hjb_rollout_set_actuator_noise's arguments.  Its L_path holds the 0-based label.
 * hjb_rollout_run_control_lookahead_campaign is hjb_rollout_run_lookahead_campaign's contract with the flown run above in the place
 * of hjb_rollout_run_lookahead: sample m of start s flies stream first_stream + s*M + m - the stream
 * hjb_rollout_run_actuator_campaign gives the same (s, m), so a label campaign on the actuator plant and this one fly common random
 * numbers; the statistics are bit for bit hjb_rollout_campaign_reduce of hjb_rollout_run_control_lookahead's own outputs; no array
 * has a dimension of n_starts * n_samples; options "chunk" and "lds" change no bit.
 * Refused before any device work, outputs untouched (text: hjb_rollout_last_error) - HJB_E_INVALID: everything
 * hjb_rollout_set_lookahead refuses of mode, n_nodes, offsets and weights; n_controls < 0 or other than the label count; an entry
 * that is not finite (named by axis, node and control); the run functions with no per-control set, with fly_noise = 1 (the campaign:
 * always) and no actuator set, and everything hjb_rollout_run_lookahead and hjb_rollout_run_lookahead_campaign refuse of the other
 * arguments.  HJB_E_UNSUPPORTED: D * n_nodes * n_controls over HJB_CTRL_DIST_MAX_ENTRIES.
 * Out of scope: histogram and paired campaigns on this controller or plant; a control-dependent belief flown on the additive
 * hjb_rollout_set_noise plant; the integrated plants. */
int32_t hjb_rollout_set_control_lookahead(void *rollout, int32_t mode, int32_t n_nodes, int32_t n_controls, const double *offsets,
                                          const double *weights);
int32_t hjb_rollout_run_control_lookahead(void *rollout, int32_t fly_noise, int32_t n_steps, const int32_t *value_plane_of_step,
                                          int64_t n_traj, const double *X0, uint64_t seed, int64_t first_stream, double *X_final,
                                          double *cost, double *X_path, double *U_path, double *L_path, double *V_path, double *W_path,
                                          double *device_ms);
int32_t hjb_rollout_control_lookahead_host(int32_t D, const int32_t *n, const double *knots, int32_t n_labels, int32_t n_u,
                                           const double *u_table, const double *A, const double *B, const double *c, const double *q,
                                           const double *r, int32_t dtype, int32_t n_value_planes, const void *values, int32_t n_steps,
                                           const int32_t *value_plane_of_step, int64_t n_traj, const double *X0, double *X_final,
                                           double *cost, double *X_path, double *U_path, double *L_path, double *V_path, int32_t mode,
                                           int32_t n_nodes, int32_t n_controls, const double *offsets, const double *weights,
                                           const int32_t *nodes, int32_t n_flight_nodes, const double *eps, const double *base);
int32_t hjb_rollout_run_control_lookahead_campaign(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_starts,
                                                   int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream,
                                                   const double *threshold, const double *tol, double *stats, double *device_ms);

/* ---- campaign cost histograms: a per-start fixed-bin histogram of the costs beside the statistics (kernel K30) -----------------
 * hjb_rollout_run_campaign_hist and hjb_rollout_run_lookahead_campaign_hist are hjb_rollout_run_campaign and
 * hjb_rollout_run_lookahead_campaign - their arguments, their trajectories, their streams, and stats bit for bit theirs - with a
 * histogram of every start's n_samples (M) costs.  No array has a dimension of n_starts * M.
 * Inputs.  n_bins in 1..HJB_CAMPAIGN_MAX_BINS; lo [n_starts] and hi [n_starts], both finite, lo[s] < hi[s].
 * Scale.  scale_s = (double)n_bins / (hi[s] - lo[s]); it must be finite.
 * The bin of a sample with cost c (csrc/hjbdp_campaign.h, campaign_bin: one function serves the kernels and the host reduce):
 *   c < lo        record index 0 (underflow);
 *   !(c < hi)     record index n_bins + 1 (overflow); a NaN lands here;
 *   otherwise     b = (c - lo) * scale, the difference and the product each rounded; the index is 1 + min(n_bins - 1, (int)b).
 * Output.  hist [n_bins + 2, n_starts] column-major, int64 counts; every column sums to n_samples.  Padding slots and lanes past
 *   a launch's last block count nothing.  Option "chunk" changes no count; for the lookahead campaign option "lds" changes none either.
 * Why atomics are allowed here: the eight statistics keep their fixed floating-point order.  Integer addition commutes, so integer
 *   atomics do not break K28's rule: the result is a function of (M, the samples) alone.  The doubles are never accumulated so.
 * Two passes give an exact range: the streams are counter-based, so a plain campaign's min and max of a start are the min and the
 *   max of the samples a histogram call with the same seed, first_stream and n_samples bins; lo = min, hi = nextafter(max, +inf)
 *   leaves the underflow and the overflow empty.
 * Device memory of a call: the plain campaign's plus [3, n_starts] doubles and hist itself, zeroed once per call on the call's
 *   stream and accumulated across launches.
 * hjb_rollout_campaign_hist_reduce is the CPU twin with no device, on a cost array such as hjb_rollout_run_noisy returns: cost
 *   [n_starts*M], trajectory s*M + m sample m of start s.
 * Refused before any device work, outputs untouched - HJB_E_INVALID: everything the plain call refuses; n_bins out of range; with
 * n_starts > 0 a null lo, hi or hist; a lo or hi that is not finite; !(lo < hi); a scale that is not finite.  n_starts = 0 is HJB_OK. */
#define HJB_CAMPAIGN_MAX_BINS 256
int32_t hjb_rollout_run_campaign_hist(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_starts,
                                      int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream, const double *threshold,
                                      const double *tol, const double *lo, const double *hi, int32_t n_bins, double *stats, int64_t *hist,
                                      double *device_ms);
int32_t hjb_rollout_run_lookahead_campaign_hist(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_starts,
                                                int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream,
                                                const double *threshold, const double *tol, const double *lo, const double *hi,
                                                int32_t n_bins, double *stats, int64_t *hist, double *device_ms);
int32_t hjb_rollout_campaign_hist_reduce(int64_t n_starts, int64_t n_samples, const double *cost, const double *lo, const double *hi,
                                         int32_t n_bins, int64_t *hist);

/* ---- paired campaigns: per-start statistics of the cost difference of two controllers, reduced on the device (kernel K31) -------
 * hjb_rollout_run_campaign_pair flies one object's plant - its affine model and the node set of hjb_rollout_set_noise - under two
 * controllers A and B.  Both controllers fly every sample on the plain campaigns' stream: sample m of start s flies stream
 * first_stream + s*M + m under A and under B, so the variance of the per-sample difference holds the pairing (the covariance) that
 * two independently reduced records do not.  No array of the call has a dimension of n_starts * M.
 * Each controller is one of three kinds:
 *   HJB_PAIR_LABELS (0)     the stored-label controller of hjb_rollout_run_campaign; planes_x are label planes, method_x is read;
 *   HJB_PAIR_LOOKAHEAD (1)  the controller of hjb_rollout_run_lookahead_campaign, under the object's hjb_rollout_set_lookahead set;
 *                           planes_x are value planes (-1: the zero function), method_x is ignored;
 *   HJB_PAIR_GREEDY (2)     the same with a lookahead set of ONE zero node of weight 1, mode expect: K26's nominal controller; it is
 *                           bit for bit what hjb_rollout_run_lookahead_campaign gives after hjb_rollout_set_lookahead(zeros(D,1),
 *                           [1.0], expect).  The object's own lookahead set is neither read nor changed: the host keeps that
 *                           one-node table on the device itself.
 * Both sides may have the same kind with different planes or method (per-stage labels against the stationary table; 'nearest'
 * against 'linear'); a pair of a controller with itself is legal.
 * Output.  stats_a [8, n_starts]: bit for bit the plain campaign of A with the same arguments, threshold and tol included;
 *   stats_b [8, n_starts]: the same for B;  stats_d [HJB_CAMPAIGN_PAIR_NSTAT, n_starts] column-major: the record of d = c_B - c_A,
 *   one rounded subtraction per sample.  A negative d means B paid less.
 * Slot values of d.  campaign_slot(d, t) with the flags  e = d < 0;  l = d > 0;  t = neither flight left the grid.  A NaN d sets
 *   neither e nor l.  Padding, G, blocks, the adjacent-pair tree and the left-to-right fold are hjb_rollout_run_campaign's, word
 *   for word (csrc/hjbdp_campaign.h: CampVals, campaign_op, campaign_tree - there is no second reduction).
 *   stats_d: 0 sum d;  1 sum d*d, each product rounded;  2 min d;  3 max d;  4 n(B lower);  5 n(A lower);  6 n(both stayed in the
 *   grid);  7 sum d over those samples.  Counts are exact integers stored as doubles.  There are no atomics anywhere in this call.
 * Options "chunk" and "lds" change no bit of any of the three records.
 * Device memory of a call: [D + 1 + 24, n_starts] doubles, 24 doubles per block of a launch, and one double and one byte per lane
 *   of a launch (the pair scratch through which A's kernel hands its costs and flags to B's).
 * hjb_rollout_campaign_pair_reduce is the CPU twin with no device (csrc/hjbdp_campaign.h, campaign_pair_start), on per-trajectory
 *   arrays such as hjb_rollout_run_noisy and hjb_rollout_run_lookahead return: trajectory s*M + m is sample m of start s; cost_a,
 *   cost_b [n_starts*M]; left_a, left_b [n_starts*M] uint8 (non-zero: left the grid), a NULL left_* means "none left".
 * Refused before any device work, outputs untouched (text: hjb_rollout_last_error) - HJB_E_INVALID: a kind outside 0..2;
 * everything the plain campaign of each kind refuses, named with the side in the text ("A:" / "B:"); a null stats_a, stats_b or
 * stats_d with n_starts > 0; the plain campaigns' refusals of sizes, streams, threshold and tol.  n_starts = 0 is HJB_OK.
 * Out of scope: a histogram of d, pairs across two objects, pairs on the integrated plants. */
#define HJB_PAIR_LABELS 0
#define HJB_PAIR_LOOKAHEAD 1
#define HJB_PAIR_GREEDY 2
#define HJB_CAMPAIGN_PAIR_NSTAT 8
int32_t hjb_rollout_run_campaign_pair(void *rollout, int32_t kind_a, int32_t method_a, const int32_t *planes_a, int32_t kind_b,
                                      int32_t method_b, const int32_t *planes_b, int32_t n_steps, int64_t n_starts, int64_t n_samples,
                                      const double *X0, uint64_t seed, int64_t first_stream, const double *threshold, const double *tol,
                                      double *stats_a, double *stats_b, double *stats_d, double *device_ms);
int32_t hjb_rollout_campaign_pair_reduce(int64_t n_starts, int64_t n_samples, const double *cost_a, const double *cost_b,
                                         const uint8_t *left_a, const uint8_t *left_b, double *stats_d);

/* The 6-D attitude closed loop (attitude-control/Solver_attitude.m:744-833, get_optimal_path after run) on the same object.
 * hjb_rollout_set_attitude_model and hjb_rollout_set_model replace each other: the last one set wins.  It needs D == 6, n_u == 3
 * and the grid axes in the reference's order (w1, w2, w3, yaw, pitch, roll); inertia = [J1 J2 J3] and h finite and > 0,
 * integrator HJB_ATT_TAYLOR / _RK4, q [7] and r [3] finite (NULL = zeros).  hjb_rollout_run_attitude steps the 7-state
 * X = [w1 w2 w3 q1 q2 q3 q4] (q4 scalar), all in double, left to right, every product rounded; step k, p = plane_of_step[k]:
 *   yaw = atan2c(2*(X6*X5 + X7*X4), ((X7*X7 + X6*X6) - X5*X5) - X4*X4),  pitch = asinc(clamp(-2*(X6*X4 - X7*X5), -1, 1)),
 *   roll = atan2c(2*(X5*X4 + X7*X6), ((X7*X7 - X6*X6) - X5*X5) + X4*X4)   (fdlibm's forms in + - * / sqrt only: <= 2 ulp of libm, tested);
 *   u = the policy lookup of plane p at (X1, X2, X3, yaw, pitch, roll), as in hjb_rollout_run;
 *   cost += ((q1*(X1*X1) + q2*(X2*X2)) + ... + q7*(X7*X7)) + r1*(u1*u1) + r2*(u2*u2) + r3*(u3*u3);
 *   X+ = X + h f(X, u) (taylor) or classical RK4 with u held over the step, f the rigid body with diagonal inertia and the
 *   quaternion kinematics (:600-620); then X4..X7 are divided by sqrt(((X4*X4 + X5*X5) + X6*X6) + X7*X7).
 * X0, X_final [7, n_traj]; cost [n_traj]; X_path [n_traj, 7, n_steps+1]; U_path [n_traj, 3, n_steps]; A_path [n_traj, 3, n_steps]
 * (the yaw, pitch, roll in radians that step k looked up at).  Every output but X_final may be NULL.  An X0 column whose
 * quaternion is all zeros is HJB_E_INVALID; so are hjb_rollout_run on an attitude object and hjb_rollout_run_attitude on an
 * affine one. */
#define HJB_ATT_TAYLOR 0   /* X+ = X + h f(X,u)                  (Solver_attitude.m:688, used by get_optimal_path :778) */
#define HJB_ATT_RK4 1      /* classical RK4, u held over the step (:679-686, next_stage_states' default) */
int32_t hjb_rollout_set_attitude_model(void *rollout, const double *inertia, double h, int32_t integrator, const double *q,
                                       const double *r);
int32_t hjb_rollout_run_attitude(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                 const double *X0, double *X_final, double *cost, double *X_path, double *U_path, double *A_path,
                                 double *device_ms);

/* The 13-state pos-att closed loop (pos-att/Solver_pos_att.m:452-730, get_optimal_path after simplified_run) on three rollout
 * objects, one per channel (x, y, z), each D == 4 over (position, velocity, angle, rate) with n_u == 4 thruster levels per label
 * (f0 f1 f6 f7 / f2 f3 f8 f9 / f4 f5 f10 f11), on one device, in one label type.  hjb_rollout_set_pos_att_model attaches the model
 * to rollout_x (it replaces, and is replaced by, the other two models: the last one set wins) and takes a share of rollout_y's
 * and rollout_z's device data as they are at the call: destroying those two afterwards is SAFE, rollout_x keeps what it reads
 * alive until it is destroyed or given another model; they stay ordinary objects.  inertia [3, 3] and rsw2eci [3, 3] (RSW2ECI of
 * the target's R0, V0, :831-847) column-major, finite, determinant not 0; mass, h finite and > 0; t_dist finite; substeps >= 1;
 * orbit_coef [5, n_nodes] column-major, finite, n_nodes == 2 * substeps * k + 1: node j holds, at t = j * h / (2 * substeps),
 *   2mu/|R|^3 + H^2/|R|^4,  2 (R.V) H/|R|^4,  2H/|R|^2,  mu/|R|^3 - H^2/|R|^4,  mu/|R|^3     (R, V the target's state, H = |R x V|):
 * all the right-hand side (:705-727) needs of the orbit.  hjb_rollout_run_pos_att steps X = [x(3) v(3) q(4) w(3)] (q4 scalar)
 * n_steps <= (n_nodes - 1) / (2 * substeps) stages, all in double, left to right, every product rounded; stage k:
 *   t_i = 2 * asinc(clamp(X[6+i], -1, 1));  xb = (ECI2body(q) * rsw2eci) x,  vb likewise (:411-415);
 *   the 'nearest' lookups of plane plane_of_step[k]: channel x at (xb0, vb0, t_y, w_y), y at (xb1, vb1, t_z, w_z), z at
 *   (xb2, vb2, t_x, w_x) (:434-447); U_M and a = rsw2eci^-1 (ECI2body(q)^-1 a_body) (:804-823), each inverse the adjugate over
 *   the determinant (q is not renormalised, as in the reference, so ECI2body(q) is only nearly orthogonal);
 *   `substeps` classical RK4 steps of h / substeps with a and U_M held, w_dot = inertia^-1 (U_M - w x (inertia w)).
 * X0, X_final [13, n_traj]; X_path [n_traj, 13, n_steps+1]; F_path [n_traj, 12, n_steps] (f0..f11); FM_path [n_traj, 6, n_steps]
 * (a_x a_y a_z U_M, :502); NULL paths are not written.  plane_of_step indexes the planes of all three channels.  A non-finite
 * X0 is HJB_E_INVALID; a state that leaves the grids or stops being finite during the run is looked up at the clamped cell
 * (NaN: cell 0) and the run completes.  hjb_rollout_run / hjb_rollout_run_attitude on a pos-att object, and
 * hjb_rollout_run_pos_att on any other, are HJB_E_INVALID. */
int32_t hjb_rollout_set_pos_att_model(void *rollout_x, void *rollout_y, void *rollout_z, const double *inertia, double mass,
                                      double t_dist, double h, int32_t substeps, const double *rsw2eci, int32_t n_nodes,
                                      const double *orbit_coef);
int32_t hjb_rollout_run_pos_att(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj, const double *X0,
                                double *X_final, double *X_path, double *F_path, double *FM_path);

/* Thruster-fault campaigns in the pos-att loop (K23): the loop above with a dead thruster in the plant and a hand-over to the fault
 * controller of channel x (pos-att/Solver_pos_att.m:235-240, channel_x_controller_1_failure), both per trajectory, and two scalars
 * per trajectory beside X_final.  hjb_rollout_set_pos_att_fault_controller attaches rollout_xf (an ordinary object, D == 4,
 * n_u == 4 = f0 f1 f6 f7, rollout_x's device and label type, a grid of its own) to the pos-att model rollout_x holds (without
 * one: HJB_E_INVALID, call hjb_rollout_set_pos_att_model first) and takes a share of its device data, as the model does of y's
 * and z's: destroying rollout_xf afterwards is SAFE.  rollout_xf NULL detaches.  Setting the pos-att model again, or another
 * model, drops the attachment; hjb_rollout_run_pos_att ignores it and stays bit for bit what it is.
 * hjb_rollout_run_pos_att_faults, trajectory i at stage k: channel x is looked up in the fault controller when
 * switch_stage[i] <= k, else in rollout_x (one lookup, on plane plane_of_step[k] like y and z); the commanded forces f0..f11 as
 * in hjb_rollout_run_pos_att; the APPLIED forces fa_j = (fault_stage[i] <= k and bit j of fault_mask[i]) ? +0.0 : f_j; U_M, a
 * and the RK4 sub-steps are hjb_rollout_run_pos_att's operations on fa.  F_path holds fa (what the plant got), FM_path is
 * formed from fa.  With no fault and no hand-over X_final and the paths are hjb_rollout_run_pos_att's, bit for bit.
 *   impulse[i] = (sum over the stages, in stage order, of ((((|fa0| + |fa1|) + |fa2|) + ...) + |fa11|)) * h, h as given to
 *     hjb_rollout_set_pos_att_model;
 *   settle_stage[i]: with X_0 = X0 and X_k+1 the state after stage k, X_m is inside when ((x0^2 + x1^2) + x2^2) <= pos_tol^2 and
 *     ((q1^2 + q2^2) + q3^2) <= att_tol^2 (a NaN state is not inside); the smallest s such that X_m is inside for every m in
 *     [s, n_steps], n_steps + 1 when X_n_steps is outside.
 * fault_mask, fault_stage, switch_stage [n_traj] int32, each may be NULL: no fault / stage 0 / never.  A stage >= n_steps never
 * comes.  impulse [n_traj], settle_stage [n_traj], the paths (laid out as hjb_rollout_run_pos_att's) and device_ms (the kernels'
 * time by HIP events) may be NULL.  HJB_E_INVALID, decided before any device work and with the outputs untouched: a mask bit
 * above 11, a negative stage, a switch_stage[i] < n_steps with no fault controller attached, a tolerance that is NaN or negative
 * (+Inf is allowed), a non-finite X0, plane_of_step outside the planes of any of the four objects, and hjb_rollout_run_pos_att's
 * own refusals.  Option "lds" and the 32 KiB rule cover the four controllers' tables together; option "chunk" as everywhere. */
int32_t hjb_rollout_set_pos_att_fault_controller(void *rollout_x, void *rollout_xf);
int32_t hjb_rollout_run_pos_att_faults(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                       const double *X0, const int32_t *fault_mask, const int32_t *fault_stage,
                                       const int32_t *switch_stage, double pos_tol, double att_tol, double *X_final, double *impulse,
                                       int32_t *settle_stage, double *X_path, double *F_path, double *FM_path, double *device_ms);

/* Solver_position's closed loop (position-control/Solver_position.m:189-311, get_optimal_path after simplified_run) on three rollout
 * objects, one per channel (x, y, z), each D == 2 over (position, velocity) with n_u == 1 (the acceleration per label), on one device,
 * in one label type.  Sharing and lifetime are those of the pos-att model: hjb_rollout_set_position_model attaches the model to
 * rollout_x (the last model set wins) and takes a share of rollout_y's and rollout_z's device data, so destroying those two
 * afterwards is safe.  The stage integrator is private/rkf45.m ON ITS SCHEDULE: at the reference's h = 0.005 s every error test
 * passes with room to spare, every step is accepted and grows fourfold, and the steps depend on the stage's t0 and tf alone.  The
 * host lists them: n_sub [n_steps] sub-steps per stage, 1 <= n_sub[k] <= max_sub <= 8, and table [32, max_sub, n_steps] column-major,
 * finite, row (s, k) = [h_form, h_apply, then at each of the six times t_s + a_j h_form (a = 0, 1/4, 3/8, 12/13, 1, 1/2) the five
 * orbit scalars of hjb_rollout_set_pos_att_model's orbit_coef]; tol finite and > 0 (rkf45's 1e-8).  hjb_rollout_run_position
 * steps y = [x(3) v(3)] n_steps <= the table's stages, all in double, left to right, every product rounded; stage k:
 *   a_i = the 'nearest' lookup of channel i on plane plane_of_step[k] at (y_i, y_3+i), held over the stage (:215-217);
 *   per sub-step, with B, C4, C5 Fehlberg's tableau and F the right-hand side f_0..2 = y_3..5,
 *   f_3 = ((c0 y0 - c1 y1) + c2 y4) + a_0, f_4 = ((c1 y0 - c3 y1) - c2 y3) + a_1, f_5 = a_2 - c4 y2:
 *     f_0 = F(y), f_i = F((..(y + (h_form B_i0) f_0) + ..) + (h_form B_i,i-1) f_i-1);
 *     te = max_i |h_form ((((f_0i d_0 + f_2i d_2) + f_3i d_3) + f_4i d_4) + f_5i d_5)|, d = C4 - C5;
 *     allowed = tol * max(max_i |y_i|, 1);  the sub-step is on schedule iff allowed >= 1100 * (te + 2^-52) (false for NaN): rkf45
 *     grows the step fourfold when allowed / (te + eps) >= 1024, and 1100 leaves room for the rounding of its pow(., 0.2);
 *     y_i += h_apply ((((f_0i C5_0 + f_2i C5_2) + f_3i C5_3) + f_4i C5_4) + f_5i C5_5)   (h_apply < h_form in a stage's last
 *     sub-step: rkf45 clips an accepted step after forming its stage derivatives, and so does this).
 * off_schedule [n_traj] (required): the first stage with a sub-step off schedule, -1 if none; such a trajectory is NOT what rkf45
 * computes from that stage on and is for the caller to recompute; the run completes on the schedule either way.  X0, X_final
 * [6, n_traj]; X_path [n_traj, 6, n_steps+1]; A_path [n_traj, 3, n_steps]; NULL paths are not written.  A non-finite X0 is
 * HJB_E_INVALID; a state that leaves the grids is looked up at the clamped cell (the reference's default start does).  The other
 * hjb_rollout_run_* calls on a position object, and hjb_rollout_run_position on any other, are HJB_E_INVALID. */
int32_t hjb_rollout_set_position_model(void *rollout_x, void *rollout_y, void *rollout_z, double tol, int32_t n_steps, int32_t max_sub,
                                       const int32_t *n_sub, const double *table);
int32_t hjb_rollout_run_position(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj, const double *X0,
                                 double *X_final, double *X_path, double *A_path, int32_t *off_schedule);

/* The simplified attitude closed loop (attitude-control/Solver_attitude.m:835-925, get_optimal_path_simplified_testode45 after
 * simplified_run; attitude-control/test/test_simplified.m:188-218) on three rollout objects, one per channel, each D == 2 over
 * (w_i, theta_i) with n_u == 1 (the torque per label), on one device, in one label type.  Sharing and lifetime are those of the
 * pos-att and position models: hjb_rollout_set_attitude_simplified_model attaches the model to rollout_1 (the last model set wins)
 * and takes a share of rollout_2's and rollout_3's device data, so destroying those two afterwards is safe.  inertia [3, 3]
 * column-major, finite, non-singular; h finite and > 0; substeps >= 1; qw, qt, r [3] finite (NULL = zeros).
 * hjb_rollout_run_attitude_simplified steps X = [w1 w2 w3 q1 q2 q3 q4] (q4 scalar), all in double, left to right, every product
 * rounded; stage k, p = plane_of_step[k]:
 *   t_i = 2 asin(clamp(X[3+i], -1, 1)) (the library's fixed asin, <= 2 ulp of libm; the clamp is ours);
 *   u_i = the 'nearest' lookup of channel i on plane p at (X[i], t_i), i = 0, 1, 2, held over the stage;
 *   g_i = (qw_i (X[i] X[i]) + qt_i (t_i t_i)) + r_i (u_i u_i);  cost += (g_0 + g_1) + g_2   (the 2-D sweeps' stage cost, :220);
 *   HJB_ATTS_FULL: `substeps` classical RK4 steps of h / substeps of w_dot = inertia^-1 (u - w x (inertia w)) (the inverse is the
 *     adjugate over the determinant, formed once) and the quaternion kinematics (:902-922), quaternion NOT renormalised.  This
 *     stands in for the reference's ode45: on the solver's default grids it differs from a Dormand-Prince 5(4) stage integrator
 *     (rtol 1e-3, atol 1e-6) by RK4's truncation error, max |dX| 4.9e-13 over 5,999 stages at substeps 1 and 1.4e-14 at 2
 *     (tests/test_rollout_attitude_simplified_abi.py), with every torque equal;
 *   HJB_ATTS_DIAGONAL: the attitude model's RK4 step (hjb_rollout_set_attitude_model, HJB_ATT_RK4) at (J1, J2, J3) =
 *     diag(inertia) > 0, ONE step of h, then q / |q| (test_simplified.m:195-217, :317-356); substeps must be 1.
 * X0, X_final [7, n_traj]; cost [n_traj]; X_path [n_traj, 7, n_steps+1]; U_path, A_path [n_traj, 3, n_steps] (A_path: the three
 * t_i the stage looked up at); every output but X_final may be NULL.  A non-finite X0 is HJB_E_INVALID; a state that leaves the
 * grids or stops being finite is looked up at the clamped cell (NaN: cell 0) and the run completes.  The other hjb_rollout_run_*
 * calls on such an object, and hjb_rollout_run_attitude_simplified on any other, are HJB_E_INVALID. */
#define HJB_ATTS_FULL 0      /* full inertia matrix, RK4 sub-steps, no renormalisation (Solver_attitude.m:835-925) */
#define HJB_ATTS_DIAGONAL 1  /* diagonal inertia, one RK4 step, q / |q| (test_simplified.m:195-217) */
int32_t hjb_rollout_set_attitude_simplified_model(void *rollout_1, void *rollout_2, void *rollout_3, const double *inertia, double h,
                                                  int32_t substeps, int32_t dynamics, const double *qw, const double *qt,
                                                  const double *r);
int32_t hjb_rollout_run_attitude_simplified(void *rollout_1, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                            const double *X0, double *X_final, double *cost, double *X_path, double *U_path,
                                            double *A_path);

/* The linear attitude controller's closed loop (attitude-control/Solver_attitude.m:508-591, linear_control_response: the PD law
 * U = -K qe(1:3) - C w the DP controllers are judged against) for many initial attitudes at once.  Stateless: there is no policy,
 * so no object; the plant is the attitude model's (hjb_rollout_set_attitude_model: inertia = [J1 J2 J3], h, HJB_ATT_TAYLOR /
 * HJB_ATT_RK4, then q / |q|), which with HJB_ATT_RK4 is next_stage_states(., 'RK4') operation for operation.  K, C [3, 3] and
 * qc [4, 4] (NULL = identity) column-major; u_limit [3] >= 0 (NULL = none); weights [10] (NULL = zeros).  All in double, left to
 * right, every product rounded; step k, X = [w1 w2 w3 q1 q2 q3 q4] (q4 scalar):
 *   qe_i = ((qc[i,0]*X4 + qc[i,1]*X5) + qc[i,2]*X6) + qc[i,3]*X7, i = 0, 1, 2 (:536; row 3 of qc is not used by the law);
 *   u_i = (-((K[i,0]*qe_0 + K[i,1]*qe_1) + K[i,2]*qe_2)) - ((C[i,0]*X1 + C[i,1]*X2) + C[i,2]*X3)   (:538);
 *   with u_limit: u_i = u_i > L_i ? L_i : u_i < -L_i ? -L_i : u_i (a NaN passes through);
 *   A_path[., k] = (yaw, pitch, roll) of X as hjb_rollout_run_attitude forms them (:540);
 *   HJB_ATTL_COST_QUAT, weights = q[7] then r[3]: hjb_rollout_run_attitude's stage cost;
 *   HJB_ATTL_COST_ANGLE, weights = qw[3], qt[3], r[3], one unused: hjb_rollout_run_attitude_simplified's, t_i = 2 asin(clamp(X[3+i], -1, 1));
 *   X+ = the attitude model's step with u held, then X4..X7 / sqrt(((X4*X4 + X5*X5) + X6*X6) + X7*X7).
 * X0, X_final [7, n_traj]; cost [n_traj]; X_path [n_traj, 7, n_steps+1]; U_path, A_path [n_traj, 3, n_steps]; every output but
 * X_final may be NULL.  chunk: trajectories per launch (0 = 1 << 20, at most 1 << 30); device_ms (may be NULL): the launches'
 * event times summed.  HJB_E_INVALID, with a text in hjb_rollout_last_error(NULL), decided before any device work: a null inertia,
 * K, C, X0 or X_final; inertia or h not finite and > 0; an unknown integrator or cost_form; a non-finite entry of K, C, qc,
 * u_limit, weights or X0; a negative limit; an X0 column whose quaternion is all zeros; n_steps < 0; n_traj < 0; chunk outside
 * 0 .. 1 << 30; a negative device; size overflow.  n_traj == 0 is HJB_OK without touching a device; after the checks, no device
 * visible is HJB_E_DEVICE. */
#define HJB_ATTL_COST_QUAT 0    /* weights = q[7] then r[3]:           hjb_rollout_run_attitude's stage cost */
#define HJB_ATTL_COST_ANGLE 1   /* weights = qw[3], qt[3], r[3], one unused: hjb_rollout_run_attitude_simplified's */
int32_t hjb_attitude_linear_response(int32_t device, const double *inertia, double h, int32_t integrator, const double *K,
                                     const double *C, const double *qc, const double *u_limit, int32_t cost_form,
                                     const double *weights, int32_t n_steps, int64_t n_traj, const double *X0, double *X_final,
                                     double *cost, double *X_path, double *U_path, double *A_path, int64_t chunk, double *device_ms);

/* ---- flat builder API -------------------------------------------------------------------------------------------
 * hjb_problem holds arrays of structs with pointers, which MATLAB's loadlibrary/calllib cannot marshal.  These entry
 * points take primitives and plain arrays only, copy what they are given (the caller may free it at once), and end in
 * hjb_create_from, after which the handle is used exactly like one from hjb_create.  They replace, for a MATLAB host,
 * the table building of the reference's run methods (test/Dynamic_Solver.m:66-84: grid vectors, a_D_M, g_D):
 *   hjb_problem_new(D, C, n, m, dtype, index_base, &b)
 *   hjb_problem_set_knots(b, axis, knots, len)                      once per state axis
 *   hjb_problem_add_next_term(b, axis, mask, data, count)           in MATLAB's left-to-right order of the sum
 *   hjb_problem_add_cost_term(b, mask, data, count)
 *   [hjb_problem_set_types(b, idx_dtype, table_dtype)]              right after hjb_problem_new
 *   [hjb_problem_set_slab(b, begin, end, halo_lo, halo_hi)]  [hjb_problem_set_model(b, model, h, t0, t1, t2, t3)]
 *   hjb_create_from(b, device, &h);  hjb_problem_free(b)
 * data: `count` elements of the problem dtype (float for HJB_F32 / HJB_F16S, double for HJB_F64), column-major over
 * the masked grid dims; count must equal the product of their sizes. */
typedef struct hjb_builder_s *hjb_builder;
int32_t hjb_problem_new(int32_t D, int32_t C, const int32_t *n, const int32_t *m, int32_t dtype, int32_t index_base,
                        hjb_builder *out);
int32_t hjb_problem_set_knots(hjb_builder b, int32_t axis, const double *knots, int32_t len);
int32_t hjb_problem_add_next_term(hjb_builder b, int32_t axis, uint32_t mask, const void *data, int64_t count);
int32_t hjb_problem_add_cost_term(hjb_builder b, uint32_t mask, const void *data, int64_t count);
int32_t hjb_problem_set_slab(hjb_builder b, int32_t slab_begin, int32_t slab_end, int32_t halo_lo, int32_t halo_hi);
/* hjb_problem.idx_dtype (HJB_IDX_*) and hjb_problem.table_dtype (HJB_TAB_*).  Call it right after hjb_problem_new:
 * with HJB_TAB_F64 the `data` of every hjb_problem_add_next_term that follows is float64 (cost terms stay float). */
int32_t hjb_problem_set_types(hjb_builder b, int32_t idx_dtype, int32_t table_dtype);
/* hjb_problem.cost_dtype (HJB_COST_*): call it before the first hjb_problem_add_cost_term - under HJB_COST_F64 the cost
 * terms' data are float64 */
int32_t hjb_problem_set_cost_type(hjb_builder b, int32_t cost_dtype);
int32_t hjb_problem_set_model(hjb_builder b, int32_t model, double model_h, const void *t0, const void *t1,
                              const void *t2, const void *t3);
/* Relabel the state axes of a problem under construction: new axis i = old axis order[i] (terms over several state
 * dims are transposed).  Which axis is last decides which stage kernel applies and which axis a multi-GPU run shards;
 * the caller permutes its own arrays the same way (MATLAB: permute(J, order + 1) in, ipermute out).  Before
 * hjb_problem_set_slab; not for problems with a state model. */
int32_t hjb_problem_permute_axes(hjb_builder b, const int32_t *order);
/* A labelling under which a faster stage kernel applies, from the terms' masks (and, for D = 4 with one control dim, the
 * control terms' ranges): order_out[D], *found = 1 when it differs from the present labelling (else the identity, 0).
 * D = 4, C = 1: the column-sweep kernel's shape (Solver_pos_att.m:299-328: the two axes the thrusters do not drive
 * first, of the other two the less-moved one last; 120^4 x 9: 1.8 ms per stage against 6.7 ms in the reference's own
 * order (x, v, theta, w)).  Otherwise: the axes no control drives first, then the driven ones in the order of the
 * control dims (Solver_attitude.m's (w1, w2, w3, yaw, pitch, roll) -> (yaw, pitch, roll, w1, w2, w3): 4.4 ms against
 * 28 ms on the reference grid). */
int32_t hjb_problem_suggest_order(hjb_builder b, int32_t *order_out, int32_t *found);
int32_t hjb_create_from(hjb_builder b, int32_t device, hjb_handle *out);
int32_t hjb_problem_free(hjb_builder b);
/* text of the last error of a builder call (b may be NULL) */
const char *hjb_problem_last_error(hjb_builder b);

/* hjb_solve without structs: every argument a scalar or a plain array (NULL where hjb_solve_opts allows NULL);
 * the three result scalars may be NULL.  No progress callback, no probe. */
int32_t hjb_solve_flat(hjb_handle h, int32_t n_stages, int32_t monitor_period, double monitor_tol, const void *terminal,
                       void *J_final, void *idx_final, void *J_stages, void *idx_stages, int32_t *stages_done,
                       int32_t *stopped_early, double *sweep_ms);
/* hjb_get_info without the struct: out[0..7] = n_states, n_controls, j_elems, kernel_variant, lds_bytes, grid,
 * halo_needed_lo, halo_needed_hi */
int32_t hjb_get_info_flat(hjb_handle h, int64_t *out8);

/* ---- single-process multi-GPU sweep -------------------------------------------------------------------------------
 * For a host that is ONE process (MATLAB): the stage loop of the reference (pos-att/Solver_pos_att.m:270-286,
 * position-control/Solver_position.m:132-141) over a grid partitioned along its LAST state axis, slab i on device
 * devices[i].  Per stage each slab gets the halo planes of J_{k+1} from its neighbours (hipMemcpyPeerAsync, xGMI), runs
 * the interior planes while the copies are in flight and the two boundary strips after them; the early-stop monitor's
 * sums are added over the slabs.  Choose WHICH axis is last by relabelling the state axes (the axis should move less
 * than a slab per stage: pos-att shards x, v or theta, not w).  hjb_solve_opts: terminal / J_final / idx_final are
 * whole-grid host arrays, as are J_stages / idx_stages (copied out slab by slab behind each stage); probe is not
 * supported.  The same device may be listed more than
 * once (several slabs on one GPU: testing).  One process per GPU with torch.distributed/RCCL is the other supported
 * form (hjbdp/sharded.py, bench.py --gpus N). */
typedef struct hjb_multi_s *hjb_multi;
int32_t hjb_create_multi(const hjb_problem *problem, int32_t n_dev, const int32_t *devices, hjb_multi *out);
int32_t hjb_create_multi_from(hjb_builder b, int32_t n_dev, const int32_t *devices, hjb_multi *out);
int32_t hjb_solve_multi(hjb_multi m, const hjb_solve_opts *opts, hjb_result *result);
int32_t hjb_solve_multi_flat(hjb_multi m, int32_t n_stages, int32_t monitor_period, double monitor_tol, const void *terminal,
                             void *J_final, void *idx_final, int32_t *stages_done, int32_t *stopped_early, double *sweep_ms);
/* planes [begin, end) of slab `slab`, its halo, whether it runs as interior + strips, its stage kernel (any out may be NULL) */
int32_t hjb_multi_slab_info(hjb_multi m, int32_t slab, int32_t *begin, int32_t *end, int32_t *halo_lo, int32_t *halo_hi,
                            int32_t *split, int32_t *kernel_variant);
int32_t hjb_multi_set_option(hjb_multi m, const char *key, int64_t value);   /* hjb_set_option on every slab handle */
int32_t hjb_destroy_multi(hjb_multi m);
const char *hjb_multi_last_error(hjb_multi m);

/* ---- one process per GPU: a rank's share of the sweep ----------------------------------------------------------------
 * For hosts that run one process per GPU and move the halo planes themselves (MPI; RCCL through torch.distributed:
 * hjbdp/sharded.py, bench.py --gpus N).  hjb_rank_create partitions the LAST state axis over `world` ranks exactly as
 * hjb_create_multi does over devices and builds this rank's handles: the slab, and - with `overlap` and an interior -
 * the interior and the two boundary strips over the same buffers.  The caller owns two J buffers of
 * (end - begin + halo_lo + halo_hi) planes and a label buffer of (end - begin) planes on `device`, and per stage
 *   1. makes its transfer stream wait for the compute stream, enqueues the halo exchange of dJ_in on it
 *      (send my boundary planes, receive into planes [0, halo_lo) and [halo_lo + owned, ...)),
 *   2. calls hjb_rank_stage(r, dJ_in, dJ_out, d_idx, compute_stream, halo_stream): ONE call enqueues the interior on
 *      compute_stream, the strips on the library's own streams behind an event recorded on halo_stream at this point,
 *      and joins them into compute_stream (halo_stream NULL: nothing to wait for).
 * hjb_rank_info: out10 = begin, end, halo_lo, halo_hi, split (1: interior + strips), kernel variant, halo_needed_lo,
 * halo_needed_hi, bytes per label, planes of the last axis. */
typedef struct hjb_rank_s *hjb_rank;
int32_t hjb_rank_create(const hjb_problem *problem, int32_t device, int32_t rank, int32_t world, int32_t overlap, hjb_rank *out);
/* the same from a flat builder (include/hjbdp_matlab.h: a MATLAB worker per GPU binds this one) */
int32_t hjb_rank_create_from(hjb_builder b, int32_t device, int32_t rank, int32_t world, int32_t overlap, hjb_rank *out);
int32_t hjb_rank_info(hjb_rank r, int32_t *out10);
int32_t hjb_rank_stage(hjb_rank r, const void *dJ_in, void *dJ_out, void *d_idx, void *compute_stream, void *halo_stream);
/* The stage with the boundary strips enqueued FIRST, behind what halo_stream holds (the previous exchange), and
 * hjb_rank_wait_strips: `stream` waits for that stage's strips (*covered = 1 when they cover every plane a neighbour needs;
 * 0: nothing is enqueued, the caller's exchange waits for the compute stream).  The pieces of hjb_rank_step_post (below) for a
 * host that moves the halo planes itself: exchange dJ_out's boundary planes behind the strips, under the rest of the interior. */
int32_t hjb_rank_stage_post(hjb_rank r, const void *dJ_in, void *dJ_out, void *d_idx, void *compute_stream, void *halo_stream);
int32_t hjb_rank_wait_strips(hjb_rank r, void *stream, int32_t *covered);
int32_t hjb_rank_set_option(hjb_rank r, const char *key, int64_t value);
int32_t hjb_rank_get_option(hjb_rank r, const char *key, int64_t *value);
int32_t hjb_rank_check_status(hjb_rank r, void *stream);
/* dJ (this rank's haloed buffer) = the separable function of hjb_device_fill_separable on the rank's planes, halo planes included:
 * vecs[a] are the GLOBAL host vectors (n[a] elements each).  A terminal cost for grids that never exist in host memory. */
int32_t hjb_rank_fill_separable(hjb_rank r, const void *const *vecs, void *dJ, void *stream);
int32_t hjb_rank_destroy(hjb_rank r);
const char *hjb_rank_last_error(hjb_rank r);

/* ---- RCCL inside the library: a rank's halo exchange and monitor all-reduce without torch or MPI -------------------------
 * per stage ncclGroupStart; ncclSend / ncclRecv x <= 4; ncclGroupEnd on a transfer stream (one xGMI link
 * per neighbour pair), every monitor period a 2-double ncclAllReduce.  librccl.so.1 is dlopen'ed on first use (override:
 * $HJBDP_RCCL_LIB); libhjbdp has no link dependency on it.  The host's part: rank 0 calls hjb_rank_comm_unique_id and hands
 * the 128 bytes to every rank by any means (a file, a socket, MATLAB's labSend); every rank calls hjb_rank_comm_init
 * (collective), then either hjb_rank_sweep (the whole `for k_s` loop incl. the monitor of Solver_pos_att.m:268-285) or,
 * stage by stage, hjb_rank_step = hjb_rank_exchange (transfer stream, behind the compute stream) + hjb_rank_stage with the
 * boundary strips waiting for the halos.  hjb_rank_monitor_sums: sum J and sum of labels over the WHOLE grid on every rank.
 * Option "comm_loopback" (hjb_rank_set_option before hjb_rank_comm_init; one-GPU transport test): a communicator of one
 * rank whose two neighbours are itself - the planes it sends down arrive in its own upper halo, those it sends up in its
 * lower halo - so the RCCL calls, pointers, counts and stream ordering run on a box with a single GPU.  Option
 * "xfer_delay_us" (emulation only, tools/emulate_ranks.py): a spin of that many microseconds on the transfer stream behind
 * every exchange, standing in for link latency the one-GPU loopback does not have.
 * Option "monitor_single" (the reference's typing, Solver_pos_att.m:276-282): hjb_rank_sweep forms `e = fsum50 - fsum50_prev`
 * and `abs(e) < tol` in single precision, as hjb_solve does.  The SUM itself: at world == 1 the library's stated float32
 * tree (= hjb_solve's, bit for bit); over several ranks each rank's planes are summed in float64 over a fixed tree and
 * the all-reduce adds the ranks in its own order - reproducible for one world size, NOT bit-identical to the one-device
 * sum, so a stop decision within rounding of `tol` can fall one monitor period apart.
 * A host without librccl: hjb_rank_comm_unique_id / hjb_rank_comm_init return HJB_E_UNSUPPORTED with the loader's message.
 * tools/bench_ranks.cpp is a C++ driver on these calls (one process per GPU, no Python).
 * hjb_rank_comm_available: HJB_OK when the library can reach RCCL (loads it on first use, nothing else - no communicator, no
 * bootstrap thread), else HJB_E_UNSUPPORTED with the loader's message in hjb_rank_last_error(NULL): what EVERY rank asks before
 * the collective hjb_rank_comm_init, so that the ranks can agree to use another transport instead of one of them failing alone. */
int32_t hjb_rank_comm_available(void);
int32_t hjb_rank_comm_unique_id(void *id128_out);
int32_t hjb_rank_comm_init(hjb_rank r, const void *id128);
/* what the communicator itself reports (ncclCommCount / ncclCommUserRank; -1 where librccl lacks the query): lets a run
 * verify that the ranks it timed were ranks of ONE communicator of the expected size */
int32_t hjb_rank_comm_info(hjb_rank r, int32_t *n_ranks, int32_t *comm_rank);
int32_t hjb_rank_exchange(hjb_rank r, void *dJ, void *compute_stream);
void *hjb_rank_transfer_stream(hjb_rank r);
int32_t hjb_rank_step(hjb_rank r, void *dJ_in, void *dJ_out, void *d_idx, void *compute_stream);
/* The stage in the order that hides the exchange: boundary strips FIRST (the halos of dJ_in arrived during the previous stage),
 * the interior beside them, and the exchange of dJ_OUT's boundary planes as soon as the strips are done, under the rest of the
 * interior.  Precondition: dJ_in's halos are valid - one hjb_rank_exchange(r, dJ_in, stream) before the first step; every step
 * leaves dJ_out's halos filled (ordered for the next hjb_rank_step_post / the transfer stream / a device synchronisation).
 * hjb_rank_sweep runs this form (option "post_exchange" 0: hjb_rank_step) and returns - and stops its clock - only behind the
 * last stage's exchange, so the final buffer's halo planes are at rest when it hands the buffer back.
 * CONCURRENT USE OF THE COMMUNICATOR: a rank has ONE communicator; the exchange runs on the transfer stream, the monitor's
 * all-reduce on the compute stream.  The library never has two RCCL operations of one rank in flight unordered: the monitor's
 * all-reduce is enqueued behind an event that follows the pending exchange (hjb_rank_monitor_sums waits for it on the compute
 * stream), and the next exchange is ordered behind the compute stream.  A host that issues its own RCCL calls on this
 * communicator must keep the same rule - one stream order per communicator. */
int32_t hjb_rank_step_post(hjb_rank r, void *dJ_in, void *dJ_out, void *d_idx, void *compute_stream);
int32_t hjb_rank_monitor_sums(hjb_rank r, const void *dJ, const void *d_idx, void *compute_stream, double *sums2);
int32_t hjb_rank_sweep(hjb_rank r, int32_t n_stages, int32_t monitor_period, double monitor_tol, void *dJ0, void *dJ1, void *d_idx,
                       void *compute_stream, int32_t *stages_done, int32_t *stopped_early, int32_t *final_in_0, double *sweep_ms);

#ifdef __cplusplus
}
#endif
#endif /* HJBDP_H */
