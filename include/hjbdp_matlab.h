/* hjbdp_matlab.h - the flat part of include/hjbdp.h for MATLAB's loadlibrary.
 *
 * loadlibrary parses C prototypes but cannot marshal hjb_problem (arrays of structs holding pointers) or incomplete
 * struct pointer types comfortably.  Every function below takes primitives, plain arrays and opaque `void *` handles
 * only; the symbols are the same ones include/hjbdp.h declares (hjb_builder / hjb_handle / hjb_multi are pointers,
 * spelled void * here).  Usage: matlab/hjbdp_solve.m; semantics: include/hjbdp.h.
 *
 *   loadlibrary('libhjbdp.so', 'hjbdp_matlab.h')
 */
#ifndef HJBDP_MATLAB_H
#define HJBDP_MATLAB_H
#include <stdint.h>

const char *hjb_version(void);
const char *hjb_status_string(int32_t status);
int32_t hjb_device_count(void);

/* problem description: replaces the table building of the reference's run methods (test/Dynamic_Solver.m:66-84) */
int32_t hjb_problem_new(int32_t D, int32_t C, const int32_t *n, const int32_t *m, int32_t dtype, int32_t index_base, void **builder_out);
int32_t hjb_problem_set_knots(void *builder, int32_t axis, const double *knots, int32_t len);
int32_t hjb_problem_add_next_term(void *builder, int32_t axis, uint32_t mask, const void *data, int64_t count);
int32_t hjb_problem_add_cost_term(void *builder, uint32_t mask, const void *data, int64_t count);
int32_t hjb_problem_set_slab(void *builder, int32_t slab_begin, int32_t slab_end, int32_t halo_lo, int32_t halo_hi);
int32_t hjb_problem_set_types(void *builder, int32_t idx_dtype, int32_t table_dtype);
int32_t hjb_problem_set_cost_type(void *builder, int32_t cost_dtype);
int32_t hjb_problem_set_model(void *builder, int32_t model, double model_h, const void *t0, const void *t1, const void *t2, const void *t3);
int32_t hjb_problem_permute_axes(void *builder, const int32_t *order);
int32_t hjb_problem_suggest_order(void *builder, int32_t *order_out, int32_t *found);
int32_t hjb_create_from(void *builder, int32_t device, void **handle_out);
int32_t hjb_problem_free(void *builder);
const char *hjb_problem_last_error(void *builder);

/* the stage loops: test/Dynamic_Solver.m:86-102, Solver_position.m:132-141, Solver_attitude.m:236-247 / :280-287,
 * Solver_pos_att.m:270-286 */
int32_t hjb_solve_flat(void *handle, int32_t n_stages, int32_t monitor_period, double monitor_tol, const void *terminal,
                       void *J_final, void *idx_final, void *J_stages, void *idx_stages, int32_t *stages_done,
                       int32_t *stopped_early, double *sweep_ms);
/* one stage: [F.Values, idx] = min(J_stage + F(x_next...), [], ctrl_dim)  (Dynamic_Solver.m:207-210) */
int32_t hjb_backup_stage(void *handle, const void *J_next, void *J_out, void *idx_out);
/* ... on device buffers (hjb_device_malloc below), asynchronous: the entry point of a host that keeps its own `for k` loop
 * (hjbdp_solve.m 'on_stage'); stream NULL = the default stream.  hjb_check_device_status synchronises and reports a left slab. */
int32_t hjb_backup_stage_device(void *handle, const void *dJ_next, void *dJ_out, void *d_idx_out, void *stream);
int32_t hjb_check_device_status(void *handle, void *stream);
/* the cost of a GIVEN policy (labels as hjb_backup_stage / hjb_solve_flat write them): one stage on host buffers, one stage on
 * device buffers, and the sweep (labels_per_stage 0: one stationary policy, 1: one plane per stage); usage: matlab/hjbdp_evaluate.m */
int32_t hjb_evaluate_stage(void *handle, const void *J_next, const void *labels, void *J_out);
int32_t hjb_evaluate_stage_device(void *handle, const void *dJ_next, const void *d_labels, void *dJ_out, void *stream);
int32_t hjb_evaluate(void *handle, int32_t n_stages, const void *terminal, const void *labels, int32_t labels_per_stage,
                     void *J_final, void *J_stages, double *sweep_ms);
/* a disturbance in the backup (kernel variant 8): mode 0 expected value / 1 worst case over n_nodes additive offsets of the next
 * state (offsets [D, n_nodes] column-major; weights [n_nodes], expected value only, NULL = equal); n_nodes 0 detaches.  Every stage
 * the handle launches afterwards carries it; usage: matlab/hjbdp_set_disturbance.m, hjbdp_solve's 'disturbance' pair */
int32_t hjb_set_disturbance(void *handle, int32_t mode, int32_t n_nodes, const double *offsets, const double *weights);
/* ... that depends on the candidate control (K32): offsets [D, n_nodes, n_controls] column-major by the 0-based column-major control
 * label, n_controls = the handle's number of controls; the two setters replace each other; usage: matlab/hjbdp_set_control_disturbance.m */
int32_t hjb_set_control_disturbance(void *handle, int32_t mode, int32_t n_nodes, int32_t n_controls, const double *offsets,
                                    const double *weights);
int32_t hjb_get_info_flat(void *handle, int64_t *out8);
int32_t hjb_set_option(void *handle, const char *key, int64_t value);
int32_t hjb_get_option(void *handle, const char *key, int64_t *value);
const char *hjb_last_error(void *handle);
int32_t hjb_destroy(void *handle);

/* the same loop over several GPUs of this process (slabs of the last state axis) */
int32_t hjb_create_multi_from(void *builder, int32_t n_dev, const int32_t *devices, void **multi_out);
int32_t hjb_solve_multi_flat(void *multi, int32_t n_stages, int32_t monitor_period, double monitor_tol, const void *terminal,
                             void *J_final, void *idx_final, int32_t *stages_done, int32_t *stopped_early, double *sweep_ms);
int32_t hjb_multi_set_option(void *multi, const char *key, int64_t value);
const char *hjb_multi_last_error(void *multi);
int32_t hjb_destroy_multi(void *multi);

/* one process (MATLAB worker) per GPU: this rank's slab of the last state axis, one call per stage; the worker owns the
 * device buffers (hjb_device_*) and moves the halo planes between stages (include/hjbdp.h "one process per GPU") */
int32_t hjb_rank_create_from(void *builder, int32_t device, int32_t rank, int32_t world, int32_t overlap, void **rank_out);
int32_t hjb_rank_info(void *rank, int32_t *out10);
int32_t hjb_rank_stage(void *rank, const void *dJ_in, void *dJ_out, void *d_idx, void *compute_stream, void *halo_stream);
int32_t hjb_rank_set_option(void *rank, const char *key, int64_t value);
int32_t hjb_rank_get_option(void *rank, const char *key, int64_t *value);
int32_t hjb_rank_check_status(void *rank, void *stream);
int32_t hjb_rank_destroy(void *rank);
const char *hjb_rank_last_error(void *rank);
/* RCCL transport inside the library (include/hjbdp.h): the 128-byte id from rank 0 goes to every worker by labSend / a file */
int32_t hjb_rank_comm_available(void);
int32_t hjb_rank_comm_unique_id(void *id128_out);
int32_t hjb_rank_comm_init(void *rank, const void *id128);
int32_t hjb_rank_step(void *rank, void *dJ_in, void *dJ_out, void *d_idx, void *compute_stream);
int32_t hjb_rank_monitor_sums(void *rank, const void *dJ, const void *d_idx, void *compute_stream, double *sums2);
int32_t hjb_rank_sweep(void *rank, int32_t n_stages, int32_t monitor_period, double monitor_tol, void *dJ0, void *dJ1, void *d_idx,
                       void *compute_stream, int32_t *stages_done, int32_t *stopped_early, int32_t *final_in_0, double *sweep_ms);
/* device buffers for hosts without a HIP binding of their own */
int32_t hjb_device_malloc(int32_t device, int64_t bytes, void **out);
int32_t hjb_device_free(int32_t device, void *p);
int32_t hjb_device_copy(int32_t device, void *dst, const void *src, int64_t bytes, int32_t kind);

/* griddedInterpolant(..., 'nearest' | 'linear') lookups of the results (Solver_position.m:144-146, Dynamic_Solver.m:132-135) */
int32_t hjb_policy_lookup(int32_t device, int32_t dtype, int32_t D, const int32_t *n, const double *const *knots,
                          const void *values, int64_t nq, const void *queries, int32_t method, void *out);

/* batched closed-loop rollouts of the stored per-stage policy (test/Dynamic_Solver.m:108-181, get_optimal_path 'Nssu' / 'ssu');
 * usage: matlab/Dynamic_Solver_hjbdp_get_optimal_paths.m */
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
/* the affine loop under sampled additive process noise (kernel K25): a node set as hjb_set_disturbance takes it (offsets
 * [D, n_nodes] column-major, weights [n_nodes] or NULL = equal; n_nodes 0 detaches), one Philox4x32-10 stream per trajectory
 * (first_stream + its index in the call), W_path the drawn node of every step; the two host twins of the sampler need no device
 * (hjbdp.h); usage: matlab/Dynamic_Solver_hjbdp_get_noisy_paths.m */
int32_t hjb_rollout_set_noise(void *rollout, int32_t n_nodes, const double *offsets, const double *weights);
int32_t hjb_rollout_run_noisy(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                              const double *X0, uint64_t seed, int64_t first_stream, double *X_final, double *cost, double *X_path,
                              double *U_path, double *W_path, double *device_ms);
int32_t hjb_rollout_noise_table(int32_t n_nodes, const double *weights, double *thresholds);
int32_t hjb_rollout_noise_draw(uint64_t seed, int64_t first_stream, int64_t n_traj, int32_t n_steps, int32_t n_nodes,
                               const double *thresholds, int32_t *nodes);
/* the noisy loop as a campaign (kernel K28): n_starts starts flown n_samples times each, sample m of start s on stream
 * first_stream + s * n_samples + m, reduced on the device to stats [8, n_starts] (sum, sum of squares, min, max, n_exceed, n_left,
 * n_settled, sum over settled; threshold [n_starts] and tol [D] may be NULL); the host reduce needs no device (hjbdp.h); usage:
 * matlab/Dynamic_Solver_hjbdp_noisy_cost_map.m */
int32_t hjb_rollout_run_campaign(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_starts,
                                 int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream, const double *threshold,
                                 const double *tol, double *stats, double *device_ms);
int32_t hjb_rollout_campaign_reduce(int64_t n_starts, int64_t n_samples, int32_t D, const double *cost, const double *X_final,
                                    const uint8_t *left, const double *threshold, const double *tol, double *stats);
/* the affine loop flown by one-step lookahead on stored value planes (kernel K26): values [nS, n_planes] column-major, dtype 0 =
 * single, 1 = double (n_planes 0 detaches); value_plane_of_step -1 = the zero terminal; L_path the chosen label + index_base,
 * V_path the minimum, per step; the host twin needs no device and no object (hjbdp.h); usage:
 * matlab/Dynamic_Solver_hjbdp_get_greedy_paths.m */
int32_t hjb_rollout_set_values(void *rollout, int32_t dtype, int32_t n_planes, const void *values);
int32_t hjb_rollout_run_greedy(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_traj,
                               const double *X0, double *X_final, double *cost, double *X_path, double *U_path,
                               double *L_path, double *V_path, double *device_ms);
int32_t hjb_rollout_greedy_host(int32_t D, const int32_t *n, const double *knots, int32_t n_labels, int32_t n_u,
                                const double *u_table, const double *A, const double *B, const double *c, const double *q,
                                const double *r, int32_t dtype, int32_t n_value_planes, const void *values, int32_t n_steps,
                                const int32_t *value_plane_of_step, int64_t n_traj, const double *X0, double *X_final,
                                double *cost, double *X_path, double *U_path, double *L_path, double *V_path);
/* the affine loop under actuator noise (kernels K33, K34): x+ = A x + B (u (1 + eps_w)) + c + base_w; eps [n_u, n_nodes] and base
 * [D, n_nodes] (or NULL) column-major, weights as hjb_rollout_set_noise's (n_nodes 0 detaches); hjb_rollout_run_noisy's and
 * hjb_rollout_run_campaign's arguments, streams and statistics (hjbdp.h); usage: matlab/Dynamic_Solver_hjbdp_actuator_cost_map.m */
int32_t hjb_rollout_set_actuator_noise(void *rollout, int32_t n_nodes, const double *eps, const double *base, const double *weights);
int32_t hjb_rollout_run_actuator(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                 const double *X0, uint64_t seed, int64_t first_stream, double *X_final, double *cost,
                                 double *X_path, double *U_path, double *W_path, double *device_ms);
int32_t hjb_rollout_run_actuator_campaign(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step,
                                          int64_t n_starts, int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream,
                                          const double *threshold, const double *tol, double *stats, double *device_ms);
/* the same loop with hjb_set_disturbance's E_w / max_w inside every candidate (kernel K27): a lookahead node set in
 * hjb_set_disturbance's layout (mode 0 = expect, 1 = worst; n_nodes 0 detaches), flown on a nominal plant (fly_noise 0) or under
 * hjb_rollout_set_noise's set (fly_noise 1, W_path the drawn nodes); the host twin needs no device and no object (hjbdp.h); usage:
 * matlab/Dynamic_Solver_hjbdp_get_lookahead_paths.m */
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
/* the flown lookahead as a campaign (kernel K29): hjb_rollout_run_campaign's arguments without the method, for the controller of
 * hjb_rollout_run_lookahead (value planes under the lookahead set) on the plant of hjb_rollout_set_noise; sample m of start s on
 * stream first_stream + s * n_samples + m - the stream hjb_rollout_run_campaign gives it, so the two campaigns of one seed fly common
 * random numbers; stats [8, n_starts] as there (hjbdp.h); usage: matlab/Dynamic_Solver_hjbdp_lookahead_cost_map.m */
int32_t hjb_rollout_run_lookahead_campaign(void *rollout, int32_t n_steps, const int32_t *value_plane_of_step, int64_t n_starts,
                                           int64_t n_samples, const double *X0, uint64_t seed, int64_t first_stream,
                                           const double *threshold, const double *tol, double *stats, double *device_ms);
/* the lookahead with a node set per candidate, the value function of hjb_set_control_disturbance flown directly (kernels K35, K36):
 * offsets [D, n_nodes, n_controls] column-major as hjb_set_control_disturbance takes them, n_controls the object's label count
 * (n_nodes 0 detaches); the run functions take hjb_rollout_run_lookahead's and hjb_rollout_run_lookahead_campaign's arguments, fly_noise
 * 1 and the campaign flying hjb_rollout_set_actuator_noise's plant on hjb_rollout_run_actuator_campaign's streams; the host twin needs
 * no device and no object (hjbdp.h); usage: matlab/Dynamic_Solver_hjbdp_actuator_lookahead_cost_map.m */
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
/* both campaigns with a histogram of every start's costs beside the statistics (kernel K30): n_bins (1..256) equal bins between
 * lo [n_starts] and hi [n_starts], hist [n_bins + 2, n_starts] int64 (underflow, the bins, overflow), stats the plain call's bits;
 * two calls on one seed - a plain campaign for min and max, then this with lo = min, hi = the next double above max - give every
 * start an exact range (hjbdp.h); the host twin of the binning needs no device; usage:
 * matlab/Dynamic_Solver_hjbdp_noisy_cost_quantile_map.m */
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
/* two controllers A and B on one plant, sample by sample on the plain campaigns' streams (kernel K31): kind 0 = stored labels
 * (planes are label planes, method read), 1 = the lookahead under the object's set, 2 = the lookahead under one zero node of weight 1
 * (planes are value planes, method ignored); stats_a and stats_b [8, n_starts] are the plain campaigns' bits, stats_d [8, n_starts] the
 * record of d = c_B - c_A (sum, sum of squares, min, max, n(B lower), n(A lower), n(both stayed in the grid), sum over those); the
 * host twin needs no device (hjbdp.h); usage: matlab/Dynamic_Solver_hjbdp_paired_cost_map.m */
int32_t hjb_rollout_run_campaign_pair(void *rollout, int32_t kind_a, int32_t method_a, const int32_t *planes_a, int32_t kind_b,
                                      int32_t method_b, const int32_t *planes_b, int32_t n_steps, int64_t n_starts, int64_t n_samples,
                                      const double *X0, uint64_t seed, int64_t first_stream, const double *threshold, const double *tol,
                                      double *stats_a, double *stats_b, double *stats_d, double *device_ms);
int32_t hjb_rollout_campaign_pair_reduce(int64_t n_starts, int64_t n_samples, const double *cost_a, const double *cost_b,
                                         const uint8_t *left_a, const uint8_t *left_b, double *stats_d);
/* the 6-D attitude loop on the same object (attitude-control/Solver_attitude.m:744-833, get_optimal_path after run);
 * usage: matlab/Solver_attitude_hjbdp_get_optimal_paths.m */
int32_t hjb_rollout_set_attitude_model(void *rollout, const double *inertia, double h, int32_t integrator, const double *q,
                                       const double *r);
int32_t hjb_rollout_run_attitude(void *rollout, int32_t method, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                 const double *X0, double *X_final, double *cost, double *X_path, double *U_path, double *A_path,
                                 double *device_ms);
/* the 13-state pos-att loop on three channel objects (pos-att/Solver_pos_att.m:452-730, get_optimal_path after simplified_run);
 * usage: matlab/Solver_pos_att_hjbdp_get_optimal_paths.m */
int32_t hjb_rollout_set_pos_att_model(void *rollout_x, void *rollout_y, void *rollout_z, const double *inertia, double mass,
                                      double t_dist, double h, int32_t substeps, const double *rsw2eci, int32_t n_nodes,
                                      const double *orbit_coef);
int32_t hjb_rollout_run_pos_att(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj, const double *X0,
                                double *X_final, double *X_path, double *F_path, double *FM_path);
/* thruster-fault campaigns in that loop (:235-240, channel_x_controller_1_failure): a fault controller for channel x attached to
 * the model (rollout_xf NULL detaches), a dead thruster and a hand-over per trajectory, impulse and settling stage per trajectory;
 * NULL ([]) for an input or output that is not wanted (hjbdp.h); usage: matlab/Solver_pos_att_hjbdp_fault_campaign.m */
int32_t hjb_rollout_set_pos_att_fault_controller(void *rollout_x, void *rollout_xf);
int32_t hjb_rollout_run_pos_att_faults(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                       const double *X0, const int32_t *fault_mask, const int32_t *fault_stage,
                                       const int32_t *switch_stage, double pos_tol, double att_tol, double *X_final, double *impulse,
                                       int32_t *settle_stage, double *X_path, double *F_path, double *FM_path, double *device_ms);
/* Solver_position's RKF45 loop on three channel objects (position-control/Solver_position.m:189-311, get_optimal_path after
 * simplified_run), on rkf45's fixed schedule with a per-trajectory off-schedule flag (hjbdp.h) */
int32_t hjb_rollout_set_position_model(void *rollout_x, void *rollout_y, void *rollout_z, double tol, int32_t n_steps, int32_t max_sub,
                                       const int32_t *n_sub, const double *table);
int32_t hjb_rollout_run_position(void *rollout_x, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj, const double *X0,
                                 double *X_final, double *X_path, double *A_path, int32_t *off_schedule);
/* the simplified attitude loop on three channel objects (attitude-control/Solver_attitude.m:835-925,
 * get_optimal_path_simplified_testode45 after simplified_run); dynamics 0 = full inertia matrix, RK4 sub-steps, 1 = diagonal
 * inertia, one RK4 step and q / |q| (hjbdp.h); usage: matlab/Solver_attitude_hjbdp_get_optimal_paths_simplified.m */
int32_t hjb_rollout_set_attitude_simplified_model(void *rollout_1, void *rollout_2, void *rollout_3, const double *inertia, double h,
                                                  int32_t substeps, int32_t dynamics, const double *qw, const double *qt,
                                                  const double *r);
int32_t hjb_rollout_run_attitude_simplified(void *rollout_1, int32_t n_steps, const int32_t *plane_of_step, int64_t n_traj,
                                            const double *X0, double *X_final, double *cost, double *X_path, double *U_path,
                                            double *A_path);
/* the linear attitude controller's closed loop (attitude-control/Solver_attitude.m:508-591, linear_control_response), stateless;
 * integrator 0 = taylor, 1 = RK4; cost_form 0 = weights q[7] r[3], 1 = weights qw[3] qt[3] r[3] and one unused (hjbdp.h); usage:
 * matlab/Solver_attitude_hjbdp_linear_control_responses.m */
int32_t hjb_attitude_linear_response(int32_t device, const double *inertia, double h, int32_t integrator, const double *K,
                                     const double *C, const double *qc, const double *u_limit, int32_t cost_form,
                                     const double *weights, int32_t n_steps, int64_t n_traj, const double *X0, double *X_final,
                                     double *cost, double *X_path, double *U_path, double *A_path, int64_t chunk, double *device_ms);
#endif
