function [Jmean, Jstd, Jmax, stats] = Dynamic_Solver_hjbdp_actuator_lookahead_cost_map(obj, n_samples, eps, weights, dist_mode, seed, mode, ssu_num, threshold, tol)
%DYNAMIC_SOLVER_HJBDP_ACTUATOR_LOOKAHEAD_COST_MAP  the cost-to-go of test/Dynamic_Solver.m designed under ACTUATOR noise, flown
% directly n_samples times from EVERY grid node on the actuator plant, the costs reduced per node on the GPU
% (hjb_rollout_set_control_lookahead / hjb_rollout_set_actuator_noise / hjb_rollout_run_control_lookahead_campaign,
% include/hjbdp.h): at every step the control of U_mesh that minimises x'Qx + R u^2 + E_w J_{k+1}(A x + B u (1 + eps_w)) (dist_mode
% 'worst': max_w) at the state actually visited, the plant delivering u * (1 + eps_w'), node w' drawn per step.  Nothing of length
% dx * dx * n_samples exists on the host or on the device.  The lookahead table is the one the design's handle holds
% (hjbdp_set_control_disturbance: d_w(l) = B * (U_mesh(l) * eps(w))), so what was designed under is what is believed and flown:
%   objA = Dynamic_Solver;  ... a run on a handle with hjbdp_set_control_disturbance(h, off, weights, dist_mode) ...
%   [Jmean, Jstd, Jmax] = Dynamic_Solver_hjbdp_actuator_lookahead_cost_map(objA, 1024, eps, weights)
% eps: [1, W] relative errors of the one input; weights: [1, W] or [] = equal ([] with dist_mode 'worst', which is then sampled
% uniformly); dist_mode 'expect' (default) or 'worst'.  Node (i, j) = (s_r(i), s_r(j)) is flown on streams
% ((i-1) + dx * (j-1)) * n_samples + (0 : n_samples-1) of `seed` - Dynamic_Solver_hjbdp_actuator_cost_map's numbering: with the same
% seed and weights the stored labels and the value function fly common random numbers, and the difference of the two maps' means
% is what the interpolated labels lose, node by node.  Jmean, Jstd, Jmax, stats, threshold and tol as in
% Dynamic_Solver_hjbdp_actuator_cost_map; the cost is charged on the commanded controls.  Step k (1-based) reads plane k + 1 of
% J_star, whose last plane is the zero terminal (:77-80); mode 'ssu' freezes plane ssu_num + 1 (:127-131).  Needs obj.J_star and
% obj.u_star_idxs from the run.
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/dynamic_solver.py actuator_lookahead_cost_map.
    if nargin < 4, weights = []; end
    if nargin < 5, dist_mode = 'expect'; end
    if nargin < 6, seed = 0; end
    if nargin < 7, mode = 'Nssu'; end
    if nargin < 8, ssu_num = 1; end
    if nargin < 9, threshold = []; end
    if nargin < 10, tol = []; end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = obj.N;  K = N - 1;  W = numel(eps);  dx = obj.dx;  ns = dx * dx;  M = n_samples;
    U_mesh = linspace(obj.u_min, obj.u_max, obj.du);                            % :72
    u_table = double(cast(U_mesh(:), class(obj.u_star)));
    s_r = double(obj.s_r(:));
    if strcmp(mode, 'ssu'), planes = int32(repmat(ssu_num, 1, K)); else, planes = int32(1:K); end   % 0-based plane k of step k-1
    ro = libpointer('voidPtrPtr');
    check(calllib(L, 'hjb_rollout_create', int32(0), int32(2), int32([obj.dx obj.dx]), [s_r; s_r], int32(0), int32(1), ...
                  int32(K), int32(obj.u_star_idxs(:)), int32(obj.du), int32(1), u_table, ro), []);   % HJB_IDX_I32, 1-based
    rv = ro.Value;
    cleanup = onCleanup(@() calllib(L, 'hjb_rollout_destroy', rv));
    check(calllib(L, 'hjb_rollout_set_model', rv, double(obj.A(:)), double(obj.B(:)), [], double(diag(obj.Q)), double(obj.R)), rv);
    is_double = isa(obj.J_star, 'double');                                      % HJB_F32 = 0, HJB_F64 = 1
    check(calllib(L, 'hjb_rollout_set_values', rv, int32(is_double), int32(N), obj.J_star(:)), rv);
    % the table of hjbdp.actuator_nodes, [2, W, du] column-major: off(a, w, l) = B(a) * (U_mesh(l) * eps(w)), in double
    ue = double(eps(:)) * double(U_mesh(:)).';                                  % [W, du]
    off = zeros(2, W, obj.du);
    for a = 1:2, off(a, :, :) = double(obj.B(a)) * ue; end
    la_mode = int32(strcmp(dist_mode, 'worst'));                                % HJB_DIST_EXPECT = 0, HJB_DIST_WORST = 1
    if la_mode == 1, la_w = []; else, la_w = double(weights(:)); end
    check(calllib(L, 'hjb_rollout_set_control_lookahead', rv, la_mode, int32(W), int32(obj.du), off(:), la_w), rv);
    check(calllib(L, 'hjb_rollout_set_actuator_noise', rv, int32(W), double(eps(:)), [], double(weights(:))), rv);   % [n_u = 1, W]; no base
    [X1, X2] = ndgrid(s_r, s_r);
    X0 = [X1(:).'; X2(:).'];                                                    % every node once, axis 1 fastest
    if ~isempty(threshold), threshold = repmat(double(threshold(1)), ns, 1); end
    sp = libpointer('doublePtr', zeros(8, ns));
    ms = libpointer('doublePtr', 0);
    check(calllib(L, 'hjb_rollout_run_control_lookahead_campaign', rv, int32(K), planes, int64(ns), int64(M), X0, uint64(seed), int64(0), ...
                  threshold, double(tol(:)), sp, ms), rv);
    stats = reshape(sp.Value, 8, dx, dx);
    S1 = reshape(stats(1, :, :), dx, dx);  S2 = reshape(stats(2, :, :), dx, dx);
    Jmean = S1 / M;
    if M > 1, Jstd = sqrt(max((S2 - S1 .* S1 / M) / (M - 1), 0)); else, Jstd = zeros(dx, dx); end
    Jmax = reshape(stats(4, :, :), dx, dx);

    function check(st, obj_)
        if st == 0, return; end
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', obj_), calllib(L, 'hjb_status_string', int32(st)));
    end
end
