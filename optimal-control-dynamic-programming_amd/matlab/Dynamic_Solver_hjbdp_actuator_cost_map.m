function [Jmean, Jstd, Jmax, stats] = Dynamic_Solver_hjbdp_actuator_cost_map(obj, n_samples, eps, weights, seed, mode, ssu_num, threshold, tol)
%DYNAMIC_SOLVER_HJBDP_ACTUATOR_COST_MAP  the stored policy of test/Dynamic_Solver.m flown n_samples times from EVERY grid node under
% sampled ACTUATOR noise - the plant delivers u * (1 + eps_w) instead of the commanded u, node w drawn per step - the costs reduced
% per node on the GPU (hjb_rollout_set_actuator_noise / hjb_rollout_run_actuator_campaign, include/hjbdp.h): nothing of length
% dx * dx * n_samples exists on the host or on the device.  Beside hjbdp_evaluate on a handle that holds the same set as a
% control-dependent disturbance (hjbdp_set_control_disturbance: d_w(l) = B * U_mesh(l) * eps(w)) this is "promised against paid"
% over the whole grid:
%   objA = Dynamic_Solver;  Dynamic_Solver_hjbdp_run(objA);
%   [Jmean, Jstd, Jmax] = Dynamic_Solver_hjbdp_actuator_cost_map(objA, 1024, eps, weights)
% eps: [1, W] relative errors of the one input; weights: [1, W] or [] = equal.  Node (i, j) = (s_r(i), s_r(j)) is flown on streams
% ((i-1) + dx * (j-1)) * n_samples + (0 : n_samples-1) of `seed` (Dynamic_Solver_hjbdp_noisy_cost_map's numbering: with the same
% seed and weights the two maps draw the same nodes).  Jmean, Jstd, Jmax: [dx, dx]; Jstd is the sample standard deviation
% sqrt((sumsq - sum^2 / M) / (M - 1)), 0 for M = 1.  stats: [8, dx, dx] - sum, sum of squares, min, max, n_exceed (cost >
% threshold; threshold a scalar or [] = none), n_left (the flight left the grid), n_settled (|x_final| <= tol on both axes; tol
% [2, 1] or [] = none), sum over the settled samples.  The cost is charged on the commanded controls.  mode / ssu_num as in
% Dynamic_Solver_hjbdp_get_optimal_paths ('Nssu' :121-126, 'ssu' :127-131).  Needs obj.u_star_idxs from the run.
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/dynamic_solver.py actuator_cost_map.
    if nargin < 4, weights = []; end
    if nargin < 5, seed = 0; end
    if nargin < 6, mode = 'Nssu'; end
    if nargin < 7, ssu_num = 1; end
    if nargin < 8, threshold = []; end
    if nargin < 9, tol = []; end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = obj.N;  K = N - 1;  W = numel(eps);  dx = obj.dx;  ns = dx * dx;  M = n_samples;
    U_mesh = linspace(obj.u_min, obj.u_max, obj.du);                            % :72
    u_table = double(cast(U_mesh(:), class(obj.u_star)));
    s_r = double(obj.s_r(:));
    if strcmp(mode, 'ssu'), planes = int32(repmat(ssu_num - 1, 1, K)); else, planes = int32(0:K-1); end
    ro = libpointer('voidPtrPtr');
    check(calllib(L, 'hjb_rollout_create', int32(0), int32(2), int32([obj.dx obj.dx]), [s_r; s_r], int32(0), int32(1), ...
                  int32(K), int32(obj.u_star_idxs(:)), int32(obj.du), int32(1), u_table, ro), []);   % HJB_IDX_I32, 1-based
    rv = ro.Value;
    cleanup = onCleanup(@() calllib(L, 'hjb_rollout_destroy', rv));
    check(calllib(L, 'hjb_rollout_set_model', rv, double(obj.A(:)), double(obj.B(:)), [], double(diag(obj.Q)), double(obj.R)), rv);
    check(calllib(L, 'hjb_rollout_set_actuator_noise', rv, int32(W), double(eps(:)), [], double(weights(:))), rv);   % [n_u = 1, W]; no base
    [X1, X2] = ndgrid(s_r, s_r);
    X0 = [X1(:).'; X2(:).'];                                                    % every node once, axis 1 fastest
    if ~isempty(threshold), threshold = repmat(double(threshold(1)), ns, 1); end
    sp = libpointer('doublePtr', zeros(8, ns));
    ms = libpointer('doublePtr', 0);
    check(calllib(L, 'hjb_rollout_run_actuator_campaign', rv, int32(1), int32(K), planes, int64(ns), int64(M), X0, uint64(seed), int64(0), ...
                  threshold, double(tol(:)), sp, ms), rv);                      % LINEAR
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
