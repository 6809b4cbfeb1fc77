function [Jmean, Jstd, Jmax, stats] = Dynamic_Solver_hjbdp_lookahead_cost_map(obj, n_samples, offsets, weights, dist_mode, lookahead, seed, mode, ssu_num, threshold, tol)
%DYNAMIC_SOLVER_HJBDP_LOOKAHEAD_COST_MAP  the cost-to-go of test/Dynamic_Solver.m flown by one-step lookahead n_samples times from
% EVERY grid node under sampled process noise, the costs reduced per node on the GPU (hjb_rollout_set_lookahead /
% hjb_rollout_set_noise / hjb_rollout_run_lookahead_campaign, include/hjbdp.h): Dynamic_Solver_hjbdp_get_lookahead_paths' noisy
% flights as a campaign, and nothing of length dx * dx * n_samples exists on the host or on the device.
%   objA = Dynamic_Solver;  prob.disturbance = ...;  Dynamic_Solver_hjbdp_run(objA);
%   [Jla, ~, ~]  = Dynamic_Solver_hjbdp_lookahead_cost_map(objA, 1024, offsets, weights, 'expect')
%   [Jlab, ~, ~] = Dynamic_Solver_hjbdp_noisy_cost_map(objA, 1024, offsets, weights)
% lookahead 'disturbed' (default): the controller looks ahead under the node set (offsets [2, W], weights [W] or [] = equal,
% dist_mode 'expect' or 'worst') the solve was made under; 'nominal': under one zero node - Dynamic_Solver_hjbdp_get_greedy_paths'
% controller.  In both the node set is the plant.  Node (i, j) = (s_r(i), s_r(j)) is flown on streams
% ((i-1) + dx * (j-1)) * n_samples + (0 : n_samples-1) of `seed`: Dynamic_Solver_hjbdp_noisy_cost_map's streams, so with the same seed
% and n_samples the two maps fly common random numbers and Jla - Jlab is what the stored labels lose to the value function they
% came from, node by node, with the sampling noise largely cancelled.  Jmean, Jstd, Jmax, stats, threshold and tol as in
% Dynamic_Solver_hjbdp_noisy_cost_map.  Step k (1-based) reads plane k + 1 of J_star, whose last plane is the zero terminal
% (:77-80); mode 'ssu' freezes plane ssu_num + 1 (:127-131).  Needs obj.J_star and obj.u_star_idxs from the run.
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/dynamic_solver.py lookahead_cost_map.
    if nargin < 4, weights = []; end
    if nargin < 5, dist_mode = 'expect'; end
    if nargin < 6, lookahead = 'disturbed'; end
    if nargin < 7, seed = 0; end
    if nargin < 8, mode = 'Nssu'; end
    if nargin < 9, ssu_num = 1; end
    if nargin < 10, threshold = []; end
    if nargin < 11, tol = []; end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = obj.N;  K = N - 1;  W = size(offsets, 2);  dx = obj.dx;  ns = dx * dx;  M = n_samples;
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
    if strcmp(lookahead, 'nominal')                                             % one zero node of weight 1, HJB_DIST_EXPECT
        la_mode = int32(0);  la_W = int32(1);  la_off = zeros(2, 1);  la_w = 1;
    else                                                                        % HJB_DIST_EXPECT = 0, HJB_DIST_WORST = 1
        la_mode = int32(strcmp(dist_mode, 'worst'));  la_W = int32(W);  la_off = double(offsets(:));  la_w = double(weights(:));
    end
    check(calllib(L, 'hjb_rollout_set_lookahead', rv, la_mode, la_W, la_off, la_w), rv);
    check(calllib(L, 'hjb_rollout_set_noise', rv, int32(W), double(offsets(:)), double(weights(:))), rv);
    [X1, X2] = ndgrid(s_r, s_r);
    X0 = [X1(:).'; X2(:).'];                                                    % every node once, axis 1 fastest
    if ~isempty(threshold), threshold = repmat(double(threshold(1)), ns, 1); end
    sp = libpointer('doublePtr', zeros(8, ns));
    ms = libpointer('doublePtr', 0);
    check(calllib(L, 'hjb_rollout_run_lookahead_campaign', rv, int32(K), planes, int64(ns), int64(M), X0, uint64(seed), int64(0), ...
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
