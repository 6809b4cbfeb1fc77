function [X, U, J, V, Wn] = Dynamic_Solver_hjbdp_get_lookahead_paths(obj, X0s, offsets, weights, dist_mode, n_samples, seed, mode, ssu_num)
%DYNAMIC_SOLVER_HJBDP_GET_LOOKAHEAD_PATHS  the closed loop of test/Dynamic_Solver.m flown by the DISTURBED cost-to-go, on the GPU
% (hjb_rollout_set_lookahead / hjb_rollout_run_lookahead, include/hjbdp.h): at every step the control of U_mesh that minimises
%   x'Qx + R u^2 + E_w J_{k+1}(A x + B u + d_w)      (dist_mode 'worst': max_w)
% over the node set (offsets [2, W], weights [W] or [] = equal) the solve was made under - Dynamic_Solver_hjbdp_get_greedy_paths
% with the disturbed backup inside every candidate, the controller that solve is exactly optimal for:
%   objA = Dynamic_Solver;  prob.disturbance = ...;  Dynamic_Solver_hjbdp_run(objA);
%   [X, U, J] = Dynamic_Solver_hjbdp_get_lookahead_paths(objA, X0s, offsets, weights, 'expect')            % nominal plant
%   [~, ~, J] = Dynamic_Solver_hjbdp_get_lookahead_paths(objA, X0s, offsets, weights, 'expect', 64, 7)     % 64 noisy samples a start
% X0s: [S, n], one initial state per column.  n_samples [] (default): the plant is nominal; X: [S, N, n], U: [N, n] (U(N, :) = 0),
% J: [n, 1] closed-loop costs, V: [N-1, n] the cost-to-go the controller believed.  n_samples given: every start is flown n_samples
% times under the same nodes (hjb_rollout_set_noise), sample j of start i on stream (i-1) * n_samples + (j-1) of `seed`; X, U, V
% then have n * n_samples columns (start-major), J is [n_samples, n] and Wn: [N-1, n * n_samples] the drawn nodes (0-based).
% Step k (1-based) reads plane k + 1 of J_star, whose last plane is the zero terminal (:77-80); mode 'ssu' freezes plane
% ssu_num + 1 (:127-131).  Needs obj.J_star and obj.u_star_idxs from the run.
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/dynamic_solver.py get_lookahead_paths.
    if nargin < 4, weights = []; end
    if nargin < 5, dist_mode = 'expect'; end
    if nargin < 6, n_samples = []; end
    if nargin < 7, seed = 0; end
    if nargin < 8, mode = 'Nssu'; end
    if nargin < 9, ssu_num = 1; end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = obj.N;  S = size(X0s, 1);  K = N - 1;  W = size(offsets, 2);
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
    is_worst = strcmp(dist_mode, 'worst');                                      % HJB_DIST_EXPECT = 0, HJB_DIST_WORST = 1
    check(calllib(L, 'hjb_rollout_set_lookahead', rv, int32(is_worst), int32(W), double(offsets(:)), double(weights(:))), rv);
    fly = ~isempty(n_samples);
    if fly
        check(calllib(L, 'hjb_rollout_set_noise', rv, int32(W), double(offsets(:)), double(weights(:))), rv);
        X0s = repelem(double(X0s), 1, n_samples);
    end
    n = size(X0s, 2);
    Xf = libpointer('doublePtr', zeros(S, n));  Jp = libpointer('doublePtr', zeros(n, 1));
    Xp = libpointer('doublePtr', zeros(n, S, N));  Up = libpointer('doublePtr', zeros(n, 1, K));
    Vp = libpointer('doublePtr', zeros(n, K));  ms = libpointer('doublePtr', 0);
    if fly, Wp = libpointer('doublePtr', zeros(n, K)); else, Wp = []; end
    check(calllib(L, 'hjb_rollout_run_lookahead', rv, int32(fly), int32(K), planes, int64(n), double(X0s), uint64(seed), int64(0), ...
                  Xf, Jp, Xp, Up, [], Vp, Wp, ms), rv);
    X = permute(reshape(Xp.Value, n, S, N), [2 3 1]);
    U = [reshape(Up.Value, n, K).'; zeros(1, n)];
    J = Jp.Value;
    V = reshape(Vp.Value, n, K).';
    Wn = [];
    if fly
        J = reshape(J, n_samples, []);
        Wn = reshape(Wp.Value, n, K).';
    end

    function check(st, obj_)
        if st == 0, return; end
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', obj_), calllib(L, 'hjb_status_string', int32(st)));
    end
end
