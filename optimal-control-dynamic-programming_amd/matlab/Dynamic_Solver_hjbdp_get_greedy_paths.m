function [X, U, J, V] = Dynamic_Solver_hjbdp_get_greedy_paths(obj, X0s, mode, ssu_num)
%DYNAMIC_SOLVER_HJBDP_GET_GREEDY_PATHS  the closed loop of test/Dynamic_Solver.m flown by the cost-to-go itself, on the GPU
% (hjb_rollout_set_values / hjb_rollout_run_greedy, include/hjbdp.h): at every step the control of U_mesh that minimises
%   x'Qx + R u^2 + J_{k+1}(A x + B u),
% J_{k+1} the plane of obj.J_star behind the step, blended linearly at the next state - one-step lookahead at the state actually
% visited, where Dynamic_Solver_hjbdp_get_optimal_paths interpolates the stored labels' controls (:121-135):
%   objA = Dynamic_Solver;  Dynamic_Solver_hjbdp_run(objA);
%   [X, U, J] = Dynamic_Solver_hjbdp_get_greedy_paths(objA, X0s)
% X0s: [S, n], one initial state per column.  X: [S, N, n], U: [N, n] (U(N, :) = 0), J: [n, 1] closed-loop costs, V: [N-1, n] the
% cost-to-go the controller believed at every step.  Step k (1-based) reads plane k + 1 of J_star, whose last plane is the zero
% terminal (:77-80); mode 'ssu' freezes plane ssu_num + 1 (:127-131).  Needs obj.J_star and obj.u_star_idxs from the run.
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/dynamic_solver.py get_greedy_paths.
    if nargin < 3, mode = 'Nssu'; end
    if nargin < 4, ssu_num = 1; end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = obj.N;  S = size(X0s, 1);  n = size(X0s, 2);  K = N - 1;
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
    Xf = libpointer('doublePtr', zeros(S, n));  Jp = libpointer('doublePtr', zeros(n, 1));
    Xp = libpointer('doublePtr', zeros(n, S, N));  Up = libpointer('doublePtr', zeros(n, 1, K));
    Vp = libpointer('doublePtr', zeros(n, K));  ms = libpointer('doublePtr', 0);
    check(calllib(L, 'hjb_rollout_run_greedy', rv, int32(K), planes, int64(n), double(X0s), Xf, Jp, Xp, Up, [], Vp, ms), rv);
    X = permute(reshape(Xp.Value, n, S, N), [2 3 1]);
    U = [reshape(Up.Value, n, K).'; zeros(1, n)];
    J = Jp.Value;
    V = reshape(Vp.Value, n, K).';

    function check(st, obj_)
        if st == 0, return; end
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', obj_), calllib(L, 'hjb_status_string', int32(st)));
    end
end
