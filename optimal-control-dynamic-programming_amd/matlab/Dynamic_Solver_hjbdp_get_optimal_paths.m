function [X, U, J] = Dynamic_Solver_hjbdp_get_optimal_paths(obj, X0s, mode, ssu_num)
%DYNAMIC_SOLVER_HJBDP_GET_OPTIMAL_PATHS  get_optimal_path (test/Dynamic_Solver.m:108-181, 'Nssu' :121-126 and 'ssu' :127-131)
% for many initial states at once, on the GPU (hjb_rollout_*, include/hjbdp.h):
%   objA = Dynamic_Solver;  Dynamic_Solver_hjbdp_run(objA);  [X, U, J] = Dynamic_Solver_hjbdp_get_optimal_paths(objA, X0s)
% X0s: [S, n], one initial state per column.  X: [S, N, n], U: [N, n] (U(N, :) = 0 as the reference leaves it), J: [n] closed-loop
% costs.  Needs obj.u_star_idxs ([dx, dx, N-1] labels into U_mesh, :100) from the run.  The policy is U_mesh in the class of
% obj.u_star, looked up in double on the double grid vectors; the loop x(k+1) = A x(k) + B u(k) (:191-194) runs in libhjbdp.
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/dynamic_solver.py get_optimal_paths.
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
    if strcmp(mode, 'ssu'), planes = int32(repmat(ssu_num - 1, 1, K)); else, planes = int32(0:K-1); end
    ro = libpointer('voidPtrPtr');
    check(calllib(L, 'hjb_rollout_create', int32(0), int32(2), int32([obj.dx obj.dx]), [s_r; s_r], int32(0), int32(1), ...
                  int32(K), int32(obj.u_star_idxs(:)), int32(obj.du), int32(1), u_table, ro), []);   % HJB_IDX_I32, 1-based
    rv = ro.Value;
    cleanup = onCleanup(@() calllib(L, 'hjb_rollout_destroy', rv));
    check(calllib(L, 'hjb_rollout_set_model', rv, double(obj.A(:)), double(obj.B(:)), [], double(diag(obj.Q)), double(obj.R)), rv);
    Xf = libpointer('doublePtr', zeros(S, n));  Jp = libpointer('doublePtr', zeros(n, 1));
    Xp = libpointer('doublePtr', zeros(n, S, N));  Up = libpointer('doublePtr', zeros(n, 1, K));
    ms = libpointer('doublePtr', 0);
    check(calllib(L, 'hjb_rollout_run', rv, int32(1), int32(K), planes, int64(n), double(X0s), Xf, Jp, Xp, Up, ms), rv);  % LINEAR
    X = permute(reshape(Xp.Value, n, S, N), [2 3 1]);
    U = zeros(N, n);
    U(1:K, :) = reshape(Up.Value, n, K).';
    J = Jp.Value;

    function check(st, obj_)
        if st == 0, return; end
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', obj_), calllib(L, 'hjb_status_string', int32(st)));
    end
end
