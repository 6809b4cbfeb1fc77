function [J, Jmean, Jstd, Jmax] = Dynamic_Solver_hjbdp_get_noisy_paths(obj, X0s, n_samples, offsets, weights, seed, mode, ssu_num)
%DYNAMIC_SOLVER_HJBDP_GET_NOISY_PATHS  the stored policy of test/Dynamic_Solver.m flown under sampled process noise, on the GPU
% (hjb_rollout_set_noise / hjb_rollout_run_noisy, include/hjbdp.h): x(k+1) = A x(k) + B u(k) + d_w, node w of the set
% (offsets [2, W], weights [W] or [] = equal) drawn per trajectory and step - the node set hjbdp_set_disturbance takes, so the
% policy designed and priced under it (hjbdp_solve's 'disturbance' pair, hjbdp_evaluate) is flown under it:
%   objA = Dynamic_Solver;  Dynamic_Solver_hjbdp_run(objA);
%   J = Dynamic_Solver_hjbdp_get_noisy_paths(objA, X0s, 4096, offsets, weights)
% X0s: [S, n], one initial state per column, each flown n_samples times; sample j of start i runs on stream (i-1) * n_samples
% + (j-1) of `seed` (Philox4x32-10, counter-based: the same call gives the same numbers).  J: [n, n_samples] closed-loop costs of
% the states actually visited; Jmean, Jstd, Jmax: [n, 1] over the samples.  mode / ssu_num as in
% Dynamic_Solver_hjbdp_get_optimal_paths ('Nssu' :121-126, 'ssu' :127-131).  Needs obj.u_star_idxs from the run.
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/dynamic_solver.py get_noisy_paths.
    if nargin < 5, weights = []; end
    if nargin < 6, seed = 0; end
    if nargin < 7, mode = 'Nssu'; end
    if nargin < 8, ssu_num = 1; end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = obj.N;  S = size(X0s, 1);  n = size(X0s, 2);  K = N - 1;  W = size(offsets, 2);
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
    check(calllib(L, 'hjb_rollout_set_noise', rv, int32(W), double(offsets(:)), double(weights(:))), rv);
    nt = n * n_samples;
    X0 = kron(double(X0s), ones(1, n_samples));                                 % every start n_samples times, samples adjacent
    Xf = libpointer('doublePtr', zeros(S, nt));  Jp = libpointer('doublePtr', zeros(nt, 1));
    ms = libpointer('doublePtr', 0);
    check(calllib(L, 'hjb_rollout_run_noisy', rv, int32(1), int32(K), planes, int64(nt), X0, uint64(seed), int64(0), Xf, Jp, ...
                  [], [], [], ms), rv);                                         % LINEAR, no paths
    J = reshape(Jp.Value, n_samples, n).';
    Jmean = mean(J, 2);  Jstd = std(J, 1, 2);  Jmax = max(J, [], 2);

    function check(st, obj_)
        if st == 0, return; end
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', obj_), calllib(L, 'hjb_status_string', int32(st)));
    end
end
