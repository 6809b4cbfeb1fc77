function [Dmean, Dse, nBlower, nAlower, stats_d, stats_a, stats_b] = Dynamic_Solver_hjbdp_paired_cost_map(obj, n_samples, offsets, weights, dist_mode, a, b, seed, mode, ssu_num, method, threshold, tol)
%DYNAMIC_SOLVER_HJBDP_PAIRED_COST_MAP  two controllers of test/Dynamic_Solver.m flown n_samples times from EVERY grid node on the
% same sampled process noise, and the per-sample cost difference d = cost_b - cost_a reduced per node on the GPU
% (hjb_rollout_run_campaign_pair, include/hjbdp.h): Dynamic_Solver_hjbdp_noisy_cost_map's and
% Dynamic_Solver_hjbdp_lookahead_cost_map's flights in one call, with the standard error their two maps cannot give, and nothing of
% length dx * dx * n_samples on the host or on the device.
%   objA = Dynamic_Solver;  prob.disturbance = ...;  Dynamic_Solver_hjbdp_run(objA);
%   [Dmean, Dse] = Dynamic_Solver_hjbdp_paired_cost_map(objA, 1024, offsets, weights, 'expect', 'labels', 'disturbed')
% a and b are 'labels' (the stored policy, read with `method` 'linear' or 'nearest'), 'disturbed' (the one-step lookahead on J_star
% under the node set: offsets [2, W], weights [W] or [] = equal, dist_mode 'expect' or 'worst') or 'nominal' (the lookahead under one
% zero node).  The node set is the plant for both.  Node (i, j) = (s_r(i), s_r(j)) is flown on streams ((i-1) + dx * (j-1)) *
% n_samples + (0 : n_samples-1) of `seed` under BOTH controllers: the other maps' streams, so stats_a and stats_b [8, dx, dx] are
% their stats bit for bit.  stats_d [8, dx, dx]: sum d, sum d*d, min d, max d, n(b lower), n(a lower), n(both stayed in the grid),
% sum d over those.  Dmean = sum d / M (negative: b paid less), Dse = sqrt(var / M) with the unbiased variance clipped at 0.
% Label planes and value planes as in the two other maps; mode 'ssu' freezes them at ssu_num.
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/dynamic_solver.py paired_cost_map.
    if nargin < 4, weights = []; end
    if nargin < 5, dist_mode = 'expect'; end
    if nargin < 6, a = 'labels'; end
    if nargin < 7, b = 'disturbed'; end
    if nargin < 8, seed = 0; end
    if nargin < 9, mode = 'Nssu'; end
    if nargin < 10, ssu_num = 1; end
    if nargin < 11, method = 'linear'; end
    if nargin < 12, threshold = []; end
    if nargin < 13, tol = []; end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = obj.N;  K = N - 1;  W = size(offsets, 2);  dx = obj.dx;  ns = dx * dx;  M = n_samples;
    U_mesh = linspace(obj.u_min, obj.u_max, obj.du);                            % :72
    u_table = double(cast(U_mesh(:), class(obj.u_star)));
    s_r = double(obj.s_r(:));
    if strcmp(mode, 'ssu')                                                      % 0-based: label plane k-1 and value plane k of step k-1
        label_planes = int32(repmat(ssu_num - 1, 1, K));  value_planes = int32(repmat(ssu_num, 1, K));
    else
        label_planes = int32(0:K-1);  value_planes = int32(1:K);
    end
    [kind_a, planes_a] = side(a);
    [kind_b, planes_b] = side(b);
    lookup = int32(strcmp(method, 'linear'));                                   % HJB_LOOKUP_NEAREST = 0, HJB_LOOKUP_LINEAR = 1
    ro = libpointer('voidPtrPtr');
    check(calllib(L, 'hjb_rollout_create', int32(0), int32(2), int32([obj.dx obj.dx]), [s_r; s_r], int32(0), int32(1), ...
                  int32(K), int32(obj.u_star_idxs(:)), int32(obj.du), int32(1), u_table, ro), []);   % HJB_IDX_I32, 1-based
    rv = ro.Value;
    cleanup = onCleanup(@() calllib(L, 'hjb_rollout_destroy', rv));
    check(calllib(L, 'hjb_rollout_set_model', rv, double(obj.A(:)), double(obj.B(:)), [], double(diag(obj.Q)), double(obj.R)), rv);
    is_double = isa(obj.J_star, 'double');                                      % HJB_F32 = 0, HJB_F64 = 1
    check(calllib(L, 'hjb_rollout_set_values', rv, int32(is_double), int32(N), obj.J_star(:)), rv);
    check(calllib(L, 'hjb_rollout_set_lookahead', rv, int32(strcmp(dist_mode, 'worst')), int32(W), double(offsets(:)), double(weights(:))), rv);
    check(calllib(L, 'hjb_rollout_set_noise', rv, int32(W), double(offsets(:)), double(weights(:))), rv);
    [X1, X2] = ndgrid(s_r, s_r);
    X0 = [X1(:).'; X2(:).'];                                                    % every node once, axis 1 fastest
    if ~isempty(threshold), threshold = repmat(double(threshold(1)), ns, 1); end
    pa = libpointer('doublePtr', zeros(8, ns));
    pb = libpointer('doublePtr', zeros(8, ns));
    pd = libpointer('doublePtr', zeros(8, ns));
    ms = libpointer('doublePtr', 0);
    check(calllib(L, 'hjb_rollout_run_campaign_pair', rv, kind_a, lookup, planes_a, kind_b, lookup, planes_b, int32(K), int64(ns), ...
                  int64(M), X0, uint64(seed), int64(0), threshold, double(tol(:)), pa, pb, pd, ms), rv);
    stats_a = reshape(pa.Value, 8, dx, dx);  stats_b = reshape(pb.Value, 8, dx, dx);  stats_d = reshape(pd.Value, 8, dx, dx);
    S1 = reshape(stats_d(1, :, :), dx, dx);  S2 = reshape(stats_d(2, :, :), dx, dx);
    Dmean = S1 / M;
    if M > 1, Dse = sqrt(max((S2 - S1 .* S1 / M) / (M - 1), 0) / M); else, Dse = zeros(dx, dx); end
    nBlower = reshape(stats_d(5, :, :), dx, dx);  nAlower = reshape(stats_d(6, :, :), dx, dx);

    function [kind, planes] = side(name)                                        % HJB_PAIR_LABELS = 0, _LOOKAHEAD = 1, _GREEDY = 2
        switch name
            case 'labels',    kind = int32(0);  planes = label_planes;
            case 'disturbed', kind = int32(1);  planes = value_planes;
            case 'nominal',   kind = int32(2);  planes = value_planes;
            otherwise, error('hjbdp:pair', 'a and b must be ''labels'', ''nominal'' or ''disturbed''');
        end
    end

    function check(st, obj_)
        if st == 0, return; end
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', obj_), calllib(L, 'hjb_status_string', int32(st)));
    end
end
