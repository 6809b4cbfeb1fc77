function [Jq, hist, lo, hi, stats] = Dynamic_Solver_hjbdp_noisy_cost_quantile_map(obj, n_samples, offsets, weights, q, n_bins, seed, mode, ssu_num)
%DYNAMIC_SOLVER_HJBDP_NOISY_COST_QUANTILE_MAP  quantiles of the closed-loop cost of the stored policy of test/Dynamic_Solver.m,
% flown n_samples times from EVERY grid node under sampled process noise, from per-node histograms reduced on the GPU
% (hjb_rollout_run_campaign / hjb_rollout_run_campaign_hist, include/hjbdp.h): nothing of length dx * dx * n_samples exists on the
% host or on the device.  Two campaigns on one seed and the same streams (Dynamic_Solver_hjbdp_noisy_cost_map's numbering): the
% first gives every node's min and max, the second flies the same samples again - the streams are counter-based - and counts them
% in n_bins equal bins between lo = min and hi = the next double above max (hi = lo + 1 where min = max), so every node's range
% fits it exactly whatever the cost's scale over the grid:
%   objA = Dynamic_Solver;  Dynamic_Solver_hjbdp_run(objA);
%   Jq = Dynamic_Solver_hjbdp_noisy_cost_quantile_map(objA, 1024, offsets, weights, [0.5 0.95 0.99], 64)
% Jq [dx, dx, numel(q)]: for the rank k = max(1, ceil(q * M)) the upper edge lo + j * (hi - lo) / n_bins of the first bin j whose
% cumulative count reaches k, clipped to [min, max] - at most one bin width above the k-th smallest cost; q = 1 gives max.
% hist [n_bins + 2, dx, dx] int64 (underflow, the bins, overflow; both ends empty here), lo, hi [dx, dx], stats [8, dx, dx] as
% Dynamic_Solver_hjbdp_noisy_cost_map returns them.  mode / ssu_num as there.  Needs obj.u_star_idxs from the run.
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/dynamic_solver.py noisy_cost_quantile_map.
    if nargin < 4, weights = []; end
    if nargin < 5 || isempty(q), q = [0.5 0.95 0.99]; end
    if nargin < 6 || isempty(n_bins), n_bins = 64; end
    if nargin < 7, seed = 0; end
    if nargin < 8, mode = 'Nssu'; end
    if nargin < 9, ssu_num = 1; end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = obj.N;  K = N - 1;  W = size(offsets, 2);  dx = obj.dx;  ns = dx * dx;  M = n_samples;  nb = n_bins;
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
    [X1, X2] = ndgrid(s_r, s_r);
    X0 = [X1(:).'; X2(:).'];                                                    % every node once, axis 1 fastest
    sp = libpointer('doublePtr', zeros(8, ns));
    ms = libpointer('doublePtr', 0);
    % pass 1: the plain campaign, for every node's min and max
    check(calllib(L, 'hjb_rollout_run_campaign', rv, int32(1), int32(K), planes, int64(ns), int64(M), X0, uint64(seed), int64(0), ...
                  [], [], sp, ms), rv);                                         % LINEAR
    s1 = sp.Value;
    lo = s1(3, :).';  mx = s1(4, :).';
    hi = mx + eps(mx);                                                          % the next double above max
    flat = ~(lo < hi) | lo == mx | ~isfinite(lo) | ~isfinite(hi);
    lo(~isfinite(lo)) = 0;
    hi(flat) = lo(flat) + 1;
    % pass 2: the same samples again, counted between lo and hi
    hp = libpointer('int64Ptr', zeros(nb + 2, ns, 'int64'));
    check(calllib(L, 'hjb_rollout_run_campaign_hist', rv, int32(1), int32(K), planes, int64(ns), int64(M), X0, uint64(seed), int64(0), ...
                  [], [], lo, hi, int32(nb), sp, hp, ms), rv);
    stats = reshape(sp.Value, 8, dx, dx);
    h = double(hp.Value);
    cum = cumsum(h, 1);                                                         % the underflow row counted first
    Jq = zeros(ns, numel(q));
    for i = 1:numel(q)
        k = max(1, ceil(q(i) * M));
        [~, row] = max(cum >= k, [], 1);                                        % the first row whose cumulative count reaches k
        j = row(:) - 1;                                                         % 0 underflow, 1 .. nb the bins, nb + 1 overflow
        edge = lo + j .* (hi - lo) / nb;
        edge(j == nb) = hi(j == nb);
        Jq(:, i) = min(max(edge, s1(3, :).'), mx);
    end
    Jq = reshape(Jq, dx, dx, numel(q));
    hist = reshape(hp.Value, nb + 2, dx, dx);
    lo = reshape(lo, dx, dx);  hi = reshape(hi, dx, dx);

    function check(st, obj_)
        if st == 0, return; end
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', obj_), calllib(L, 'hjb_status_string', int32(st)));
    end
end
