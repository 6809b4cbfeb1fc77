function [X, U, X_ANGLES] = Solver_attitude_hjbdp_get_optimal_paths(obj, X0s, method, integrator)
%SOLVER_ATTITUDE_HJBDP_GET_OPTIMAL_PATHS  get_optimal_path (attitude-control/Solver_attitude.m:744-833) for many initial attitudes
% at once, on the GPU (hjb_rollout_set_attitude_model / hjb_rollout_run_attitude, include/hjbdp.h):
%   sa = Solver_attitude;  Solver_attitude_hjbdp_run(sa);  [X, U, X_ANGLES] = Solver_attitude_hjbdp_get_optimal_paths(sa, X0s)
% X0s: [7, n], one state X = [w1 w2 w3 q1 q2 q3 q4] (q4 scalar) per column (default obj.defaultX0, :746).  X: [7, N, n], U: [3, N, n] (U(:, N, :) = 0),
% X_ANGLES: [9, N, n] = [w; roll; pitch; yaw in degrees; U] (:780-782, last column 0).  method 'nearest' (the reference's,
% default) or 'linear' (HJB_LOOKUP_NEAREST 0 / _LINEAR 1); integrator 'taylor' (the reference's, :778, default) or 'RK4';
% any other name is an error.  The policy is the one run leaves:
% labels (i1-1) + 3 (i2-1) + 9 (i3-1) + 1 rebuilt from obj.U1_Opt .. obj.U3_Opt against single(obj.U_vector), the control
% table the 27 torque triples in single precision, on the grid vectors (w1, w2, w3, yaw, pitch, roll) in double (:759-764).
% The angles come from the library's fixed atan2 / asin forms (<= 2 ulp of libm, tested).
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/solver_attitude.py get_optimal_paths.
    if nargin < 2 || isempty(X0s), X0s = obj.defaultX0; end     % :746
    if nargin < 3, method = 'nearest'; end
    if nargin < 4, integrator = 'taylor'; end
    meths = {'nearest', 'linear'};  integs = {'taylor', 'RK4'};
    m = find(strcmpi(method, meths));  g = find(strcmpi(integrator, integs));
    if isempty(m), error('hjbdp:method', 'method ''%s'': ''nearest'' or ''linear''', method); end
    if isempty(g), error('hjbdp:integrator', 'integrator ''%s'': ''taylor'' or ''RK4''', integrator); end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = obj.N_stage;  K = N - 1;  n = size(X0s, 2);
    UV = single(obj.U_vector(:));  nu = numel(UV);
    [~, i1] = ismember(obj.U1_Opt, UV);  [~, i2] = ismember(obj.U2_Opt, UV);  [~, i3] = ismember(obj.U3_Opt, UV);
    labels = uint8((i1(:) - 1) + nu * (i2(:) - 1) + nu * nu * (i3(:) - 1) + 1);
    [a, b, c] = ndgrid(1:nu, 1:nu, 1:nu);
    u_table = double([UV(a(:)), UV(b(:)), UV(c(:))]);            % [27, 3], label l = a + 3 (b-1) + 9 (c-1)
    knots = {obj.sr_1, obj.sr_2, obj.sr_3, obj.s_yaw, obj.s_pitch, obj.s_roll};
    n_k = int32(cellfun(@numel, knots));
    kcat = cell2mat(cellfun(@(k) double(k(:)), knots, 'UniformOutput', false)');
    ro = libpointer('voidPtrPtr');
    check(calllib(L, 'hjb_rollout_create', int32(0), int32(6), n_k, kcat, int32(1), int32(1), ...
                  int32(1), labels, int32(nu ^ 3), int32(3), u_table(:), ro), []);     % HJB_IDX_U8, 1-based, one plane
    rv = ro.Value;
    cleanup = onCleanup(@() calllib(L, 'hjb_rollout_destroy', rv));
    check(calllib(L, 'hjb_rollout_set_attitude_model', rv, double([obj.J1 obj.J2 obj.J3]), double(obj.h), ...
                  int32(g - 1), [], []), rv);                                        % HJB_ATT_TAYLOR 0 / HJB_ATT_RK4 1
    Xf = libpointer('doublePtr', zeros(7, n));
    Xp = libpointer('doublePtr', zeros(n, 7, N));  Up = libpointer('doublePtr', zeros(n, 3, K));
    Ap = libpointer('doublePtr', zeros(n, 3, K));  ms = libpointer('doublePtr', 0);
    check(calllib(L, 'hjb_rollout_run_attitude', rv, int32(m - 1), int32(K), int32(zeros(1, K)), int64(n), ...
                  double(X0s), Xf, [], Xp, Up, Ap, ms), rv);
    X = permute(reshape(Xp.Value, n, 7, N), [2 3 1]);
    U = zeros(3, N, n);
    U(:, 1:K, :) = permute(reshape(Up.Value, n, 3, K), [2 3 1]);
    A = permute(reshape(Ap.Value, n, 3, K), [2 3 1]);             % yaw, pitch, roll (rad)
    X_ANGLES = zeros(9, N, n);
    X_ANGLES(:, 1:K, :) = [X(1:3, 1:K, :); rad2deg(A([3 2 1], :, :)); U(:, 1:K, :)];

    function check(st, obj_)
        if st == 0, return; end
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', obj_), calllib(L, 'hjb_status_string', int32(st)));
    end
end
