function [T, X, U, ANG, cost] = Solver_attitude_hjbdp_get_optimal_paths_simplified(obj, X0s, substeps, dynamics)
%SOLVER_ATTITUDE_HJBDP_GET_OPTIMAL_PATHS_SIMPLIFIED  get_optimal_path_simplified_testode45 (attitude-control/Solver_attitude.m:835-925,
% without the plots) for many initial attitudes at once, on the GPU (hjb_rollout_set_attitude_simplified_model /
% hjb_rollout_run_attitude_simplified, include/hjbdp.h):
%   sa = Solver_attitude;  Solver_attitude_hjbdp_simplified_run(sa);  [T, X, U, ANG] = Solver_attitude_hjbdp_get_optimal_paths_simplified(sa, X0s)
% X0s: [7, n], one state X = [w1 w2 w3 q1 q2 q3 q4] (q4 scalar) per column (default: obj.defaultX0).
% T: [N, 1]; X: [N, 7, n]; U: [N, 3, n] (the torques each stage applied; last row 0); ANG: [N, 3, n] = yaw, pitch, roll in degrees
% from quat2angle([X7 X6 X5 X4]) (:856; last row 0); cost: [n, 1], the 2-D sweeps' stage cost (:220) summed along the path with
% (Q1..3, Qt1..3, R1..3); N = obj.N_stage.
% dynamics 0 (default): the full inertia matrix with `substeps` (default 1) classical RK4 steps of h / substeps per stage in place of
%   ode45, the torques held, quaternion not renormalised.  Against a Dormand-Prince 5(4) stage integrator this differs by RK4's
%   truncation error: max |dX| 4.9e-13 over the 5,999 stages at substeps 1, 1.4e-14 at substeps 2 (measured by the Python twin's
%   test with a switching policy on the default grids, every torque equal); MATLAB's own ode45 differs from that integrator by more.
% dynamics 1: the development script's loop (test/test_simplified.m:188-218): diag(InertiaM), one RK4 step per stage, q / |q| -
%   the reference's own arithmetic; substeps must be 1.
% The three policies are the griddedInterpolants simplified_run leaves (obj.U1_Opt .. U3_Opt over {s_w, s_t}, :249-251); their
% Values are mapped back to 1-based labels into obj.U_vector.
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/solver_attitude.py get_optimal_paths_simplified.
    if nargin < 2 || isempty(X0s), X0s = obj.defaultX0(:); end
    if nargin < 3 || isempty(substeps), substeps = 1; end
    if nargin < 4 || isempty(dynamics), dynamics = 0; end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = obj.N_stage;  K = N - 1;  n = size(X0s, 2);
    pol = {obj.U1_Opt, obj.U2_Opt, obj.U3_Opt};
    u_table = double(obj.U_vector(:));
    rv = cell(1, 3);
    cleanup = cell(1, 3);
    for c = 1:3
        knots = pol{c}.GridVectors;
        n_k = int32(cellfun(@numel, knots));
        kcat = cell2mat(cellfun(@(k) double(k(:)), knots(:), 'UniformOutput', false));
        [~, lab] = min(abs(double(pol{c}.Values(:)) - u_table.'), [], 2);      % the label of each stored torque
        ro = libpointer('voidPtrPtr');
        check(calllib(L, 'hjb_rollout_create', int32(0), int32(2), n_k, kcat, int32(1), int32(1), ...
                      int32(1), uint8(lab), int32(numel(u_table)), int32(1), u_table, ro), []);      % HJB_IDX_U8, 1-based, one plane
        rv{c} = ro.Value;
        cleanup{c} = onCleanup(@() calllib(L, 'hjb_rollout_destroy', ro.Value));
    end
    qw = double([obj.Q1 obj.Q2 obj.Q3]);  qt = double([obj.Qt1 obj.Qt2 obj.Qt3]);  r = double([obj.R1 obj.R2 obj.R3]);
    check(calllib(L, 'hjb_rollout_set_attitude_simplified_model', rv{1}, rv{2}, rv{3}, double(obj.InertiaM(:)), double(obj.h), ...
                  int32(substeps), int32(dynamics), qw, qt, r), rv{1});
    Xf = libpointer('doublePtr', zeros(7, n));  Cp = libpointer('doublePtr', zeros(n, 1));
    Xp = libpointer('doublePtr', zeros(n, 7, N));  Up = libpointer('doublePtr', zeros(n, 3, K));
    Ap = libpointer('doublePtr', zeros(n, 3, K));
    check(calllib(L, 'hjb_rollout_run_attitude_simplified', rv{1}, int32(K), int32(zeros(1, K)), int64(n), double(X0s), Xf, Cp, Xp, Up, ...
                  Ap), rv{1});
    T = (0:K).' * obj.h;
    X = permute(reshape(Xp.Value, n, 7, N), [3 2 1]);
    U = zeros(N, 3, n);
    U(1:K, :, :) = permute(reshape(Up.Value, n, 3, K), [3 2 1]);
    cost = Cp.Value(:);
    ANG = zeros(N, 3, n);
    for i = 1:n
        [yaw, pitch, roll] = quat2angle([X(1:K, 7, i), X(1:K, 6, i), X(1:K, 5, i), X(1:K, 4, i)]);     % :856
        ANG(1:K, :, i) = rad2deg([yaw, pitch, roll]);
    end

    function check(st, obj_)
        if st == 0, return; end
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', obj_), calllib(L, 'hjb_status_string', int32(st)));
    end
end
