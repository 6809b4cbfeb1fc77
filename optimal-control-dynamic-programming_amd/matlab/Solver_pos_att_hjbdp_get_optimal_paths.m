function [T, X, F_Th_Opt, Force_Moment] = Solver_pos_att_hjbdp_get_optimal_paths(obj, X0s, substeps, channel_x_file)
%SOLVER_POS_ATT_HJBDP_GET_OPTIMAL_PATHS  get_optimal_path (pos-att/Solver_pos_att.m:452-730, without the plots) for many initial
% states at once, on the GPU (hjb_rollout_set_pos_att_model / hjb_rollout_run_pos_att, include/hjbdp.h):
%   pa = Solver_pos_att;  Solver_pos_att_hjbdp_simplified_run(pa);  [T, X, F, FM] = Solver_pos_att_hjbdp_get_optimal_paths(pa, X0s)
% X0s: [13, n], one state X = [x(3) v(3) q(4) w(3)] (q4 scalar) per column (default: the reference's X0, :457-466).
% T: [N, 1]; X: [N, 13, n]; F_Th_Opt: [N, 12, n]; Force_Moment: [N, 6, n] = [a_x a_y a_z U_M] (:502), last rows 0 as in the
% reference; N = obj.N_stage.  substeps (default 1): classical RK4 steps of h / substeps per stage with the forces held, in place
% of ode45 - at the reference's h = 0.005 s both integrators sit at round-off (the Python twin's test holds them together to
% 1e-12 over the whole horizon).  channel_x_file (default 'channel_x_controller_1.mat'): pass
% 'channel_x_controller_1_failure.mat' to simulate the failed thruster.  The three controllers are the files
% calculate_one_channel_U_Opt saved (:289, :470-473): labels U_Optimal_id as uint8, thruster table [f0 f1 f6 f7]_allcomb.
% The orbit table comes from the reference's own update_RV_target (:755-782) at the node times j * h / (2 * substeps).
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/solver_pos_att.py get_optimal_paths.
    global mu
    mu = 398600;                                                  % :454
    if nargin < 2 || isempty(X0s)
        q0 = angle2quat(deg2rad(0), deg2rad(3), deg2rad(0));     % :462-463
        X0s = [-0.1 0 0, 0 0 0, q0(end:-1:1), 0 0 0].';
    end
    if nargin < 3 || isempty(substeps), substeps = 1; end
    if nargin < 4 || isempty(channel_x_file), channel_x_file = 'channel_x_controller_1.mat'; end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = obj.N_stage;  K = N - 1;  n = size(X0s, 2);  S = substeps;
    files = {channel_x_file, 'channel_y_controller_1.mat', 'channel_z_controller_1.mat'};
    rv = cell(1, 3);
    cleanup = cell(1, 3);
    for c = 1:3
        Cc = load(files{c});
        knots = Cc.F_gI.GridVectors;
        n_k = int32(cellfun(@numel, knots));
        kcat = cell2mat(cellfun(@(k) double(k(:)), knots(:), 'UniformOutput', false));
        labels = uint8(Cc.U_Optimal_id(:));
        u_table = double([Cc.f0_allcomb(:), Cc.f1_allcomb(:), Cc.f6_allcomb(:), Cc.f7_allcomb(:)]);
        ro = libpointer('voidPtrPtr');
        check(calllib(L, 'hjb_rollout_create', int32(0), int32(4), n_k, kcat, int32(1), int32(1), ...
                      int32(1), labels, int32(size(u_table, 1)), int32(4), u_table(:), ro), []);     % HJB_IDX_U8, 1-based, one plane
        rv{c} = ro.Value;
        cleanup{c} = onCleanup(@() calllib(L, 'hjb_rollout_destroy', ro.Value));
    end
    % the five scalars of t the right-hand side needs (:695-715), at the nodes of the fixed-step integrator
    [R0, V0] = get_target_R0V0(obj);                             % :482
    rsw = RSW2ECI(obj, R0, V0);
    n_nodes = 2 * S * K + 1;
    coef = zeros(5, n_nodes);
    for j = 0:n_nodes - 1
        [R, V] = update_RV_target(obj, R0, V0, j * obj.h / (2 * S));
        nR = (R * R.')^.5;  RdV = sum(R .* V);  Hn = norm(cross(R, V));
        coef(:, j + 1) = [2 * mu / nR^3 + Hn^2 / nR^4; 2 * RdV / nR^4 * Hn; 2 * Hn / nR^2; mu / nR^3 - Hn^2 / nR^4; mu / nR^3];
    end
    check(calllib(L, 'hjb_rollout_set_pos_att_model', rv{1}, rv{2}, rv{3}, double(obj.InertiaM(:)), double(obj.Mass), ...
                  double(obj.T_dist), double(obj.h), int32(S), double(rsw(:)), int32(n_nodes), coef(:)), rv{1});
    Xf = libpointer('doublePtr', zeros(13, n));
    Xp = libpointer('doublePtr', zeros(n, 13, N));  Fp = libpointer('doublePtr', zeros(n, 12, K));
    FMp = libpointer('doublePtr', zeros(n, 6, K));
    check(calllib(L, 'hjb_rollout_run_pos_att', rv{1}, int32(K), int32(zeros(1, K)), int64(n), double(X0s), Xf, Xp, Fp, FMp), rv{1});
    T = (0:K).' * obj.h;
    X = permute(reshape(Xp.Value, n, 13, N), [3 2 1]);
    F_Th_Opt = zeros(N, 12, n);
    F_Th_Opt(1:K, :, :) = permute(reshape(Fp.Value, n, 12, K), [3 2 1]);
    Force_Moment = zeros(N, 6, n);
    Force_Moment(1:K, :, :) = permute(reshape(FMp.Value, n, 6, K), [3 2 1]);

    function check(st, obj_)
        if st == 0, return; end
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', obj_), calllib(L, 'hjb_status_string', int32(st)));
    end
end
