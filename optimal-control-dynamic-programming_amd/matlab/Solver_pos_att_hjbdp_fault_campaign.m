function out = Solver_pos_att_hjbdp_fault_campaign(obj, X0s, fault_mask, fault_stage, switch_stage, pos_tol, att_tol, substeps)
%SOLVER_POS_ATT_HJBDP_FAULT_CAMPAIGN  The scenario channel_x_controller_1_failure was solved for (pos-att/Solver_pos_att.m:235-240):
% the closed loop of get_optimal_path (pos-att/Solver_pos_att.m:452-730, without the plots) for many initial states at once on the
% GPU, in which, per trajectory, thrusters die in the plant and channel x is handed over from channel_x_controller_1 to
% channel_x_controller_1_failure (hjb_rollout_set_pos_att_fault_controller / hjb_rollout_run_pos_att_faults, include/hjbdp.h):
%   pa = Solver_pos_att;  Solver_pos_att_hjbdp_simplified_run(pa);
%   out = Solver_pos_att_hjbdp_fault_campaign(pa, X0s, 1, 200, 400, 0.05, 0.02)     % f0 dead from stage 200, hand-over at 400
% X0s: [13, n], one state X = [x(3) v(3) q(4) w(3)] (q4 scalar) per column (default: the reference's X0, :457-466).
% fault_mask (bit j = thruster j, default 0), fault_stage (default 0), switch_stage (default: never): scalars or [1, n], 0-based
% stages; a stage >= N - 1 never comes.  pos_tol, att_tol (default Inf): the settling radii on |x(1:3)| and |q(1:3)|.
% out.X_final [13, n]; out.impulse [n, 1] = h * sum over stages and thrusters of |applied force|; out.settle_stage [n, 1]: the
% first state index (0-based) from which the path stays inside both radii to the end, N when the last state is outside;
% out.device_ms: the kernels' time.  Paths are not kept (a campaign of 10^5 starts cannot keep them; pass non-empty pointers
% laid out as Solver_pos_att_hjbdp_get_optimal_paths does to get them: F_path then holds the APPLIED forces).
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/solver_pos_att.py get_fault_campaign.
    global mu
    mu = 398600;                                                  % :454
    if nargin < 2 || isempty(X0s)
        q0 = angle2quat(deg2rad(0), deg2rad(3), deg2rad(0));     % :462-463
        X0s = [-0.1 0 0, 0 0 0, q0(end:-1:1), 0 0 0].';
    end
    N = obj.N_stage;  K = N - 1;  n = size(X0s, 2);
    if nargin < 3 || isempty(fault_mask), fault_mask = 0; end
    if nargin < 4 || isempty(fault_stage), fault_stage = 0; end
    if nargin < 5 || isempty(switch_stage), switch_stage = K; end
    if nargin < 6 || isempty(pos_tol), pos_tol = Inf; end
    if nargin < 7 || isempty(att_tol), att_tol = Inf; end
    if nargin < 8 || isempty(substeps), substeps = 1; end
    S = substeps;
    per_traj = @(v) int32(repmat(v(:).', 1, n / numel(v)));      % scalars broadcast over the starts
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    % nominal x, y, z and the failure controller of channel x (:235-240)
    files = {'channel_x_controller_1.mat', 'channel_y_controller_1.mat', 'channel_z_controller_1.mat', 'channel_x_controller_1_failure.mat'};
    rv = cell(1, 4);
    cleanup = cell(1, 4);
    for c = 1:4
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
    check(calllib(L, 'hjb_rollout_set_pos_att_fault_controller', rv{1}, rv{4}), rv{1});
    Xf = libpointer('doublePtr', zeros(13, n));
    imp = libpointer('doublePtr', zeros(n, 1));
    settle = libpointer('int32Ptr', zeros(n, 1, 'int32'));
    ms = libpointer('doublePtr', 0);
    check(calllib(L, 'hjb_rollout_run_pos_att_faults', rv{1}, int32(K), int32(zeros(1, K)), int64(n), double(X0s), ...
                  per_traj(fault_mask), per_traj(fault_stage), per_traj(switch_stage), double(pos_tol), double(att_tol), ...
                  Xf, imp, settle, [], [], [], ms), rv{1});
    out = struct('X_final', reshape(Xf.Value, 13, n), 'impulse', imp.Value, 'settle_stage', settle.Value, 'device_ms', ms.Value);

    function check(st, obj_)
        if st == 0, return; end
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', obj_), calllib(L, 'hjb_status_string', int32(st)));
    end
end
