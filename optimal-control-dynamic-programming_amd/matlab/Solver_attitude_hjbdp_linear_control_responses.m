function [X, U, XANGLES, cost] = Solver_attitude_hjbdp_linear_control_responses(obj, X0s, T_final, dt, K, C, qc, u_limit, cost_form, weights)
%SOLVER_ATTITUDE_HJBDP_LINEAR_CONTROL_RESPONSES  linear_control_response (attitude-control/Solver_attitude.m:508-591, without the
% plots) for many initial attitudes at once, on the GPU (hjb_attitude_linear_response, include/hjbdp.h):
%   sa = Solver_attitude;  [X, U, XANGLES] = Solver_attitude_hjbdp_linear_control_responses(sa, X0s)
% The call is stateless: it needs neither run() nor simplified_run(), and creates no library object.
% X0s: [7, n], one state X = [w1 w2 w3 q1 q2 q3 q4] (q4 scalar) per column (default: obj.defaultX0).
% T_final, dt: as the reference's (defaults obj.T_final, obj.h); N = round(T_final / dt) steps.
% K, C: [3, 3] gains of U = -K*qe(1:3) - C*w (defaults 0.2*eye(3), eye(3), :523-528); qc: [4, 4], qe = qc*q (default eye(4), :519-522).
% u_limit: [3, 1] >= 0, the torques are clipped to +-u_limit ([] = no limit, the reference's law).
% cost_form, weights: 0 with weights = [q(7); r(3)], the stage cost of hjb_rollout_run_attitude, or 1 with weights =
%   [qw(3); qt(3); r(3); 0], that of hjb_rollout_run_attitude_simplified ([] = zeros).
% X: [7, N+1, n]; U: [3, N, n]; XANGLES: [3, N, n] = yaw, pitch, roll in radians of quat2angle([X7 X6 X5 X4]) (:540) from the
% library's fixed atan2 / asin (<= 2 ulp of libm); cost: [n, 1].  The plant is next_stage_states(., 'RK4') operation for operation.
% NOT executed in the build image (no MATLAB); tested twin: hjbdp/solver_attitude.py linear_control_responses.
    if nargin < 2 || isempty(X0s), X0s = obj.defaultX0(:); end
    if nargin < 3 || isempty(T_final), T_final = obj.T_final; end
    if nargin < 4 || isempty(dt), dt = obj.h; end
    if nargin < 5 || isempty(K), K = 0.2 * eye(3); end
    if nargin < 6 || isempty(C), C = eye(3); end
    if nargin < 7 || isempty(qc), qc = eye(4); end
    if nargin < 8, u_limit = []; end
    if nargin < 9 || isempty(cost_form), cost_form = 0; end
    if nargin < 10, weights = []; end
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    N = round(T_final / dt);  n = size(X0s, 2);
    inertia = double([obj.J1 obj.J2 obj.J3]);
    if isempty(u_limit), lim = libpointer('doublePtr'); else, lim = double(u_limit(:)); end        % a null pointer: no limit
    if isempty(weights), wts = libpointer('doublePtr'); else, wts = double(weights(:)); end
    Xf = libpointer('doublePtr', zeros(7, n));  Cp = libpointer('doublePtr', zeros(n, 1));
    Xp = libpointer('doublePtr', zeros(n, 7, N + 1));  Up = libpointer('doublePtr', zeros(n, 3, N));
    Ap = libpointer('doublePtr', zeros(n, 3, N));  ms = libpointer('doublePtr', 0);
    st = calllib(L, 'hjb_attitude_linear_response', int32(0), inertia, double(dt), int32(1), double(K(:)), double(C(:)), double(qc(:)), ...
                 lim, int32(cost_form), wts, int32(N), int64(n), double(X0s), Xf, Cp, Xp, Up, Ap, int64(0), ms);      % device 0, RK4
    if st ~= 0
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_rollout_last_error', []), calllib(L, 'hjb_status_string', int32(st)));
    end
    X = permute(reshape(Xp.Value, n, 7, N + 1), [2 3 1]);
    U = permute(reshape(Up.Value, n, 3, N), [2 3 1]);
    XANGLES = permute(reshape(Ap.Value, n, 3, N), [2 3 1]);
    cost = Cp.Value(:);
end
