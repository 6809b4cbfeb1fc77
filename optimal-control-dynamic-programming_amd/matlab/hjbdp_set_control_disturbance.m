function hjbdp_set_control_disturbance(h, offsets, weights, mode)
%HJBDP_SET_CONTROL_DISTURBANCE  Put a control-dependent disturbance on a libhjbdp handle (hjbdp.h hjb_set_control_disturbance,
%   kernel variant 8 in its per-control form): every stage the handle launches afterwards - hjb_solve_flat,
%   hjb_backup_stage(_device), hjb_evaluate* - forms
%     J_k(x) = min_l g(x,u_l) + sum_w p_w F_{k+1}(x_next(x,u_l) + d_w(l))     mode 'expect' (weights p; [] = 1/W each)
%     J_k(x) = min_l g(x,u_l) + max_w     F_{k+1}(x_next(x,u_l) + d_w(l))     mode 'worst'  (weights must be [])
%   - actuator noise x+ = A x + B (u .* (1 + eps_w)) is d_w(l) = B * (u_l .* eps_w).
%
%   hjbdp_set_control_disturbance(h, offsets, weights, mode)
%     h        the handle (hjb_create_from's void pointer, library 'libhjbdp' loaded: hjbdp_solve.m does both)
%     offsets  [D x W x nU] double: offsets(:, w, l) = node w's offset under the control with column-major label l
%              (the label hjb_solve_flat writes with index_base 1), row a = state axis a AS THE HANDLE RUNS IT; W <= 128,
%              nU = the handle's number of controls (a table of another size is refused)
%     weights  [W] non-negative, or []
%   hjbdp_set_control_disturbance(h, [], [], 'expect') detaches, as hjbdp_set_disturbance does: the two settings replace each other.
    L = 'libhjbdp';
    switch mode
        case 'expect', md = 0;
        case 'worst',  md = 1;
        otherwise, error('hjbdp:arg', 'mode must be expect or worst');
    end
    W = size(offsets, 2);
    nU = size(offsets, 3);
    if isempty(offsets), W = 0; nU = 0; offsets = []; end
    if isempty(weights), wts = []; else, wts = double(weights(:)); end
    st = calllib(L, 'hjb_set_control_disturbance', h, int32(md), int32(W), int32(nU), double(offsets(:)), wts);
    if st ~= 0
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_last_error', h), calllib(L, 'hjb_status_string', int32(st)));
    end
end
