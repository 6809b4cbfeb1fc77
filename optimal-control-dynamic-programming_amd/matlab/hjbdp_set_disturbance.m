function hjbdp_set_disturbance(h, offsets, weights, mode)
%HJBDP_SET_DISTURBANCE  Put a disturbance on a libhjbdp handle (hjbdp.h hjb_set_disturbance, kernel variant 8): every stage the
%   handle launches afterwards - hjb_solve_flat, hjb_backup_stage(_device), hjb_evaluate* - forms
%     J_k(x) = min_u g(x,u) + sum_w p_w F_{k+1}(x_next(x,u) + d_w)     mode 'expect' (weights p; [] = 1/W each)
%     J_k(x) = min_u g(x,u) + max_w     F_{k+1}(x_next(x,u) + d_w)     mode 'worst'  (weights must be [])
%
%   hjbdp_set_disturbance(h, offsets, weights, mode)
%     h        the handle (hjb_create_from's void pointer, library 'libhjbdp' loaded: hjbdp_solve.m does both)
%     offsets  [D x W] double, column w = node w's offset d_w, row a = state axis a AS THE HANDLE RUNS IT
%              (hjbdp_solve's 'disturbance' pair permutes the rows for a relabelled problem); W <= 128
%     weights  [W] non-negative, or []
%   hjbdp_set_disturbance(h, [], [], 'expect') detaches: the handle is back to the nominal backup, same bits as before.
    L = 'libhjbdp';
    switch mode
        case 'expect', md = 0;
        case 'worst',  md = 1;
        otherwise, error('hjbdp:arg', 'mode must be expect or worst');
    end
    W = size(offsets, 2);
    if isempty(offsets), W = 0; offsets = []; end
    if isempty(weights), wts = []; else, wts = double(weights(:)); end
    st = calllib(L, 'hjb_set_disturbance', h, int32(md), int32(W), double(offsets(:)), wts);
    if st ~= 0
        error('hjbdp:status', '%s (%s)', calllib(L, 'hjb_last_error', h), calllib(L, 'hjb_status_string', int32(st)));
    end
end
