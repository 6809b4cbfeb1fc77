function out = hjbdp_evaluate(prob, labels, n_stages, varargin)
%HJBDP_EVALUATE  The cost of a GIVEN policy over the whole grid, on an AMD MI355X GPU through libhjbdp's FLAT C API
%   (include/hjbdp_matlab.h; the same builder calls as hjbdp_solve.m, then hjb_evaluate instead of hjb_solve_flat):
%
%       J_k(x) = g(x, u_k(x)) + F_{k+1}(x_next(x, u_k(x)))          no min: u_k is given
%
%   out = hjbdp_evaluate(prob, labels, n_stages, 'terminal', [], 'keep_stages', true, 'device', 0)
%
%   What the reference's solvers cannot say: they keep only the LAST stage's labels and fly that one table for the whole horizon
%   (position-control/Solver_position.m:144-146, attitude-control/Solver_attitude.m:249-251, pos-att/Solver_pos_att.m:288-296:
%   U1_Opt = griddedInterpolant(..., 'nearest')), while F.Values is the cost of the time-varying optimum.  With labels = that
%   table this returns the cost of the controller actually flown, from every grid point, over n_stages stages; with another
%   prob (fuel only, other Q / R) the same labels are judged under a cost they were not built for.
%   prob: the struct hjbdp_solve takes (knots, m, next_terms, cost_terms, single; prob.terminal is used unless 'terminal' is given).
%         A prob.model (HJB_MODEL_QUAT_EULER321) is refused by the library.
%   labels: 1-based labels as hjbdp_solve returns them (out.idx, out.idx_stages): [nS] or the grid's own shape = ONE stationary
%         policy used at every stage; [nS x n_stages] = stage k_s reads column k_s.  Class uint8 / uint16 / int32 is kept (and is
%         the storage class inside the library); anything else goes in as int32.  Every label must lie in 1 .. prod(m): the
%         library checks the whole array before any device work and touches no output otherwise.
%   The axes run in the caller's own order (no 'fast_axes' relabelling: the labels are tied to the grid as given); per state the
%   value is bit-identical to the candidate the stage kernels compare for that control, so hjbdp_evaluate on
%   hjbdp_solve(..., 'fast_axes', false, 'keep_stages', true)'s own idx_stages reproduces its J_stages.
%   'double_tables' / 'double_cost': as in hjbdp_solve (hjbdp.h HJB_TAB_F64 / HJB_COST_F64).
%   out: J [grid shape] (the last stage computed, k_s = 1), with keep_stages J_stages [nS x n_stages] (stage k_s in column k_s),
%        sweep_ms (device time of the loop).
    p = inputParser;
    addParameter(p, 'terminal', []);
    addParameter(p, 'keep_stages', false);
    addParameter(p, 'device', 0);
    addParameter(p, 'double_tables', false);
    addParameter(p, 'double_cost', false);
    parse(p, varargin{:});
    o = p.Results;
    L = 'libhjbdp';
    if ~libisloaded(L)
        here = fileparts(mfilename('fullpath'));
        loadlibrary(fullfile(here, '..', 'hjbdp', 'libhjbdp.so'), fullfile(here, '..', '..', 'include', 'hjbdp_matlab.h'), 'alias', L);
    end
    D = numel(prob.knots);  C = numel(prob.m);
    if prob.single, cls = 'single'; ptr = 'singlePtr'; dt = 0; else, cls = 'double'; ptr = 'doublePtr'; dt = 1; end
    n = cellfun(@numel, prob.knots);
    nS = prod(double(n));
    switch class(labels)
        case 'uint8',  idt = 1;  icls = 'uint8';
        case 'uint16', idt = 2;  icls = 'uint16';
        otherwise,     idt = 0;  icls = 'int32';
    end
    if numel(labels) == nS
        per_stage = 0;
    elseif numel(labels) == nS * n_stages
        per_stage = 1;
    else
        error('hjbdp:arg', 'labels: %d elements, expected %d (stationary) or %d (one column per stage)', numel(labels), nS, nS * n_stages);
    end
    lab = cast(labels(:), icls);
    b = libpointer('voidPtrPtr');
    check(calllib(L, 'hjb_problem_new', int32(D), int32(C), int32(n), int32(prob.m), int32(dt), int32(1), b), [], 'builder');
    bv = b.Value;
    freeb = onCleanup(@() calllib(L, 'hjb_problem_free', bv));
    ncls = cls;  ccls = cls;
    if (o.double_tables || o.double_cost) && ~prob.single, error('hjbdp:arg', 'double_tables / double_cost are for prob.single = true'); end
    if o.double_tables || idt ~= 0
        check(calllib(L, 'hjb_problem_set_types', bv, int32(idt), int32(o.double_tables)), bv, 'builder');   % HJB_IDX_*, HJB_TAB_F64
    end
    if o.double_tables, ncls = 'double'; end
    if o.double_cost
        check(calllib(L, 'hjb_problem_set_cost_type', bv, int32(1)), bv, 'builder');          % HJB_COST_F64
        ccls = 'double';
    end
    mask = @(dims) uint32(sum(bitshift(1, dims - 1)));
    for a = 1:D
        check(calllib(L, 'hjb_problem_set_knots', bv, int32(a - 1), double(prob.knots{a}(:)), int32(n(a))), bv, 'builder');
        T = prob.next_terms{a};
        for k = 1:numel(T)
            v = cast(T(k).data(:), ncls);
            check(calllib(L, 'hjb_problem_add_next_term', bv, int32(a - 1), mask(T(k).dims), v, int64(numel(v))), bv, 'builder');
        end
    end
    for k = 1:numel(prob.cost_terms)
        v = cast(prob.cost_terms(k).data(:), ccls);
        check(calllib(L, 'hjb_problem_add_cost_term', bv, mask(prob.cost_terms(k).dims), v, int64(numel(v))), bv, 'builder');
    end
    term = o.terminal;
    if isempty(term) && isfield(prob, 'terminal'), term = prob.terminal; end
    if ~isempty(term), term = cast(term(:), cls); end
    h = libpointer('voidPtrPtr');
    check(calllib(L, 'hjb_create_from', bv, int32(o.device), h), bv, 'builder');
    hv = h.Value;
    freeh = onCleanup(@() calllib(L, 'hjb_destroy', hv));
    Jf = libpointer(ptr, zeros(nS, 1, cls));
    Js = [];
    if o.keep_stages, Js = libpointer(ptr, zeros(nS * n_stages, 1, cls)); end
    ms = libpointer('doublePtr', 0);
    check(calllib(L, 'hjb_evaluate', hv, int32(n_stages), term, lab, int32(per_stage), Jf, Js, ms), hv, 'handle');
    shape = double(n);  if D == 1, shape = [shape 1]; end
    out.J = reshape(Jf.Value, shape);
    if o.keep_stages, out.J_stages = reshape(Js.Value, [nS, n_stages]); end
    out.sweep_ms = ms.Value;

    function check(st, obj, kind)
        if st == 0, return; end
        switch kind
            case 'builder', msg = calllib(L, 'hjb_problem_last_error', obj);
            otherwise,      msg = calllib(L, 'hjb_last_error', obj);
        end
        error('hjbdp:status', '%s (%s)', msg, calllib(L, 'hjb_status_string', int32(st)));
    end
end
