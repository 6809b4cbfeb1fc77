"""Constructed problems for K10 (k_backup_colsweep, variant 7: csrc/kernels_colsweep.h with its body and step files) and a numpy
restatement of what its host side decides (not reference code: generators of inputs, and the rules of csrc/hjbdp_colsweep.hip and
csrc/hjbdp_choose.hip written out again from their definitions - nothing here calls the library).

shape_problem builds a variant-7 problem by construction: D = 4, one control dim, integer knots on every axis, every next-state move
and every cost term a multiple of 1/8 - so queries, cells and weights are the same numbers in float32 and float64 (tables_exact) and
one stage from lattice_terminal is exact in float32 (one_stage_exact proves it per case).  The caller gives, per (group-axis index,
window-axis index, control), the CELL the control lands in on the group axis and on the window axis: a column's plan - its groups,
which window pair each control takes, which slots are late - is then chosen, not met.  Axis 0 takes a shift per i0 (and per i2, i3):
one chosen state can sit in another cell than its chunk.  Axis 1 takes a shift per i1 (and per index of one other dim): a chosen
step repeats a cell or jumps two.

The restatements: plan_of (colsweep_plan), pick_of (the group-axis rule of ensure_colsweep), dpp_of (colsweep_dpp_ok and the kernel's
own kb / odd-state rule), split_of (colsweep_split and the part bounds), xcd_of (colsweep_map's eight counts), grid_of (choose_launch),
cost_record_of / cost_form_of (the cost record and Launch::cost_form), auto_variant_of, instantiation_of, coverage.

CASES registers the problems tests/test_colsweep_shapes.py (no device) and tests/test_gpu_colsweep_shapes.py run.

Every case registers the conditions it is there for (Case.reaches); tests/test_colsweep_shapes.py asserts them case by case.

Sizes: n0 is 8, 60, 61, 64 or 121 (a partial chunk, exactly one chunk, a chunk of one state behind a full one, a partial chunk behind
a full one, two full chunks and one state) and 62 where a chunk of TWO states is wanted - the only chunk whose kb tie keeps the
first state's value and is still admitted; n1 is 4 to 9; the group axis has at most 15 knots and the window axis 3 to 9 (9: nine
indices on the split axis under cs_xcd_axis 1).  pick-none alone has 15 knots on both axes 2 and 3: seven distinct cells two apart
on either axis are what makes both plans fail.  No case has more than 1e5 states.

Not pinned on the device: the ORDER of colsweep_map's index table (xcd_of returns it for reference; only its eight counts reach a
readback, through the grid - the results under each cs_xcd_mod being bit-equal says the table lists every index once)."""
from __future__ import annotations

import numpy as np

from hjbdp import ProblemSpec, Term

K_GMAX = 6                              # groups per column (kCsGMax)
K_MMAX = 6                              # member slots per group, three per window pair (kCsMMax)
K_PS = K_MMAX // 2
K_UMAX = 16                             # controls (kCsUMax)
K_MAXCU = 4                             # control-only cost terms (kCsMaxCu)
LANES = 60                              # states per wave in the one-load form (kCsDppLanes)


# ---- the problems -----------------------------------------------------------------------------------------------------------------
# cost shapes: (dims of the leading column terms, dims of the per-step terms, control-only terms).  The first four are those of
# problems.colsweep_problem.
COSTS = {
    "fast": (((0,), (2,), (3,)), ((1,),), 1),
    "step01": ((), ((0, 1), (2,), (3,)), 1),            # nothing is column-invariant, the step terms are not wave-uniform
    "multi": (((0,),), ((1,), (3,)), 2),
    "ctrl_only": ((), (), 1),                           # npre == 0
    "col0": ((), ((1,),), 1),
    "col1": (((0,),), ((1,),), 1),
    "col4": (((0,), (2,), (3,), (0, 2)), ((1,),), 1),   # four column terms: the cost record stops holding them
    "two_step": (((0,),), ((1,), (1, 2)), 1),           # two wave-uniform per-step terms: no single-term shortcut
    "no_step": (((0,), (2,)), (), 1),
    "cu0": (((0,),), ((1,),), 0),
    "cu4": (((0, 3),), ((1,),), K_MAXCU),
    "ctrl_only2": ((), (), 2),
    "cu5": (((0,),), ((1,),), K_MAXCU + 1),             # refused
}


def _reduced(table):
    """A table over (i2, i3, control) without the state dims it does not vary along -> (dims, data)."""
    dims, t = [], table
    for a in (2, 3):
        if t.shape[len(dims)] > 1 and np.ptp(t, axis=len(dims)).any():
            dims.append(a)
        else:
            t = np.take(t, 0, axis=len(dims))
    return tuple(dims) + (4,), t


def shape_problem(n, gax, cg, cw, tg=None, tw=None, a0=0.25, a0_s2=None, a0_s3=None, a1=0.375, a1_s=None, a1_dim=3, cost="fast",
                  seed=0, index_base=1):
    """n: the four sizes; gax: the axis (2 or 3) the controls are meant to be grouped by.  cg, cw [group-axis index, window-axis index,
    control] (broadcast): the cell a control's query has on the group and on the window axis (a cell outside 0 .. size - 2 is a query
    outside the grid: the library clamps it); tg, tw: the weights there, multiples of 1/8 (default: a pattern over column and control).
    a0 (scalar or per i0), a0_s2 [n2], a0_s3 [n3]: axis 0's query is i0 + a0[i0] + a0_s2[i2] + a0_s3[i3].  a1, a1_s over state dim
    a1_dim: the same for axis 1.  cost: a name of COSTS."""
    rng = np.random.default_rng(seed)
    n = tuple(int(x) for x in n)
    wax = 5 - gax
    n_g, n_w = n[gax], n[wax]
    cg, cw = np.asarray(cg), np.asarray(cw)
    nU = cg.shape[-1]
    full = (n_g, n_w, nU)
    cg, cw = np.broadcast_to(cg, full), np.broadcast_to(cw, full)
    ig, iw, iu = np.arange(n_g)[:, None, None], np.arange(n_w)[None, :, None], np.arange(nU)[None, None, :]
    if tg is None:
        tg = ((3 * iu + ig + 2 * iw + 1) % 8) / 8.0
    if tw is None:
        tw = ((5 * iu + 2 * ig + iw + 2) % 8) / 8.0
    mg = np.broadcast_to(cg + np.asarray(tg, dtype=np.float64) - ig, full)          # the move: query - own knot
    mw = np.broadcast_to(cw + np.asarray(tw, dtype=np.float64) - iw, full)
    assert np.array_equal(mg * 8, np.round(mg * 8)) and np.array_equal(mw * 8, np.round(mw * 8))
    if gax == 2:                                                                    # tables over (i2, i3, u)
        tabs = {2: mg, 3: mw}
    else:
        tabs = {3: np.swapaxes(mg, 0, 1), 2: np.swapaxes(mw, 0, 1)}
    knots = [np.arange(k, dtype=np.float64) for k in n]
    per = lambda v, k: np.broadcast_to(np.asarray(v, dtype=np.float64), (k,)).copy()
    nxt = [None] * 4
    nxt[0] = [Term((0,), knots[0] + per(a0, n[0]))]
    if a0_s2 is not None:
        nxt[0].append(Term((2,), per(a0_s2, n[2])))
    if a0_s3 is not None:
        nxt[0].append(Term((3,), per(a0_s3, n[3])))
    nxt[1] = [Term((1,), knots[1] + per(a1, n[1]))]
    if a1_s is not None:
        nxt[1].append(Term((a1_dim,), per(a1_s, n[a1_dim])))
    for a in (2, 3):
        dims, data = _reduced(tabs[a])
        nxt[a] = [Term((a,), knots[a].copy()), Term(dims, data)]
    g = n + (nU,)
    col, step, ncu = COSTS[cost]
    term = lambda dims, top: Term(dims, rng.integers(0, top, tuple(g[d] for d in dims)) / 8.0)
    ct = [term(d, 9) for d in col] + [term(d, 9) for d in step] + [term((4,), 4) for _ in range(ncu)]      # few control values: ties
    return ProblemSpec(knots, [nU], nxt, ct, dtype=np.float32, index_base=index_base)


def with_typing(spec, storage=None, cost64=False, idx_dtype=None, index_base=None, cost_terms=None):
    return ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms if cost_terms is None else cost_terms, dtype=np.float32,
                       index_base=spec.index_base if index_base is None else index_base, j_storage=storage, idx_dtype=idx_dtype,
                       cost_dtype=np.float64 if cost64 else None)


def tie_twin(spec, winner):
    """The same moves with ONE control-only cost term: 1 for the controls below `winner`, 0 from it on.  On a zero terminal every
    total of a state is that term alone: `winner` and every control after it tie, and the first of them must be returned."""
    cu = (np.arange(spec.nU) < winner).astype(np.float64)
    return with_typing(spec, storage=None if spec.j_dtype == spec.dtype else spec.j_dtype, idx_dtype=spec.idx_dtype,
                       cost_terms=[Term((4,), cu)])


def lattice_terminal(spec, seed=0):
    """Multiples of 1/8 in [0, 8): exact in float32 and in binary16."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 64, spec.nS) / 8.0).astype(spec.j_dtype)


# ---- cells and weights ----------------------------------------------------------------------------------------------------------------
def cells_and_weights(knots, q, dtype):
    """The library's rule in `dtype`: c = clip(upper_bound(k, q) - 1, 0, n - 2), t = (q - k[c]) * (1 / (k[c + 1] - k[c]))."""
    dt = np.dtype(dtype).type
    k = np.asarray(knots).astype(dt)
    c = np.clip(np.searchsorted(k, q, side="right") - 1, 0, len(k) - 2)
    rdx = (dt(1) / (k[1:] - k[:-1]).astype(dt)).astype(dt)
    return c, ((q - k[c]).astype(dt) * rdx[c]).astype(dt)


def axis_query(spec, a, dtype):
    """Axis a's queries, the terms' ordered sum in `dtype`, as an array over (n0, n1, n2, n3, nU) with 1 where it does not depend."""
    acc = None
    for t in spec.next_terms[a]:
        shape = [1] * 5
        for ax, d in enumerate(t.dims):
            shape[d] = t.data.shape[ax]
        x = np.asarray(t.data).astype(dtype).reshape(shape)
        acc = x if acc is None else (acc + x).astype(dtype)
    return acc


def axis_cells(spec, a, dtype=np.float32):
    return cells_and_weights(spec.knots[a], axis_query(spec, a, dtype), dtype)


def tables_exact(spec):
    """Queries, cells and weights of all four axes are the same numbers in float32 and float64, the weights multiples of 1/8."""
    for a in range(4):
        q32, q64 = axis_query(spec, a, np.float32), axis_query(spec, a, np.float64)
        c32, t32 = cells_and_weights(spec.knots[a], q32, np.float32)
        c64, t64 = cells_and_weights(spec.knots[a], q64, np.float64)
        if not (np.array_equal(q32.astype(np.float64), q64) and np.array_equal(c32, c64) and np.array_equal(t32.astype(np.float64), t64)):
            return False
        if not np.array_equal(t64 * 8, np.round(t64 * 8)):
            return False
    return True


def one_stage_exact(spec, terminal):
    """One stage on `terminal` is exact in float32.  The terminal and every cost term are multiples of 1/8 and so is every weight: a
    lerp a + t (b - a) of multiples of 2^-k is a multiple of 2^-(k + 3), the four lerps end on multiples of 2^-15 and the cost adds
    multiples of 2^-3.  With S = (sum over the cost terms of their largest magnitude) + max |terminal| x (product over the axes of the
    largest |1 - t| + |t|) below 2^9, every intermediate - the differences b - a included, which are multiples of a coarser lattice
    and below 2^10 - is an integer multiple of 2^-15 below 2^24 of them: a float32.  The result is then the float64 value, and its
    binary16 storage that value rounded once."""
    if not tables_exact(spec):
        return False
    term = np.asarray(terminal).astype(np.float64)
    if not np.array_equal(term * 8, np.round(term * 8)):
        return False
    S = 0.0
    for t in spec.cost_terms:
        x = np.asarray(t.data, dtype=np.float64)
        if not np.array_equal(x * 8, np.round(x * 8)):
            return False
        S += float(np.abs(x).max())
    w = 1.0
    for a in range(4):
        _, t = axis_cells(spec, a, np.float64)
        w *= float((np.abs(1.0 - t) + np.abs(t)).max())
    return S + w * float(np.abs(term).max()) < 2.0 ** 9


# ---- the shape rule -------------------------------------------------------------------------------------------------------------
def _axis_mask(spec, a):
    m = 0
    for t in spec.next_terms[a]:
        m |= t.mask
    return m


def cost_record_of(spec):
    """What ensure_colsweep and colsweep_upload take from the cost terms: npre (leading state-only terms), npre_col (those before the
    first that depends on state dim 1), step_uniform (none of the others depends on state dim 0), ncu, whether the cost record holds
    the column terms, and has_su (the record carries the one per-step term)."""
    smask = (1 << 4) - 1
    masks = [t.mask for t in spec.cost_terms]
    npre = next((k for k, m in enumerate(masks) if m & ~smask), len(masks))
    npre_col = next((k for k in range(npre) if masks[k] & 2), npre)
    step_uniform = all((masks[k] & 1) == 0 for k in range(npre_col, npre))
    c64 = spec.cost_dtype is not None
    holds = (not c64) and npre_col <= 3
    return {"npre": npre, "npre_col": npre_col, "step_uniform": step_uniform, "ncu": len(masks) - npre, "holds": holds,
            "has_su": int(holds and step_uniform and npre - npre_col == 1), "n_step": npre - npre_col, "c64": c64}


def shape_admitted(spec):
    """ensure_colsweep's rule on the problem's shape, before any plan: None, or why not."""
    cbit = 1 << 4
    if spec.D != 4 or spec.C != 1:
        return "D, C"
    if spec.nU > K_UMAX:
        return "controls"
    m = [_axis_mask(spec, a) for a in range(4)]
    if (m[0] & (cbit | 2)) or (m[1] & (cbit | 1)) or (m[2] & 3) or (m[3] & 3):
        return "axes"
    rec = cost_record_of(spec)
    if rec["ncu"] > K_MAXCU:
        return "control terms"
    if any(t.mask != cbit for t in spec.cost_terms[rec["npre"]:]):
        return "mixed cost term"
    return None


def cost_form_of(spec):
    """Launch::cost_form: 2 the usual shape summed in float64, 1 the usual shape (state terms + one control term), 0 general.
    None: float64 cost terms in another shape - variant 7 does not serve."""
    rec = cost_record_of(spec)
    usual = rec["ncu"] == 1 and rec["npre"] > 0
    if rec["c64"]:
        return 2 if usual else None
    return 1 if usual else 0


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def _column(cg, cw, nwk):
    """One column's groups from its controls' cells (group axis, window axis), in visiting order.  None: more than K_GMAX groups."""
    nU = len(cg)
    wmin, pulled = [], []
    for u in range(nU):
        same = sorted({cw[v] for v in range(nU) if cg[v] == cg[u]})     # greedy cover of this group cell's window cells by windows of two
        start = same[0]
        while cw[u] > start + 1:
            start = min(c for c in same if c > start + 1)
        pulled.append(start + 2 > nwk - 1)                             # three knots must exist: the last window starts one lower
        wmin.append(nwk - 3 if pulled[u] else start)
    groups = []
    for u in range(nU):
        pair = cw[u] - wmin[u]
        assert pair in (0, 1), (cw[u], wmin[u])
        for G in groups:
            if G["cell"] == cg[u] and G["wmin"] == wmin[u] and len(G["pairs"][pair]) < K_PS:
                break
        else:
            if len(groups) == K_GMAX:
                return None
            G = {"cell": cg[u], "wmin": wmin[u], "pairs": ([], []), "first": u, "pulled": False}
            groups.append(G)
        G["pairs"][pair].append(u)
        G["pulled"] = G["pulled"] or pulled[u]
    order = sorted(range(len(groups)), key=lambda g: max(groups[g]["pairs"][0] + groups[g]["pairs"][1]))     # (stable)
    out, seen = [], -1
    for g in order:
        G = groups[g]
        used = late = 0
        for p in range(2):
            for s, u in enumerate(G["pairs"][p]):
                used |= 1 << (K_PS * p + s)
                if u < seen:
                    late |= 1 << (K_PS * p + s)
                seen = max(seen, u)
        out.append({"cell": int(G["cell"]), "wmin": int(G["wmin"]), "slots": (tuple(G["pairs"][0]), tuple(G["pairs"][1])), "used": used,
                    "late": late, "first": G["first"], "pulled": G["pulled"]})
    return out


def plan_of(spec, gax, planes=None):
    """colsweep_plan restated.  planes = (begin, end, halo_lo, halo_hi): a slab of the last axis.  -> None where the builder refuses,
    else {"cols": {(i2, i3): {"groups", "ng", "halo"}}, "ng_max", "rows_total", "mid_rows"}; i3 counts the OWNED planes."""
    wax = 5 - gax
    n2, n3g = spec.n[2], spec.n[3]
    b, e, hl, hh = planes if planes is not None else (0, n3g, 0, 0)
    plane0, nplanes = b - hl, (e - b) + hl + hh
    nwk = nplanes if wax == 3 else spec.n[wax]
    if nwk < 3:
        return None
    cells = {}
    for a in (2, 3):
        c, _ = axis_cells(spec, a)
        cells[a] = np.broadcast_to(c, (1, 1, n2, n3g, spec.nU))[0, 0]
    cols, ng_max, rows_total = {}, 1, 0
    for i3 in range(e - b):
        for i2 in range(n2):
            c2 = [int(x) for x in cells[2][i2, b + i3]]
            c3, halo = [], 0
            for x in cells[3][i2, b + i3]:
                x = int(x) - plane0
                if x < 0 or x + 1 >= nplanes:
                    halo, x = 1, (0 if x < 0 else nplanes - 2)
                c3.append(x)
            groups = _column(c3 if gax == 3 else c2, c2 if gax == 3 else c3, nwk)
            if groups is None:
                return None
            cols[(i2, i3)] = {"groups": groups, "ng": len(groups), "halo": halo}
            ng_max = max(ng_max, len(groups))
            rows_total += 6 * len(groups)
    mid = cols[(n2 // 2, (e - b) // 2)]
    mid_rows = sum(2 * (1 + ((G["used"] & 7) != 0) + ((G["used"] & 0x38) != 0)) for G in mid["groups"])
    return {"cols": cols, "ng_max": ng_max, "rows_total": rows_total, "mid_rows": mid_rows, "gax": gax}


def pick_of(spec, planes=None):
    """The group-axis rule of ensure_colsweep: the axis whose plan has fewer groups, equal counts decided by the corner rows in total
    (axis 3 on equality).  -> (axis or None, {2: plan, 3: plan}, why): why names the branch that decided."""
    plans = {g: plan_of(spec, g, planes) for g in (2, 3)}
    p2, p3 = plans[2], plans[3]
    if p2 is None and p3 is None:
        return None, plans, "both_refused"
    if p2 is None:
        return 3, plans, "2_refused"
    if p3 is None:
        return 2, plans, "3_refused"
    if p3["ng_max"] != p2["ng_max"]:
        return (3 if p3["ng_max"] < p2["ng_max"] else 2), plans, "fewer_groups"
    return (3 if p3["rows_total"] <= p2["rows_total"] else 2), plans, ("rows_equal" if p3["rows_total"] == p2["rows_total"] else "rows_decide")


def admitted(spec, planes=None):
    """Variant 7 serves the problem."""
    return shape_admitted(spec) is None and pick_of(spec, planes)[0] is not None and cost_form_of(spec) is not None


def wave_knots(col, NG):
    """(nH0, nH1) of a column under a kernel of NG groups, in window knots: per group of the half 1 + (pair 0 used) + (pair 1 used), a
    padded group - the column has fewer than NG - counting 1."""
    ngh = (NG + 1) // 2
    k = [1 + ((G["used"] & 7) != 0) + ((G["used"] & 0x38) != 0) for G in col["groups"]] + [1] * (NG - col["ng"])
    return sum(k[:ngh]), sum(k[ngh:])


# ---- the one-load form ------------------------------------------------------------------------------------------------------------
def dpp_of(spec):
    """colsweep_dpp_ok restated, chunk by chunk: {"ok", "chunks": {(chunk, i2, i3): (kb, odd lane or None, states, flipped)}} over the
    (i2, i3) axis 0 depends on (index 0 where it does not).  kb is the value of (cell - index) at least half the states share (a tie
    keeps the first state's); more than one state elsewhere and the host refuses the form."""
    c, _ = axis_cells(spec, 0)
    n0 = spec.n[0]
    r2, r3 = c.shape[2], c.shape[3]
    out, ok = {}, True
    for i3 in range(r3):
        for i2 in range(r2):
            rel = c[:, 0, i2, i3, 0] - np.arange(n0)
            for ch, lo in enumerate(range(0, n0, LANES)):
                r = rel[lo:lo + LANES]
                same = int((r == r[0]).sum())
                kb, flipped = int(r[0]), False
                if 2 * same < len(r):
                    kb, flipped = int(r[r != r[0]][0]), True
                odd = np.flatnonzero(r != kb)
                if len(odd) > 1:
                    ok = False
                out[(ch, i2, i3)] = (kb, int(odd[0]) if len(odd) == 1 else (None if len(odd) == 0 else -1), len(r), flipped)
    return {"ok": ok, "chunks": out}


def split_of(spec, dpp, cs_split=0):
    """colsweep_split restated -> (parts in effect, [(first step, end) of every part])."""
    n0, n1, n2, n3 = spec.n
    lanes = LANES if dpp else 64
    waves = ((n0 + lanes - 1) // lanes) * n2 * n3
    S = int(cs_split)
    if S <= 0:
        S = 1
        while S < 8 and waves * S * 2 <= 5 * 6144 and n1 // (S * 2) >= 12:
            S *= 2
        while S < 8 and waves * S * 2 <= 4096 and n1 // (S * 2) >= 5:
            S *= 2
        if waves * S <= 4608 and 4 <= n1 <= 40:
            S = max(S, min(n1 // 2, 4608 // max(waves, 1), 16))
        S = max(S, min(8, (n1 + 30) // 60))
    S = max(1, min(S, max(1, n1)))
    return S, [(n1 * p // S, n1 * (p + 1) // S) for p in range(S)]


def xcd_of(spec, gax, axis=0, mod=0, plan=None):
    """colsweep_map restated -> (the eight counts, the index order they are cut from).  axis 1: the XCDs split the window axis (the
    modulus is then 1); mod -1: the smallest spacing of the mid-grid column's distinct group cells.  The counts are what the launch grid
    is made of and are compared with the device through it; the order has no readback and is compared with nothing."""
    ngx = spec.n[5 - gax] if axis else spec.n[gax]
    M = 1 if axis else int(mod)
    if M == 0:
        M = 1
    if M < 0:
        mid = plan["cols"][(spec.n[2] // 2, spec.n[3] // 2)]
        cells = sorted({G["cell"] for G in mid["groups"]})
        gaps = [b - a for a, b in zip(cells, cells[1:])]
        M = max(1, min(min(gaps) if gaps else 0, ngx))
    order = sorted(range(ngx), key=lambda i: i % M)                     # (stable)
    return [ngx * (x + 1) // 8 - ngx * x // 8 for x in range(8)], order


def grid_of(spec, gax, dpp, split, axis=0):
    """choose_launch's grid of variant 7: eight times the workgroups (four waves) the largest XCD share needs."""
    lanes = LANES if dpp else 64
    chunks = (spec.n[0] + lanes - 1) // lanes
    nfull = spec.n[gax] if axis else spec.n[5 - gax]
    most = max(xcd_of(spec, gax, axis)[0]) * chunks * nfull * split
    return max(1, 8 * ((most + 3) // 4))


def auto_variant_of(spec):
    """The automatic choice for a problem of this shape (hjbdp_choose.hip auto_variant, hjbdp_tables.hip analyse_tabled): neither the
    packed, the nested nor the control-split kernel applies; the row kernel's lean form is wanted when the axis-0 rows fill 45 % of
    their 64-lane chunks, and then the column sweep where it serves; else the table kernel."""
    n0 = spec.n[0]
    lane_use = n0 / (64.0 * ((n0 + 63) // 64))
    rec = cost_record_of(spec)
    lean = spec.nU <= 64 and rec["ncu"] <= K_MAXCU and all(t.mask == 1 << 4 for t in spec.cost_terms[rec["npre"]:])
    row_auto = (lean and lane_use >= 0.45) or (lane_use >= 0.7 and spec.nS >= 1 << 20)
    if row_auto and admitted(spec):
        return 7
    return 6 if row_auto and spec.cost_dtype is None else 5         # (float64 cost terms: the row kernel does not serve, the table kernel does)


def instantiation_of(spec, cs_dpp=1):
    """(storage, GAX, NG, cost form, DPP) of the kernel a stage of the problem launches, None where variant 7 does not serve."""
    if not admitted(spec):
        return None
    gax, plans, _ = pick_of(spec)
    return ("f16" if spec.j_dtype == np.float16 else "f32", gax, plans[gax]["ng_max"], cost_form_of(spec), bool(cs_dpp and dpp_of(spec)["ok"]))


ALL_INSTANTIATIONS = frozenset((s, g, ng, f, d) for s in ("f32", "f16") for g in (2, 3) for ng in range(1, 7) for f in (0, 1, 2)
                               for d in (False, True))


# ---- what a case reaches --------------------------------------------------------------------------------------------------------------
def axis1_steps(spec):
    """Per column the axis-1 cell of every step: {(i2, i3): cells}, over the (i2, i3) axis 1 depends on."""
    c, _ = axis_cells(spec, 1)
    return {(i2, i3): c[0, :, i2, i3, 0] for i2 in range(c.shape[2]) for i3 in range(c.shape[3])}


def coverage(spec, splits=(), xcd_mods=()):
    """The named conditions (tests/test_colsweep_shapes.py lists them) the problem reaches, as a set of strings."""
    out = set()
    nU = spec.nU
    out.add("nU:%d" % nU)
    why = shape_admitted(spec)
    if why is not None:
        out.add("refused:" + why)
        return out
    gax, plans, branch = pick_of(spec)
    out.add("pick:" + branch)
    if gax is None:
        return out
    form = cost_form_of(spec)
    if form is None:
        out.add("refused:cost64 shape")
        return out
    plan = plans[gax]
    NG = plan["ng_max"]
    storage = "f16" if spec.j_dtype == np.float16 else "f32"
    # the plans
    for col in plan["cols"].values():
        h0, h1 = wave_knots(col, NG)
        out.update(("nH0:%d" % h0, "nH1:%d" % h1))
        ngh = (NG + 1) // 2
        if col["ng"] == NG:
            out.add("ng_full:%d" % NG)
        else:
            if col["ng"] < ngh:
                out.add("pad_first:%d" % NG)
            out.add("pad_second:%d" % NG)
        groups = col["groups"]
        if [G["first"] for G in groups] != sorted(G["first"] for G in groups):
            out.add("plan:order_differs")
        nwk = spec.n[5 - gax]
        for k, G in enumerate(groups):
            p0, p1 = G["used"] & 7, (G["used"] >> 3) & 7
            out.add("used:both" if p0 and p1 else ("used:p0_only" if p0 else "used:p1_only"))
            for p in (p0, p1):
                if p:
                    out.add("members:%d" % bin(p).count("1"))
            if G["late"] & 7:
                out.add("plan:late_p0")
            if G["late"] & 0x38:
                out.add("plan:late_p1")
            for H in groups[:k]:
                if H["cell"] == G["cell"] and H["wmin"] == G["wmin"]:
                    out.add("plan:split_full_pair")
                if H["cell"] == G["cell"] and H["wmin"] != G["wmin"]:
                    out.add("plan:two_windows")
            if G["pulled"]:
                out.add("plan:wmin_clamped")        # (recorded where _column pulls a window opened at nwk - 2 down to nwk - 3)
        if nwk == 3:
            out.add("plan:nwk3")
    # the one-load form
    dpp = dpp_of(spec)
    if not dpp["ok"]:
        out.add("dpp_refused:g%d:%s" % (gax, storage))
    else:
        kbs = {}
        for (ch, i2, i3), (kb, odd, count, flipped) in dpp["chunks"].items():
            out.add("dpp:kb=%d" % kb)
            kbs.setdefault(ch, set()).add(kb)
            if flipped:
                out.add("dpp:kb_flip")
            if count == 1:
                out.add("dpp:last_chunk_one")
            if count == 2 and odd is not None:
                out.add("dpp:two_state_tie")
            if odd is not None:
                if odd == 0:
                    out.add("dpp:odd_lane0")
                elif odd == LANES - 1:
                    out.add("dpp:odd_lane59")
                elif odd == count - 1 and count < LANES:
                    out.add("dpp:odd_last_partial")
                elif count == LANES:
                    out.add("dpp:odd_mid")
        if any(len(v) > 1 for v in kbs.values()):
            out.add("dpp:kb_differs")
        if spec.n[0] == LANES:
            out.add("dpp:n0_60")
    for cs_dpp in (0, 1):
        out.add("inst:%s:g%d:ng%d:c%d:dpp%d" % (storage, gax, NG, form, int(bool(cs_dpp and dpp["ok"]))))
    # the steps and the parts
    n1 = spec.n[1]
    for cells in axis1_steps(spec).values():
        d = np.diff(cells)
        rep, jump = np.flatnonzero(d == 0) + 1, np.flatnonzero(d == 2) + 1
        if np.any(rep < n1 - 1):
            out.add("step:repeat_mid")
        if np.any(rep == n1 - 1):
            out.add("step:repeat_last")
        if len(jump):
            out.add("step:jump2")
        for s in splits:
            S, parts = split_of(spec, dpp["ok"], s)
            starts = {b for b, _ in parts[1:]}
            if starts & set(rep.tolist()):
                out.add("step:part_on_repeat")
            if starts & set(jump.tolist()):
                out.add("step:part_on_jump")
    for s in splits:
        S, parts = split_of(spec, dpp["ok"], s)
        if s > n1:
            out.add("step:split_above_n1")
        if S > 1 and any(e - b == 1 for b, e in parts):
            out.add("step:one_step_parts")
        if n1 % S:
            out.add("step:uneven_parts")
    # the XCD shares
    for axis in (0, 1):
        out.add("xcd:%d:%d" % (axis, spec.n[5 - gax] if axis else spec.n[gax]))
    for m in xcd_mods:
        out.add("xcd_mod:%d" % m)
    # the cost
    rec = cost_record_of(spec)
    out.update(("cost:form%d" % form, "cost:npre_col%d" % rec["npre_col"], "cost:has_su%d" % rec["has_su"], "cost:ncu%d" % rec["ncu"]))
    if not rec["step_uniform"]:
        out.add("cost:step_nonuniform")
    if rec["n_step"] == 2 and rec["step_uniform"]:
        out.add("cost:two_step_terms")
    if rec["npre"] == 0:
        out.add("cost:npre0")
    if rec["c64"] and rec["npre_col"] > 3:
        out.add("cost:c64_npre_col4")
    out.add("labels:%d:%d" % (spec.idx_np_dtype.itemsize, spec.index_base))
    return out


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------
def reference64(spec, terminal):
    """One stage of oracle.hjb_oracle.backup_stage on Problem(..., dtype=float64) built from the same terms -> J, labels (with
    index_base): flat, first state axis fastest."""
    from oracle import hjb_oracle as O
    conv = lambda ts: [O.Term(t.dims, np.asarray(t.data, dtype=np.float64)) for t in ts]
    p = O.Problem(spec.knots, spec.m, [conv(ts) for ts in spec.next_terms], conv(spec.cost_terms), dtype=np.float64)
    Jn = np.asarray(terminal).astype(np.float64).reshape(spec.n, order="F")
    J, idx = O.backup_stage(p, Jn, chunk_states=max(1, (1 << 22) // (spec.nU << 4)))
    flat = lambda x: np.asarray(x).reshape(-1, order="F")
    return flat(J), flat(idx).astype(np.int64) + spec.index_base


_REFS = {}


def case_reference(name):
    """(spec, terminal, J64, labels64, exact): the registered case, its lattice terminal, the float64 reference of one stage and
    whether one float32 stage is exact (one_stage_exact).  Computed once and shared."""
    if name not in _REFS:
        spec = CASES[name].build()
        term = lattice_terminal(spec, 3)
        J64, lab = reference64(spec, term)
        for a in (term, J64, lab):
            a.setflags(write=False)
        _REFS[name] = (spec, term, J64, lab, one_stage_exact(spec, term))
    return _REFS[name]


# ---- column designs ---------------------------------------------------------------------------------------------------------------
TOP = "T"                               # window cell nwk - 2: a window opened there is pulled down, its controls take pair 1


def design(counts, perm=None):
    """A column from member counts: group j takes counts[j] = (controls in pair 0, controls in pair 1), numbered consecutively; a
    group with pair 1 alone sits on the last window cell.  -> per control (group key, window offset or TOP); perm renumbers them."""
    d = []
    for j, (m0, m1) in enumerate(counts):
        d += [(j, 0)] * m0 + [(j, TOP if m0 == 0 else 1)] * m1
    if perm is not None:
        assert sorted(perm) == list(range(len(d)))
        d = [d[perm.index(u)] for u in range(len(d))]       # control perm[k] takes the k-th place
    return d


def design_problem(n, gax, designs, spread=2, **kw):
    """shape_problem from column designs, cycled over the columns: group key j sits on group cell base + spread j, window offsets count
    from a base cell that walks with the window-axis index."""
    n = tuple(n)
    n_g, n_w = n[gax], n[5 - gax]
    nU = len(designs[0])
    assert all(len(d) == nU for d in designs)
    jmax = max(j for d in designs for j, _ in d)
    wmax = max([1] + [w for d in designs for _, w in d if w != TOP])
    room_g, room_w = n_g - 1 - spread * jmax, n_w - 1 - wmax
    assert room_g >= 1 and room_w >= 1, (room_g, room_w)
    cg, cw = np.zeros((n_g, n_w, nU), dtype=int), np.zeros((n_g, n_w, nU), dtype=int)
    for ig in range(n_g):
        for iw in range(n_w):
            d = designs[(ig + n_g * iw) % len(designs)]
            for u, (j, w) in enumerate(d):
                cg[ig, iw, u] = ig % room_g + spread * j
                cw[ig, iw, u] = n_w - 2 if w == TOP else iw % room_w + w
    return shape_problem(n, gax, cg, cw, **kw)


def natural_problem(n, gax, levels, wmoves, **kw):
    """The shape problems.colsweep_problem draws, by construction: control u moves the group axis by levels[u] cells and the window axis
    by wmoves[u], the same on every column - the groups merge where the grid's edge clamps the cells.  The moves become terms over
    the control alone."""
    n_g, n_w = n[gax], n[5 - gax]
    lev, wm = np.asarray(levels, dtype=np.float64), np.asarray(wmoves, dtype=np.float64)
    qg = np.arange(n_g)[:, None, None] + lev[None, None, :]
    qw = np.arange(n_w)[None, :, None] + wm[None, None, :]
    cg, cw = np.floor(qg), np.floor(qw)
    return shape_problem(n, gax, cg.astype(int), cw.astype(int), tg=qg - cg, tw=qw - cw, **kw)


# ---- the registry -----------------------------------------------------------------------------------------------------------------
class Case:
    """build: the problem; reaches: the conditions (names of coverage) the case is registered for - each asserted on the case itself;
    splits, xcd_mods: the cs_split and cs_xcd_mod values the device test runs it under."""

    def __init__(self, build, reaches, splits=(1,), xcd_mods=(1,), admitted=True):
        self.build, self.reaches, self.splits, self.xcd_mods, self.admitted = build, tuple(reaches), tuple(splits), tuple(xcd_mods), admitted


CASES = {}

# per NG: (n0, n1, group-axis size, window-axis size) and the column designs, all of one control count
_SIZES = {1: (8, 9, 3, 7), 2: (60, 5, 7, 3), 3: (61, 6, 8, 8), 4: (64, 4, 9, 9), 5: (121, 4, 11, 5), 6: (62, 7, 13, 4)}
_N0_F16 = {1: 60, 2: 8, 3: 64, 4: 61, 5: 8, 6: 8}
_DESIGNS = {
    1: [design([(2, 1)]), design([(3, 0)]), design([(0, 3)]), design([(1, 2)])],
    2: [design([(2, 1), (2, 1)]), design([(3, 3)]), design([(3, 0), (3, 0)]), design([(3, 0), (0, 3)]), design([(1, 2), (3, 0)], perm=[3, 4, 5, 0, 1, 2])],
    3: [design([(1, 1)] * 3), design([(3, 3)]), design([(3, 0), (3, 0)]), design([(2, 0)] * 3), design([(3, 0), (2, 0), (0, 1)]),
        design([(1, 1)] * 3, perm=[4, 1, 2, 3, 0, 5])],
    4: [design([(1, 1), (1, 1), (1, 0), (1, 0)]), design([(3, 3)]), design([(1, 0), (1, 0), (1, 1), (2, 0)]), design([(3, 2), (0, 1)]),
        design([(1, 0), (1, 1), (1, 0), (0, 2)])],
    5: [design([(1, 1), (1, 1), (1, 1), (1, 0), (1, 0)]), design([(3, 3), (2, 0)]), design([(3, 3), (0, 2)]), design([(2, 0), (2, 0), (2, 0), (1, 0), (0, 1)]),
        design([(1, 1), (2, 0), (1, 0), (1, 1), (0, 1)], perm=[7, 1, 2, 3, 4, 5, 6, 0])],
    6: [design([(1, 1)] * 6), design([(3, 3), (3, 3)]), design([(2, 1)] * 3 + [(1, 0)] * 3), design([(2, 2)] * 3),
        design([(3, 0), (2, 0), (1, 0), (1, 1), (1, 1), (1, 1)]), design([(2, 0), (1, 0), (2, 0), (1, 1), (2, 2), (1, 0)]),
        design([(2, 2), (2, 2), (1, 0), (1, 0), (1, 0), (1, 0)]), design([(2, 0), (2, 0), (2, 0), (2, 1), (2, 0), (1, 0)])],
}
# what the designs of an NG are there for: the counted-wait entries (nH0 | nH1), padding, used bits, member counts, builder paths
_REACH_NG = {
    1: "nH0:2 nH0:3 nH1:0 ng_full:1 used:both used:p0_only used:p1_only members:1 members:2 members:3 plan:wmin_clamped",
    2: "nH0:2 nH0:3 nH1:1 nH1:2 nH1:3 ng_full:2 pad_second:2 used:both used:p0_only used:p1_only members:3 plan:nwk3 plan:wmin_clamped",
    3: "nH0:4 nH0:6 nH1:1 nH1:2 nH1:3 ng_full:3 pad_first:3 pad_second:3 used:p1_only plan:late_p0 plan:late_p1 plan:order_differs plan:wmin_clamped",
    4: "nH0:4 nH0:5 nH0:6 nH1:2 nH1:4 nH1:5 ng_full:4 pad_first:4 pad_second:4 plan:wmin_clamped",
    5: "nH0:6 nH0:9 nH1:2 nH1:4 nH1:6 ng_full:5 pad_first:5 pad_second:5 plan:late_p1 plan:order_differs plan:wmin_clamped",
    6: "nH0:6 nH0:7 nH0:8 nH0:9 nH1:3 nH1:6 nH1:7 nH1:8 nH1:9 ng_full:6 pad_first:6 pad_second:6 members:3",
}
_COST_OF_FORM = {0: ("multi", "ctrl_only", "cu0", "cu4", "ctrl_only2", "multi"), 1: ("fast", "step01", "col0", "col4", "two_step", "no_step"),
                 2: ("fast", "col4", "step01", "two_step", "col0", "col1")}
# what a cost shape is there for ("su": the cost record carries the one per-step term - unless the cost is summed in float64)
_REACH_COST = {
    "fast": "npre_col3 ncu1 su", "step01": "npre_col0 ncu1 step_nonuniform", "multi": "npre_col1 ncu2 two_step_terms",
    "ctrl_only": "npre_col0 ncu1 npre0", "col0": "npre_col0 ncu1 su", "col1": "npre_col1 ncu1 su", "col4": "npre_col4 ncu1 has_su0",
    "two_step": "npre_col1 ncu1 two_step_terms has_su0", "no_step": "npre_col2 ncu1 has_su0", "cu0": "npre_col1 ncu0 su",
    "cu4": "npre_col1 ncu%d su" % K_MAXCU, "ctrl_only2": "npre_col0 ncu2 npre0",
}
_LABELS = ((None, 1), (np.uint8, 0), (np.uint16, 1), (np.int32, 0), (np.uint8, 1), (np.uint16, 0))


def _axis0(n0, ng):
    """Axis 0's shifts for a size - every chunk keeps at most one state out of line (the one-load form is admitted) - and what the
    size is there for."""
    a0 = np.full(n0, 0.25)
    kw = {}
    if n0 == 61:
        a0[30] = 1.25                                   # one state in mid-chunk a cell higher; the last chunk is one state
        reach = "odd_mid last_chunk_one"
    elif n0 == 121:
        a0[:60], a0[60:120] = 1.25, -1.5                # kb = 1 on the first chunk, -2 on the second; the third is one state
        reach = "kb=1 kb=-2 kb=-1 last_chunk_one"
    elif n0 == 60 and ng % 2 == 0:
        a0[:] = -0.5                                    # kb = -1 by the flip branch: state 0 is clamped, alone and first
        reach = "n0_60 kb_flip kb=-1 odd_lane0"
    elif n0 == 60:
        reach = "n0_60 odd_lane59 kb=0"                 # the last state is clamped: the halo lane's knot too
    elif n0 == 62:
        reach = "two_state_tie kb=0"
    else:
        kw["a0_s2"] = lambda n2: -1.0 * (np.arange(n2) % 2)       # kb 0 / -1 by column
        reach = "kb_differs kb=0 kb=-1 kb_flip odd_lane0 odd_last_partial"
    return a0, kw, ["dpp:" + r for r in reach.split()]


def _matrix_params(gax, ng, storage, form):
    """The sizes and typing of the case (storage, gax, ng, form), and the conditions it is registered for."""
    n0, n1, n_g, n_w = _SIZES[ng]
    if storage == "f16":
        n0 = _N0_F16[ng]
    k = ng - 1 + (3 if storage == "f16" else 0) + (gax - 2)
    cost = _COST_OF_FORM[form][k % 6]
    idt, base = _LABELS[(k + form) % 6]
    first = storage == "f32" and form == 1
    splits = (1, 2, 3, n1, n1 + 3) if first else (1, n1)
    mods = (1, 3, -1) if first else (3,)
    reach = ["inst:%s:g%d:ng%d:c%d:dpp%d" % (storage, gax, ng, form, d) for d in (0, 1)] + _REACH_NG[ng].split() + _axis0(n0, ng)[2]
    for r in _REACH_COST[cost].split():
        reach.append("cost:" + (("has_su0" if form == 2 else "has_su1") if r == "su" else r))
    reach.append("cost:form%d" % form)
    if form == 2 and cost == "col4":
        reach.append("cost:c64_npre_col4")
    reach.append("labels:%d:%d" % (4 if idt is None else np.dtype(idt).itemsize, base))
    reach += ["step:repeat_last", "xcd:0:%d" % n_g, "xcd:1:%d" % n_w] + ["xcd_mod:%d" % m for m in mods]
    if n1 >= 6:
        reach += ["step:repeat_mid", "step:jump2"]
    if first:
        reach += ["step:split_above_n1", "step:one_step_parts"]
        if ng == 1:
            reach += ["step:part_on_repeat", "step:part_on_jump", "step:uneven_parts"]     # nine steps in 3 and in 2 parts: bounds 3 and 4
    if ng >= 5:
        reach.append("pick:%d_refused" % (5 - gax))     # the other axis would need more than K_GMAX groups
    return {"n0": n0, "n1": n1, "n_g": n_g, "n_w": n_w, "k": k, "cost": cost, "labels": (idt, base), "splits": splits, "mods": mods, "reach": reach}


def _matrix_case(gax, ng, storage, form):
    def build():
        P = _matrix_params(gax, ng, storage, form)
        n0, n1, k = P["n0"], P["n1"], P["k"]
        n = (n0, n1, P["n_w"], P["n_g"]) if gax == 3 else (n0, n1, P["n_g"], P["n_w"])
        a0, kw, _ = _axis0(n0, ng)
        kw = {key: v(n[2]) for key, v in kw.items()}
        a1 = np.full(n1, 0.375)
        if n1 >= 6:
            a1[3] = -0.625                              # step 3 repeats step 2's cell, step 4 jumps two
        a1_dim = 2 + k % 2
        spec = design_problem(n, gax, _DESIGNS[ng], a0=a0, a1=a1, a1_s=0.125 * (np.arange(n[a1_dim]) % 3), a1_dim=a1_dim,
                              cost=P["cost"], seed=100 * ng + 10 * gax + form, **kw)
        idt, base = P["labels"]
        return with_typing(spec, storage=np.float16 if storage == "f16" else None, cost64=form == 2, idx_dtype=idt, index_base=base)
    return build


def _register():
    for gax in (3, 2):
        for ng in range(1, 7):
            for storage in ("f32", "f16"):
                for form in (1, 0, 2):
                    P = _matrix_params(gax, ng, storage, form)
                    CASES["g%d-ng%d-%s-c%d" % (gax, ng, storage, form)] = Case(_matrix_case(gax, ng, storage, form), P["reach"], splits=P["splits"],
                                                                              xcd_mods=P["mods"])
    # the one-load form refused by the host: two states of a chunk out of line
    for gax in (3, 2):
        for storage in ("f32", "f16"):
            def build(gax=gax, storage=storage):
                a0 = np.full(64, 0.25)
                a0[[10, 20]] = 1.25
                n = (64, 4, 4, 7) if gax == 3 else (64, 4, 7, 4)
                spec = design_problem(n, gax, _DESIGNS[3], a0=a0, cost="fast", seed=7 + gax)
                return with_typing(spec, storage=np.float16 if storage == "f16" else None)
            CASES["dpp-refused-g%d-%s" % (gax, storage)] = Case(build, ["dpp_refused:g%d:%s" % (gax, storage), "inst:%s:g%d:ng3:c1:dpp0" % (storage, gax)])
    # a two-state chunk: the tie keeps the first state's value; n0 = 60: the halo lane's knot is clamped, the last state moves to the spare pair
    CASES["dpp-tie62"] = Case(lambda: design_problem((62, 4, 3, 5), 3, _DESIGNS[2], cost="fast", seed=62), ["dpp:two_state_tie"])
    CASES["dpp-n0-60"] = Case(lambda: design_problem((60, 4, 3, 5), 3, _DESIGNS[2], cost="col1", seed=60), ["dpp:n0_60", "dpp:odd_lane59"])
    # plan builder paths, placed
    def paths(gax):
        # control:       0        1        2        3        4        5         6        7       8
        d_split = [(0, 0), (0, 0), (0, 0), (0, 0), (1, 0), (1, 1), (0, 1), (2, 0), (2, 3)]          # four on one pair; two windows under key 2
        d_late = [(0, 0), (1, 0), (1, 1), (2, 1), (0, 1), (3, 0), (3, TOP), (2, 0), (0, 0)]          # keys 1, 2 come before key 0's high controls
        d_top = [(0, 0), (0, TOP), (1, TOP), (1, TOP), (2, 0), (2, 0), (2, 2), (0, 1), (1, 0)]       # two windows, the second pulled down
        n = (8, 5, 7, 12) if gax == 3 else (8, 5, 12, 7)
        return design_problem(n, gax, [d_split, d_late, d_top], cost="fast", seed=31 + gax, index_base=gax - 2)
    for gax in (3, 2):
        CASES["plan-paths-g%d" % gax] = Case(lambda gax=gax: paths(gax), ["plan:split_full_pair", "plan:two_windows", "plan:wmin_clamped", "plan:late_p0",
                                                                         "plan:late_p1", "plan:order_differs", "inst:f32:g%d:ng6:c1:dpp1" % gax])
    # control counts
    CASES["nu1"] = Case(lambda: design_problem((8, 4, 4, 5), 3, [design([(1, 0)]), design([(0, 1)])], cost="fast", seed=1), ["nU:1", "members:1"])
    lev16 = np.array([-1.75] * 6 + [0.25] * 5 + [1.25] * 5)                 # three levels: a pair fills and splits; edge columns merge levels
    wm16 = np.array([0.125, 0.25, 0.375, 0.5, 1.125, 1.25] + [0.125, 0.25, 0.375, 1.125, 1.25] * 2)
    CASES["nu16"] = Case(lambda: natural_problem((60, 5, 5, 9), 3, lev16, wm16, cost="fast", seed=16), ["nU:16", "plan:split_full_pair", "ng_full:6"])
    CASES["nu17"] = Case(lambda: natural_problem((8, 4, 5, 9), 3, np.append(lev16, 0.25), np.append(wm16, 0.125), cost="fast", seed=17),
                         ["nU:17", "refused:controls"], admitted=False)
    # moves over the control alone (tables of nU entries), group axis 2; a step that jumps two
    CASES["natural-g2"] = Case(lambda: natural_problem((64, 6, 9, 5), 2, np.repeat([-1.75, 0.25, 1.25], 3), np.tile([-0.625, 0.125, 0.5], 3), cost="multi", seed=18,
                                                       a1=np.array([0.375, 1.375, 0.375, 0.375, 0.375, 0.375])),
                               ["step:jump2", "inst:f32:g2:ng3:c0:dpp1"])
    # the pick rule
    def rows_decide():
        # both axes need two groups at most; axis 2 needs them on fewer columns
        cg = np.zeros((6, 5, 2), dtype=int)
        cw = np.zeros((6, 5, 2), dtype=int)
        for ig in range(6):
            for iw in range(5):
                cg[ig, iw] = (ig % 4, ig % 4 + (1 if iw == 0 else 0))        # two group cells on one window-axis index only
                cw[ig, iw] = (iw % 3, iw % 3 + (1 if ig < 3 else 0))         # two window cells on half the group-axis indices
        return shape_problem((8, 4, 6, 5), 2, cg, cw, cost="fast", seed=41)
    CASES["pick-rows"] = Case(rows_decide, ["pick:rows_decide", "inst:f32:g2:ng2:c1:dpp1"])

    def both_refused():
        # seven distinct cells, two apart, on either axis: neither plan fits K_GMAX groups
        cg = (np.arange(8)[None, None, :] * 2) + np.zeros((15, 15, 1), dtype=int)
        cw = (np.arange(8)[None, None, ::-1] * 2) + np.zeros((15, 15, 1), dtype=int)
        return shape_problem((8, 4, 15, 15), 3, cg % 14, cw % 14, cost="fast", seed=43)
    CASES["pick-none"] = Case(both_refused, ["pick:both_refused"], admitted=False)
    CASES["cost-cu5"] = Case(lambda: design_problem((8, 4, 4, 5), 3, _DESIGNS[1], cost="cu5", seed=5), ["refused:control terms"], admitted=False)
    CASES["cost-c64-general"] = Case(lambda: with_typing(design_problem((8, 4, 4, 5), 3, _DESIGNS[1], cost="multi", seed=6), cost64=True),
                                     ["refused:cost64 shape"], admitted=False)


_register()
RUN_CASES = [name for name in CASES if CASES[name].admitted]
REFUSED_CASES = [name for name in CASES if not CASES[name].admitted]
LATE_CASES = ["plan-paths-g3", "plan-paths-g2", "g3-ng5-f32-c1", "g2-ng3-f16-c1"]       # each registers a late slot


