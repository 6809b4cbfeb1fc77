"""GPU tests (-m gpu) of the fixed-label stage's three index forms AT THE SIZES WHERE THE HOST CHANGES FORM (k_evaluate in
csrc/kernels_evaluate.h; eval_runs_i32 / eval_runs_m24 in csrc/hjbdp_host.h, hjbdp_choose.hip): 64-bit indices, 32-bit indices
with division by multiplication, and 32-bit indices with 24-bit index products (__umul24 drops the bits above 24 of an operand
silently: the offset only shrinks, so nothing faults - a wrong J for the states, labels or planes beyond 2^24).

Per case, everything on the device: fill_separable -> backup_stage_device -> evaluate_stage_device from every source of cells
and weights the handle has, in the automatic form and in every more general form (eval_m24 0; eval_i32 0).  Bars, bit for bit:
  own labels       the evaluation equals the backup's J (whole grid by download up to 6e7 states, on the sample above that);
  own labels       on the sample, the backup's J and labels equal the C twin's (oracle.c_oracle.backup_states);
  other labels     a seeded block repeated with a period coprime to every axis size (np.resize): every form equals the 64-bit
                   form (whole grid or sample as above) and, on the sample, evaluate_refs.evaluate_ref_states (a float64-summed
                   cost: the C twin's backups of the problem restricted to one control, as tests/test_gpu_evaluate.py does);
  form             get_option("eval_form") before each launch equals the case's stated form for that source.
The sample (a condition, _sample checks it): first and last state, both sides of every 256-state workgroup boundary adjacent to
2^24, 2^25, 2^31 - 2^26, 2^31 and 2^32 the grid reaches, the last 300 states, the last plane's first and last state, 20,000
seeded random states.  Where a case's form is not 2 and there are states a 24-bit product (or, rows l and m, a 32-bit index)
would corrupt, the sample holds at least 100 of them (`risk`); rows b and i have none - the predicate is conservative there, the
largest factor is 2^24 - 1 - and row h has five states in all, three of them beyond the line.

CASES states, per row, the form per source and every conjunct of the two predicates that is false; _factors restates the
quantities from the shapes, the tests hold table, restatement and library to each other, and the last test checks that every
conjunct is false in some row and true at its largest admissible value in another."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K24 = 1 << 24
LIM32 = (1 << 31) - (1 << 26)              # kTab32Lim (csrc/kernels_tabled.h)
PERIOD = 8191                              # of the second label array: a prime that divides no axis size used here
NEAR32 = 1 << 21                           # "at its largest admissible value" for the two 32-bit conjuncts: within 0.1 % of the limit

# the conjuncts of eval_runs_m24 (every quantity below 2^24) and, on n_owned / j_elems, of eval_runs_i32 (below 2^31 - 2^26)
M24_ALWAYS = ("q0", "nU", "n", "jstride", "nplanes", "cost_stride")
M24_TABLES = ("sstride", "cstride")        # source 1: the (cell, t) tables' strides
M24_TERMS = ("next_stride",)               # source 0: the next-state terms' strides
I32 = ("n_owned", "j_elems")


def _case(n, m, expect, false=(), risk=None, nonuniform=False, storage="f32", idx="auto", base=1, **kw):
    return dict(n=tuple(n), m=tuple(m), expect=expect, false=frozenset(false), risk=risk, nonuniform=nonuniform, storage=storage,
                idx=idx, base=base, **kw)


# expect: {source: form}, source 0 = terms summed in the kernel, 1 = (cell, t) tables; forms 0 64-bit, 1 32-bit, 2 24-bit products.
# false: EVERY conjunct that is false for the row (sstride / cstride: for the tables, next_stride: for the terms).
W = (0, 2, 3)       # the "wide" term's dims on a D = 3 grid with n1 = 3: (axis 0, axis 2, control) - control stride n0 * n2
CASES = {
    # a: first quotient 4095 * 4097 = 2^24 - 1, M24 at its largest operand; nothing false
    "a": _case((2, 4095, 4097), (2,), {0: 2, 1: 2}, nonuniform=True, idx=np.uint8),
    # b: q0 false alone - n_owned / n0 = 2^24 exactly (the largest quotient a state forms is 2^24 - 1: no state at risk)
    "b": _case((2, 4096, 4096), (3,), {0: 1, 1: 1}, {"q0"}, storage="f16", idx=np.uint16, base=0),
    # c: q0 false alone - 16,781,312; the 8,192 states from 2^25 on form a quotient of 2^24 or more.  (Measured once with a
    # library whose launch took the 24-bit products regardless: those states still came out right - the masked quotient puts an
    # error of a multiple of 2^24 into the remainder, which every later 24-bit product drops again - while rows e1, f, f2, g64, h
    # and o came out wrong.  The q0 condition is sufficient, not necessary; it stays as it is.)
    "c": _case((2, 4097, 4096), (2,), {0: 1, 1: 1}, {"q0"}, risk="q0", nonuniform=True, idx=np.int32),
    # d: jstride[2] = 2^24 - 1, and (axis 2 moves with axes 0 and 1) its table's stride along dim 2 too; nothing false
    "d": _case((4095, 4097, 2), (2,), {0: 2, 1: 2}, nonuniform=True, storage="f16", idx=np.uint8, base=0, last_sees_all=True),
    # e: jstride[2] = 2^24 and the table stride sstride[2] with it (one cell along axis 2: the J offset js * cell is 0 either
    # way; the tables' sstride[2] * plane is not - the states of plane 1 are at risk from the tables)
    "e1": _case((4096, 4096, 2), (2,), {0: 1, 1: 1}, {"jstride", "sstride"}, risk="plane", last_sees_all=True),
    # ... 4097: jstride[2] = sstride[2] = 16,781,312; prob.n[0] still small
    "e2": _case((4097, 4096, 2), (3,), {0: 1, 1: 1}, {"jstride", "sstride"}, risk="plane", nonuniform=True, storage="f16",
                last_sees_all=True),
    # f: q0 = 12,288, jstrides (1, 4097, 12291); axis 1's ONE next-state term over (0, 2, control) has control stride
    # 4097 * 4096 >= 2^24 - the term's stride (terms) and the table's cstride (tables), nothing else
    "f": _case((4097, 3, 4096), (2,), {0: 1, 1: 1}, {"next_stride", "cstride"}, risk="ctrl", nonuniform=True, wide_next=W),
    # ... 4095 * 4097 = 2^24 - 1: both at their largest admissible value
    "f_max": _case((4095, 3, 4097), (2,), {0: 2, 1: 2}, wide_next=W),
    # ... the same domain from two narrow terms, (0, control) and (2,): the terms' strides are small, the table over their union
    # has cstride 4097 * 4096 - the two sources legitimately run different forms
    "f2": _case((4097, 3, 4096), (2,), {0: 2, 1: 1}, {"cstride"}, risk="ctrl", nonuniform=True, storage="f16", split_next=True),
    # g: as f, the wide term a COST term - both sources read it; once float32, once cost_dtype float64 (cost64[]: "the same strides")
    "g": _case((4097, 3, 4096), (2,), {0: 1, 1: 1}, {"cost_stride"}, risk="ctrl", nonuniform=True, wide_cost=W),
    "g64": _case((4097, 3, 4096), (2,), {0: 1, 1: 1}, {"cost_stride"}, risk="ctrl", nonuniform=True, wide_cost=W, cost64=True, base=0),
    "g_max": _case((4095, 3, 4097), (2,), {0: 2, 1: 2}, wide_cost=W),
    # h: nU = 2^24 + 3 false alone (the label itself is the control index the (state, control) term's stride multiplies);
    # evaluation only, labels by hand on both sides of 2^24; its table of 5 nU entries does not fit: terms only
    "h": _case((5,), (K24 + 3,), {0: 1}, {"nU"}, risk="label", idx=np.int32, state_control_term=True,
               labels=(0, K24 - 1, K24, K24 + 1, K24 + 2)),
    # ... nU = 2^24 - 1: at its largest admissible value
    "h_max": _case((5,), (K24 - 1,), {0: 2}, idx=np.int32, state_control_term=True, labels=(0, 1, K24 - 3, K24 - 2, K24 - 2)),
    # i: nU = 4097 * 4096 >= 2^24 false alone, though no single product overflows (cj0 < 4097, cj1 < 4096): conservative
    "i": _case((11,), (4097, 4096), {0: 1, 1: 1}, {"nU"}, idx=np.int32, base=0),
    # k: 2,079,178,200 states, 1,196,584 below 2^31 - 2^26: the 32-bit form and M24 at nearly the largest index they may see
    "k": _case((1275, 1276, 1278), (2,), {0: 2, 1: 2}, nonuniform=True, storage="f16", idx=np.uint8),
    # l: 2,148,197,465 states > 2^31: n_owned and j_elems false; state indices on both sides of 2^31 - 2^26 and 2^31
    "l": _case((1283, 1285, 1303), (2,), {0: 0, 1: 0}, {"n_owned", "j_elems"}, risk="i32", storage="f16", idx=np.uint8, base=0),
    # m: 4,296,110,364 states > 2^32: the 64-bit form on both sides of 2^32
    "m": _case((1618, 1621, 1638), (2,), {0: 0, 1: 0}, {"n_owned", "j_elems"}, risk="i32", nonuniform=True, storage="f16", idx=np.uint8),
    # n / o: D = 1, where the one axis is the last: prob.n[0] = nplanes = 2^24 - 1 (largest admissible; so is the (state, control)
    # table's control stride n0), then 2^24 + 300 (all three false; the 300 states from 2^24 on are an index the term and table
    # offsets multiply)
    "n": _case((K24 - 1,), (2,), {0: 2, 1: 2}, idx=np.uint8, int_knots=True),
    "o": _case((K24 + 300,), (3,), {0: 1, 1: 1}, {"n", "nplanes", "cstride"}, risk="index", storage="f16", idx=np.uint8, base=0, int_knots=True),
}
# j: row d's axes 0 and 1 with four planes, so that a slab with a halo on both sides exists (planes 1 - 2 owned, 0 and 3 halo):
# jstride[2] = 2^24 - 1 multiplies cells 0 .. 2; plane0, nplanes, out0 = inner * halo_lo, local against global last index
SLAB_CASE = _case((4095, 4097, 4), (2,), {0: 2, 1: 2}, nonuniform=True, idx=np.uint8)
SLAB = (1, 3, 1, 1)
BIG = ("k", "l", "m")                      # compared on the sample; f16 J, one-byte labels: 11, 11 and 22 GB of HBM


def _prod(xs):
    out = 1
    for x in xs:
        out *= int(x)
    return out


def _term_dims(case):
    """(next_dims[a] = the dims tuple of each next-state term of axis a, cost_dims) - what _build builds."""
    n, m = case["n"], case["m"]
    D, C = len(n), len(m)
    nxt = []
    for a in range(D):
        if case.get("wide_next") and a == 1:
            nxt.append([case["wide_next"]])
            continue
        if case.get("split_next") and a == 1:
            nxt.append([(0, D), (2,)])
            continue
        ts = [(a,)]
        if case.get("state_control_term"):
            ts.append((0, 1))
        elif case.get("last_sees_all") and a == D - 1:
            ts += [(b,) for b in range(D - 1)]
        else:
            if D > 1:
                ts.append((min((b for b in range(D) if b != a), key=lambda b: n[b]),))      # the smallest other axis: small tables
            ts.append((D + a % C,))
        nxt.append(ts)
    cost = [(a,) for a in range(D)] + [(D + c,) for c in range(C)]
    if case.get("wide_cost"):
        cost.append(case["wide_cost"])
    return nxt, cost


def _factors(case, slab=None):
    """The quantities the two predicates bound, from the shapes alone (column-major strides: products of the sizes before)."""
    n, m = case["n"], case["m"]
    D = len(n)
    g = n + m
    owned_last = n[-1] if slab is None else slab[1] - slab[0]
    nplanes = n[-1] if slab is None else owned_last + slab[2] + slab[3]
    inner = _prod(n[:-1])

    def strides(dims, sizes):
        out, s = {}, 1
        for d in dims:
            out[d] = s
            s *= sizes[d]
        return out
    nxt, cost = _term_dims(case)
    local = n[:-1] + (owned_last,) + m                                 # the tables cover the owned planes
    f = {"n_owned": inner * owned_last, "j_elems": inner * nplanes, "q0": inner * owned_last // n[0], "nU": _prod(m), "n": max(n),
         "jstride": inner, "nplanes": nplanes,
         "next_stride": max(max(strides(t, g).values()) for ts in nxt for t in ts),
         "cost_stride": max(max(strides(t, g).values()) for t in cost), "sstride": 0, "cstride": 0}
    for ts in nxt:
        dom = strides(sorted(set(d for t in ts for d in t)), local)
        f["sstride"] = max([f["sstride"]] + [s for d, s in dom.items() if d < D])
        f["cstride"] = max([f["cstride"]] + [s for d, s in dom.items() if d >= D])
    return f


def _model_form(case, source, slab=None):
    f = _factors(case, slab)
    if not all(f[k] < LIM32 for k in I32):
        return 0
    return 2 if all(f[k] < K24 for k in M24_ALWAYS + (M24_TABLES if source == 1 else M24_TERMS)) else 1


def _false(case, slab=None):
    f = _factors(case, slab)
    return frozenset([k for k in I32 if f[k] >= LIM32] + [k for k in M24_ALWAYS + M24_TABLES + M24_TERMS if f[k] >= K24])


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi, c_oracle


def _repeat(rng, shape, lo, hi, period=PERIOD):
    """A seeded block of `period` float32 values repeated over `shape` (column-major): a table of 3e7 .. 8e7 elements without
    drawing that many numbers; the period is coprime to the sizes, so no axis sees a repeating pattern."""
    block = rng.uniform(lo, hi, period).astype(np.float32)
    return np.resize(block, _prod(shape)).reshape(shape, order="F")


def _build(hjbdp, case, seed):
    """-> (spec, vecs): the problem of _term_dims(case) and the separable terminal cost's vectors.  Moves of a few cells on long
    axes, of less than half a cell on axes of six knots or fewer (halo 1); binary16 storage: vecs in eighths below 64, so that their
    float32 sum is exact and a binary16 number - the C twin's backup_states reads the unrounded sum."""
    rng = np.random.default_rng(seed)
    n, m = case["n"], case["m"]
    D = len(n)
    g = n + m
    knots = []
    for a in range(D):
        if case.get("int_knots"):
            k = np.arange(n[a], dtype=np.float64) - float(1 << 23)       # every knot an integer below 2^24 in magnitude: exact in float32
        elif case["nonuniform"]:
            k = np.cumsum(rng.uniform(0.5, 1.5, n[a]))
            k = (k - k[0]) / (k[-1] - k[0]) * 2.0 - 1.0
        else:
            k = np.linspace(-1.0, 1.0, n[a])
        knots.append(k.astype(np.float32).astype(np.float64))
    move = [(knots[a][-1] - knots[a][0]) / (n[a] - 1) * (5.0 if n[a] > 6 else 0.2) for a in range(D)]
    unit = [(knots[a] - knots[a][0]) / (knots[a][-1] - knots[a][0]) * 2.0 - 1.0 for a in range(D)]
    dims_next, dims_cost = _term_dims(case)

    def table(dims, lo, hi):
        shape = tuple(g[d] for d in dims)
        return _repeat(rng, shape, lo, hi) if _prod(shape) > (1 << 22) else rng.uniform(lo, hi, shape)
    nxt = []
    for a in range(D):
        ts = []
        for dims in dims_next[a]:
            if dims == (a,):
                ts.append(hjbdp.Term(dims, knots[a].copy()))
            elif a == 1 and (case.get("wide_next") or case.get("split_next")):      # axis 1 (three knots) has no term of its own
                ts.append(hjbdp.Term(dims, table(dims, -0.5, 0.5)))
            else:
                ts.append(hjbdp.Term(dims, table(dims, -move[a], move[a])))
        nxt.append(ts)
    cost = []
    for dims in dims_cost:
        if len(dims) == 1 and dims[0] < D:
            cost.append(hjbdp.Term(dims, (1.0 + dims[0]) * unit[dims[0]] ** 2))
        else:
            cost.append(hjbdp.Term(dims, table(dims, 0.0, 0.5)))
    spec = hjbdp.ProblemSpec(knots, m, nxt, cost, dtype=np.float32, index_base=case["base"],
                             j_storage=np.float16 if case["storage"] == "f16" else None, idx_dtype=case["idx"],
                             cost_dtype=np.float64 if case.get("cost64") else None)
    if case["storage"] == "f16":
        vecs = [(rng.integers(0, 512, k) / 8.0).astype(np.float32) for k in n]
    else:
        vecs = [(rng.random(k) * (1.0 + a)).astype(np.float32) for a, k in enumerate(n)]
    assert all(math.gcd(PERIOD, k) == 1 for k in n)
    return spec, vecs


def _sample(n, rng):
    """The sample rule of the module docstring, checked."""
    nS = _prod(n)
    inner = nS // n[-1]
    lines = [b + d for B in (K24, 1 << 25, LIM32, 1 << 31, 1 << 32) for b in (B - 256, B, B + 256) for d in (-1, 0)]
    tail = np.arange(max(0, nS - 300), nS, dtype=np.int64)
    parts = [np.array([0, nS - 1, nS - inner] + lines, dtype=np.int64), tail, rng.integers(0, nS, 20000, dtype=np.int64)]
    sel = np.unique(np.concatenate(parts))
    sel = sel[(sel >= 0) & (sel < nS)]
    have = set(sel.tolist())
    assert {0, nS - 1, nS - inner} <= have and set(tail.tolist()) <= have
    assert all(x in have for x in lines if 0 <= x < nS)
    assert nS <= 20000 or sel.size >= 20000
    return sel


def _at_risk(case, states, labels0):
    """The listed states a 24-bit product (risk 'i32': a 32-bit index) would corrupt, by the row's stated kind."""
    n = case["n"]
    kind = case["risk"]
    if kind == "q0":
        return states // n[0] >= K24                       # the first quotient of the state index
    if kind == "index":
        return states >= K24                               # D = 1: the state index is the axis index the strides multiply
    if kind == "plane":
        return states // _prod(n[:-1]) >= 1                # the tables' stride along the last dim times the plane
    if kind == "ctrl":
        return labels0 > 0                                 # C = 1: the wide control stride times the control index
    if kind == "label":
        return labels0 >= K24
    assert kind == "i32"
    return states >= LIM32


def _sources(hjbdp, _abi, bk):
    from test_gpu_evaluate import _sources as sources
    return sources(hjbdp, _abi, bk)


def _forms(auto):
    """(eval_i32, eval_m24, the form that must run) - most general first: its result is what the others are compared with."""
    out = [(1, 0, min(auto, 1)), (1, 1, auto)]
    return ([(0, 1, 0)] if auto != 0 else []) + out


def _upload_repeated(hjbdp, _abi, dL, block, nS, dtype):
    """dL = np.resize(block, nS) as `dtype`: a chunk that is a whole number of periods from the host, doubled on the device."""
    chunk = PERIOD * 1024
    if nS <= chunk:
        dL.upload(np.resize(block, nS).astype(dtype))
        return
    dL.upload(np.resize(block, chunk).astype(dtype))
    ib = np.dtype(dtype).itemsize
    filled = chunk
    while filled < nS:
        cnt = min(filled, nS - filled)
        assert dL.lib.hjb_device_copy(0, dL.ptr + filled * ib, dL.ptr, cnt * ib, _abi.HJB_COPY_D2D) == 0
        filled += cnt


def _oracle_backup(env, spec, vecs, sel):
    """The C twin's backup of the sampled states from the separable terminal cost -> (J in the J storage type, labels).  The twin's
    sampled entry takes float32 storage only: a binary16-stored spec goes in retyped - same arithmetic; its terminal cost is exact
    in binary16 (_build), and the float32 J it returns is rounded to binary16 once, as the kernels store it."""
    hjbdp, _abi, c_oracle = env
    if spec.j_dtype != spec.dtype:
        from test_gpu_evaluate import _retype
        s32 = _retype(hjbdp, spec)
        for v in vecs:
            assert np.array_equal(v.astype(np.float16).astype(np.float32), v)
        tot = sum(float(v.max()) for v in vecs)
        assert tot < 256.0                                     # eighths below 2^8: every partial sum is a binary16 number
    else:
        s32 = spec
    J, idx = c_oracle.backup_states(_abi, s32, vecs, sel)
    return J.astype(spec.j_dtype), idx


def _other_labels_ref(env, spec, vecs, sel, lab0):
    """The fixed-label stage's value at the sampled states for 0-based labels lab0, in the J storage type."""
    hjbdp, _abi, c_oracle = env
    if spec.cost_dtype is None:
        from evaluate_refs import evaluate_ref_states, oracle_problem, separable_jnext
        return evaluate_ref_states(oracle_problem(spec), sel, lab0, separable_jnext(vecs, np.float32, spec.j_dtype)).astype(spec.j_dtype)
    from test_gpu_evaluate import _restrict_to_control
    out = np.empty(sel.size, dtype=np.float32)
    for u in range(spec.nU):                               # the C twin's backup of the problem with control u alone IS its candidate
        Ju, _ = _oracle_backup(env, _restrict_to_control(hjbdp, spec, u), vecs, sel)
        out[lab0 == u] = Ju[lab0 == u]
    return out.astype(spec.j_dtype)


def _run(env, case, seed):
    hjbdp, _abi, c_oracle = env
    n = case["n"]
    nS = _prod(n)
    by_download = nS <= 6 * 10 ** 7                      # (rows a - e: 3.4e7 states, rows f, g: 5.0e7)
    jd = np.dtype(np.float16 if case["storage"] == "f16" else np.float32)
    spec, vecs = _build(hjbdp, case, seed)
    ld = spec.idx_np_dtype
    assert spec.nS == nS and spec.j_dtype == jd and (case["idx"] == "auto" or ld == np.dtype(case["idx"]))
    need = 3 * nS * jd.itemsize + 2 * nS * ld.itemsize
    free, _ = hjbdp.device_mem_info(0)
    if free < need + (4 << 30):
        pytest.skip("needs %.0f GB of free HBM, have %.0f GB" % ((need + (4 << 30)) / 2 ** 30, free / 2 ** 30))
    rng = np.random.default_rng(seed + 1)
    sel = _sample(n, rng)
    base = spec.index_base
    own = case.get("labels") is None                       # (rows h: evaluation only, labels by hand)
    if own:
        block = rng.integers(0, spec.nU, PERIOD)
        lab0 = block[sel % PERIOD]
    else:
        lab0 = np.asarray(case["labels"], dtype=np.int64)
        assert lab0.size == nS and sel.size == nS
    want_other = _other_labels_ref(env, spec, vecs, sel, lab0)
    bufs = [hjbdp.DeviceBuffer(nS * jd.itemsize) for _ in range(3)] + [hjbdp.DeviceBuffer(nS * ld.itemsize) for _ in range(2)]
    dA, dB, dC, dI, dL = bufs
    try:
        with hjbdp.Backup(spec) as bk:
            bk.fill_separable(vecs, dA)
            if own:
                _upload_repeated(hjbdp, _abi, dL, block + base, nS, ld)
                bk.backup_stage_device(dA, dB, dI)
                bk.check_device_status()
                Jr, ir = _oracle_backup(env, spec, vecs, sel)
                JBs, IBs = dB.gather(jd, sel), dI.gather(ld, sel)
                assert np.array_equal(JBs, Jr), ("backup J", sel[np.flatnonzero(JBs != Jr)[:5]])
                assert np.array_equal(IBs, ir), ("backup labels", sel[np.flatnonzero(IBs != ir)[:5]])
                JB = dB.download(jd) if by_download else None
                own0 = IBs.astype(np.int64) - base
                assert np.mean(own0 != lab0) > 0.2             # the second label array is not the argmin
            else:
                dL.upload((lab0 + base).astype(ld))
                own0 = lab0
            if case["risk"]:                                   # the states the test is about are in the sample
                at_risk = int(np.sum(_at_risk(case, sel, lab0 if case["risk"] == "label" else own0)))
                assert at_risk >= (100 if nS > 100 else 3), at_risk
            srcs = _sources(hjbdp, _abi, bk)
            assert srcs == sorted(case["expect"]), (srcs, case["expect"])
            for s in srcs:
                bk.set_option("eval_tables", s)
                auto = case["expect"][s]
                assert auto == _model_form(case, s)
                ref_other = None
                for i32, m24, form in _forms(auto):
                    bk.set_option("eval_i32", i32)
                    bk.set_option("eval_m24", m24)
                    tag = (s, i32, m24)
                    if own:                                    # own labels: the backup's J
                        assert bk.get_option("eval_form") == form, (tag, bk.get_option("eval_form"))
                        bk.evaluate_stage_device(dA, dI, dC)
                        bk.check_device_status()
                        if by_download:
                            got = dC.download(jd)
                            assert np.array_equal(got, JB), (tag, "own", np.flatnonzero(got != JB)[:5])
                        else:
                            got = dC.gather(jd, sel)
                            assert np.array_equal(got, JBs), (tag, "own", sel[np.flatnonzero(got != JBs)[:5]])
                    assert bk.get_option("eval_form") == form, (tag, bk.get_option("eval_form"))
                    bk.evaluate_stage_device(dA, dL, dC)       # the other labels: the 64-bit form's result, and the reference
                    bk.check_device_status()
                    got = dC.download(jd) if by_download else dC.gather(jd, sel)
                    if ref_other is None:
                        ref_other = got
                    assert np.array_equal(got, ref_other), (tag, "forms", np.flatnonzero(got != ref_other)[:5])
                    gs = got[sel] if by_download else got
                    assert np.array_equal(gs, want_other), (tag, "reference", sel[np.flatnonzero(gs != want_other)[:5]])
                bk.set_option("eval_i32", 1)
                bk.set_option("eval_m24", 1)
    finally:
        for b in bufs:
            b.free()


def _params():
    return [pytest.param(k, marks=pytest.mark.order(6)) if k in BIG else k for k in CASES]


@pytest.mark.parametrize("name", _params())
def test_forms_at_the_line(env, name):
    case = CASES[name]
    assert case["false"] == _false(case), (name, sorted(_false(case)))      # the table's statement against the shapes
    _run(env, case, 7000 + 13 * sorted(CASES).index(name))


def test_slab_with_halos_at_the_jstride_line(env):
    """Row j.  The slab handle reads the whole-grid J (its two halo planes are the grid's first and last plane) and the owned
    planes' part of the label arrays; on the owned planes it gives the whole-grid handle's result in every form, from every source."""
    hjbdp, _abi, c_oracle = env
    case = SLAB_CASE
    assert _false(case) == _false(case, SLAB) == frozenset() and _factors(case, SLAB)["jstride"] == K24 - 1
    spec, vecs = _build(hjbdp, case, 7777)
    n = case["n"]
    nS, inner = spec.nS, spec.nS // n[-1]
    b, e, lo, hi = SLAB
    assert b - lo == 0 and e + hi == n[-1] and lo == hi == 1
    rng = np.random.default_rng(7778)
    block = rng.integers(0, spec.nU, PERIOD)
    bufs = [hjbdp.DeviceBuffer(nS * 4) for _ in range(3)] + [hjbdp.DeviceBuffer(nS) for _ in range(2)]
    dA, dB, dC, dI, dL = bufs
    try:
        with hjbdp.Backup(spec) as bk:
            inf = bk.info()
            assert inf["halo_needed_lo"] <= lo and inf["halo_needed_hi"] <= hi
            bk.fill_separable(vecs, dA)
            _upload_repeated(hjbdp, _abi, dL, block + spec.index_base, nS, spec.idx_np_dtype)
            bk.backup_stage_device(dA, dB, dI)
            bk.check_device_status()
            JB = dB.download(np.float32)
            assert bk.get_option("eval_form") == 2
            bk.evaluate_stage_device(dA, dL, dC)
            bk.check_device_status()
            JO = dC.download(np.float32)
        sel = _sample(n, rng)
        Jr, ir = _oracle_backup(env, spec, vecs, sel)
        assert np.array_equal(JB[sel], Jr) and np.array_equal(dI.gather(np.uint8, sel), ir)
        assert np.array_equal(JO[sel], _other_labels_ref(env, spec, vecs, sel, block[sel % PERIOD]))
        JA = dA.download(np.float32)
        with hjbdp.Backup(spec, slab=SLAB) as bk:
            assert bk.info()["j_elems"] == nS and bk.info()["n_states"] == inner * (e - b)
            for s in _sources(hjbdp, _abi, bk):
                bk.set_option("eval_tables", s)
                assert case["expect"][s] == _model_form(case, s, SLAB)
                for i32, m24, form in _forms(case["expect"][s]):
                    bk.set_option("eval_i32", i32)
                    bk.set_option("eval_m24", m24)
                    for dLab, want in ((dI, JB), (dL, JO)):
                        assert bk.get_option("eval_form") == form
                        assert bk.lib.hjb_device_copy(0, dC.ptr, dA.ptr, nS * 4, _abi.HJB_COPY_D2D) == 0      # the output's halo planes are not touched
                        bk.evaluate_stage_device(dA, dLab.ptr + inner * b, dC)      # (one-byte labels: the owned planes start at inner * b)
                        bk.check_device_status()
                        got = dC.download(np.float32)
                        assert np.array_equal(got[inner * b:inner * e], want[inner * b:inner * e]), (s, i32, m24)
                        assert np.array_equal(got[:inner * b], JA[:inner * b]) and np.array_equal(got[inner * e:], JA[inner * e:])
    finally:
        for x in bufs:
            x.free()


def test_eval_form_is_read_only_and_follows_the_options(env):
    hjbdp, _abi, _ = env
    from problems import random_problem
    spec = random_problem(3, (6, 5, 4), (3, 2), dtype=np.float32)
    with hjbdp.Backup(spec) as bk:
        assert bk.get_option("eval_form") == 2                 # before anything was evaluated or built
        for i32, m24, form in [(1, 0, 1), (0, 1, 0), (0, 0, 0), (1, 1, 2)]:
            bk.set_option("eval_i32", i32)
            bk.set_option("eval_m24", m24)
            for s in (0, 1, -1):
                bk.set_option("eval_tables", s)
                assert bk.get_option("eval_form") == form
        for v in (0, 1, 2):
            with pytest.raises(hjbdp.HjbError) as ei:
                bk.set_option("eval_form", v)
            assert ei.value.status == _abi.HJB_E_INVALID
        assert bk.get_option("eval_form") == 2


def test_the_table_covers_both_sides_of_every_conjunct():
    """From the table itself: every conjunct of eval_runs_m24 is false in some row and, in another, true at 2^24 - 1; the two
    conjuncts of eval_runs_i32 on the grid's size are false in some row and true within 0.1 % of 2^31 - 2^26 in another.  A conjunct
    of one source counts only in rows whose source exists; and each row's stated forms follow from its stated false conjuncts."""
    rows = dict(CASES, j=SLAB_CASE)
    false_in, max_in = {}, {}
    for name, case in rows.items():
        f = _factors(case, SLAB if name == "j" else None)
        assert case["false"] == _false(case, SLAB if name == "j" else None), name
        for s, form in case["expect"].items():
            assert form == _model_form(case, s, SLAB if name == "j" else None), (name, s)
            for k in M24_ALWAYS + (M24_TABLES if s == 1 else M24_TERMS):
                if f[k] >= K24:
                    false_in.setdefault(k, name)
                if f[k] == K24 - 1 and form == 2:
                    max_in.setdefault(k, name)
            for k in I32:
                if f[k] >= LIM32:
                    false_in.setdefault(k, name)
                if LIM32 - NEAR32 <= f[k] < LIM32 and form != 0:
                    max_in.setdefault(k, name)
    every = set(M24_ALWAYS + M24_TABLES + M24_TERMS + I32)
    assert set(false_in) == every, sorted(every - set(false_in))
    assert set(max_in) == every, sorted(every - set(max_in))
    assert {c["storage"] for c in rows.values()} == {"f16", "f32"}
    assert 2 * sum(c["nonuniform"] for c in rows.values()) >= len(rows)
    assert all(len(set(c["n"])) == len(c["n"]) for k, c in rows.items() if k not in ("b", "e1"))      # unequal sizes (b, e1: 4096 twice, by their line)
