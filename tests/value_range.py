"""Helpers of the value-range tests (tests/test_value_range_refs.py on the CPU, tests/test_gpu_value_range.py on the GPU): the
same problems as the parity suite's, with the cost-to-go moved into the regimes of the storage type that order-one data never
reach - subnormals, the normal / subnormal boundary, signed zeros, binary16's top binade and its overflow to infinity.

* half_rne: binary16 round-to-nearest-even from the float32 bit pattern in integer arithmetic, the independent reference of the
  store; census32: the float32 values it is checked on (every finite half, every midpoint and the midpoints' neighbours).
* scaled / range_terminal: a problem with every cost term times a power of two s, and a terminal of the same size with both zeros.
* the regimes `sub`, `edge`, `top`: a scale per (problem, regime) and a predicate over the oracle's stored stages that says the
  regime is one.  The predicates are conditions on the oracle's output, not tolerances: the kernels are held to the oracle's bits.
* the corpus: one small problem per kernel family and form (tests/test_gpu_launch_choice.py::_corpus is where most come from).

Not a conftest: nothing here is collected or changes how pytest runs."""
from __future__ import annotations

import ctypes as C

import numpy as np

STAGES = 3
SUB_SCALE_LOG2 = {np.dtype(np.float16): -20, np.dtype(np.float32): -140, np.dtype(np.float64): -1060}
EDGE_FIRST_LOG2 = {np.dtype(np.float16): -16, np.dtype(np.float32): -128, np.dtype(np.float64): -1024}
BITS = {np.dtype(np.float16): np.uint16, np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def bits(a):
    """The raw bits of a float array (so that -0 differs from +0 and a NaN equals itself)."""
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.dtype])


# ---- binary16 rounding in integer arithmetic -------------------------------------------------------------------------------------
def half_rne(x_f32):
    """float32 -> binary16 bit patterns (uint16), round to nearest, ties to even, written on the float32 bit pattern: subnormal
    results (the tie at 2^-25 goes to 0), overflow to infinity from 65520 upward, 65504 below that, NaN -> a quiet NaN."""
    u = np.ascontiguousarray(x_f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    sign = (u >> np.uint64(16)) & np.uint64(0x8000)
    a = u & np.uint64(0x7fffffff)
    exp = (a >> np.uint64(23)).astype(np.int64)                       # biased float32 exponent
    man = a & np.uint64(0x7fffff)
    # a normal half (exp >= 113 = 127 - 14): rebias, drop 13 bits; the carry of the rounding runs into the exponent
    m = np.where(exp >= 113, a - np.uint64(112 << 23), np.uint64(0))
    hn, rem = m >> np.uint64(13), m & np.uint64(0x1fff)
    hn = hn + ((rem > np.uint64(0x1000)) | ((rem == np.uint64(0x1000)) & ((hn & np.uint64(1)) == np.uint64(1)))).astype(np.uint64)
    hn = np.minimum(hn, np.uint64(0x7c00))                           # 65520 and above: infinity
    # a subnormal half: the 24-bit significand shifted right by 13 + (113 - exp) bits (float32 subnormals count as exp 1: all gone)
    sig = np.where(exp > 0, man | np.uint64(0x800000), man)
    sh = np.minimum(13 + (113 - np.maximum(exp, 1)), 40).astype(np.uint64)
    hs = sig >> sh
    rem = sig & ((np.uint64(1) << sh) - np.uint64(1))
    half = np.uint64(1) << (sh - np.uint64(1))
    hs = hs + ((rem > half) | ((rem == half) & ((hs & np.uint64(1)) == np.uint64(1)))).astype(np.uint64)
    h = np.where(exp >= 113, hn, hs)
    h = np.where(a == np.uint64(0x7f800000), np.uint64(0x7c00), h)
    h = np.where(a > np.uint64(0x7f800000), np.uint64(0x7e00), h)
    return (h | sign).astype(np.uint16)


def finite_halves():
    """Every finite binary16 bit pattern, both zeros included: 63,488 of them, in the order +0 .. +65504, -0 .. -65504."""
    b = np.arange(0x7c00, dtype=np.uint16)
    return np.concatenate([b, b | np.uint16(0x8000)])


def census32():
    """The float32 values the store is checked on: every finite half, the float32 midpoint between it and its successor in
    magnitude (65520 for 65504) with that midpoint's two float32 neighbours, +-2^-25 with its neighbours, +-65519.996, +-65520,
    +-65536 and +-FLT_MAX.  No NaN, no infinity."""
    h = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)
    nxt = np.concatenate([h[1:], np.float32([65536.0])])
    mid = (h + nxt) * np.float32(0.5)                                 # exact: a 12-bit significand
    assert np.array_equal(mid.astype(np.float64), (h.astype(np.float64) + nxt.astype(np.float64)) / 2)
    t = np.float32(2.0 ** -25)
    extra = np.float32([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)), 65519.996, 65520.0, 65536.0,
                        np.finfo(np.float32).max])
    pos = np.concatenate([h, mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf)), extra])
    out = np.concatenate([pos, -pos]).astype(np.float32)
    assert np.isfinite(out).all()
    return out


# ---- the scaled problem ----------------------------------------------------------------------------------------------------------
def scaled(spec, s):
    """The same problem with every cost term's data times the power of two s (in the terms' own type); knots, next-state terms,
    typing options, model, index_base, storage and disturbance unchanged."""
    import hjbdp
    from hjbdp import Term
    assert s > 0 and np.log2(s) == int(np.log2(s)), s
    cost = [Term(t.dims, t.data * t.data.dtype.type(s)) for t in spec.cost_terms]
    for t0, t1 in zip(spec.cost_terms, cost):
        assert t1.data.dtype == t0.data.dtype
    return hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, cost, dtype=spec.dtype, index_base=spec.index_base,
                             j_storage=None if spec.j_dtype == spec.dtype else spec.j_dtype, model=spec.model,
                             idx_dtype=spec.idx_dtype, table_dtype=spec.table_dtype, cost_dtype=spec.cost_dtype,
                             disturbance=spec.disturbance)


def range_terminal(spec, s, seed=0, n=None):
    """random_terminal * s cast to the storage type; every 10th entry is +0.0, every 20th entry, offset 5, is -0.0."""
    rng = np.random.default_rng(seed)
    t = (rng.random(spec.nS if n is None else n).astype(spec.dtype) * spec.dtype.type(s)).astype(spec.j_dtype)
    t[0::10] = 0.0
    t[5::20] = -0.0
    return t


# ---- the regimes -----------------------------------------------------------------------------------------------------------------
def shares(J):
    """Shares of a stored array: NaN, infinite, non-zero subnormal of its own type, finite in the top binade (binary16: >= 32768)."""
    J = np.asarray(J)
    a = np.abs(J.astype(np.float64)) if J.dtype != np.float64 else np.abs(J)
    fi = np.finfo(J.dtype)
    n = float(J.size)
    return {"nan": np.isnan(a).sum() / n, "inf": np.isinf(a).sum() / n,
            "sub": ((a > 0) & (a < float(fi.smallest_normal))).sum() / n,
            "top": (np.isfinite(a) & (a >= float(fi.max) / 2)).sum() / n}


def check_regime(regime, J, what=""):
    """The regime's predicate over the oracle's stored stages (a condition: a regime that is not one fails here)."""
    sh = shares(J)
    assert sh["nan"] == 0, (what, regime, sh)
    if regime == "sub":
        assert sh["inf"] == 0 and sh["sub"] >= 0.70, (what, regime, sh)
    elif regime == "edge":
        assert sh["inf"] == 0 and 0.10 <= sh["sub"] <= 0.90, (what, regime, sh)
    elif regime == "top":
        assert J.dtype == np.float16 and 0.02 <= sh["inf"] <= 0.40 and sh["top"] >= 0.25, (what, regime, sh)
    else:
        raise ValueError(regime)
    return sh


# Problems without a `top` regime: the pos-att channel's stage costs are below 1e-3 of a terminal in [0, s), so one stage returns
# values below the terminal's largest - and a finite binary16 terminal (s <= 2^15) then has no infinite output at all.  Variant 6
# in binary16 storage gets its `top` case from the column-sweep problem, which it also serves.
NO_TOP = ("posatt_ref_terms_f16s",)


def regimes_of(spec, name=None):
    return ("sub", "edge", "top") if spec.j_dtype == np.float16 and name not in NO_TOP else ("sub", "edge")


def oracle_sweep(abi, c_oracle, spec, n_stages, terminal, monitor_single=False):
    """orc_sweep with every stage kept, monitor_period 1, monitor_tol 0 and the oracle's progress calls [(k_s, e, e2)]."""
    lib = c_oracle.lib(abi)
    p, keep = spec.to_c()
    o, r = abi.hjb_solve_opts(), abi.hjb_result()
    o.n_stages, o.monitor_period, o.monitor_tol, o.monitor_single = n_stages, 1, 0.0, int(monitor_single)
    term = np.ascontiguousarray(terminal, dtype=spec.j_dtype)
    o.terminal = term.ctypes.data
    events = []
    cb = abi.hjb_progress_fn(lambda user, k_s, e, e2, sec: events.append((k_s, e, e2)))
    o.progress = cb
    J, idx = np.empty(spec.nS, dtype=spec.j_dtype), np.empty(spec.nS, dtype=np.int32)
    Js = np.zeros((spec.nS, n_stages), dtype=spec.j_dtype, order="F")
    Is = np.zeros((spec.nS, n_stages), dtype=np.int32, order="F")
    o.J_final, o.idx_final, o.J_stages, o.idx_stages = J.ctypes.data, idx.ctypes.data, Js.ctypes.data, Is.ctypes.data
    st = lib.orc_sweep(C.byref(p), C.byref(o), C.byref(r), lib.orc_max_threads())
    assert st == 0, st
    return {"J": J, "idx": idx, "J_stages": Js, "idx_stages": Is, "stages_done": r.stages_done, "stopped_early": bool(r.stopped_early),
            "last_e": r.last_e, "last_e2": r.last_e2, "events": events}


_REFS = {}


def regime_ref(abi, c_oracle, name, spec, regime, seed=11):
    """{k, spec (scaled by 2^k), terminal, stages, ref (oracle_sweep), shares} of one (problem, regime); the predicate is asserted.
    Computed once per process and shared (and left unchanged) by every test that needs it.

    sub: the fixed scale of the storage type.  edge: the power of two whose subnormal share over the three stages is nearest 50 %,
    found with the oracle (J is linear in s up to rounding, so the search starts from the median |J| of the unscaled sweep and
    walks while the distance to 50 % falls).  top: one stage; the smallest k with at least 2 % of the outputs infinite."""
    key = (name, regime)
    if key in _REFS:
        return _REFS[key]
    jd = np.dtype(spec.j_dtype)
    stages = 1 if regime == "top" else STAGES

    def run(k):
        sp = scaled(spec, 2.0 ** k)
        term = range_terminal(sp, 2.0 ** k, seed)
        assert np.isfinite(term.astype(np.float64)).all(), (name, regime, k)
        return sp, term, oracle_sweep(abi, c_oracle, sp, stages, term)

    if regime == "sub":
        k = SUB_SCALE_LOG2[jd]
        sp, term, ref = run(k)
    else:
        base = _REFS.get((name, "unit", stages))
        if base is None:
            base = _REFS[(name, "unit", stages)] = run(0)[2]
        a0 = np.abs(base["J_stages"].astype(np.float64))
        assert np.isfinite(a0).all(), (name, "the unscaled sweep is not finite")
        if regime == "edge":
            k = int(round(np.log2(float(np.finfo(jd).smallest_normal) / np.median(a0[a0 > 0]))))
            dist = lambda r: abs(shares(r[2]["J_stages"])["sub"] - 0.5)
            got = run(k)
            for step in (1, -1):
                while True:
                    nxt = run(k + step)
                    if dist(nxt) >= dist(got):
                        break
                    got, k = nxt, k + step
            sp, term, ref = got
        else:
            # the first k at which the largest unscaled output reaches 65520, then up to the 2 % share
            k = int(np.floor(np.log2(65520.0 / a0.max())))
            while shares(run(k - 1)[2]["J_stages"])["inf"] >= 0.02:
                k -= 1
            while True:
                sp, term, ref = run(k)
                if shares(ref["J_stages"])["inf"] >= 0.02:
                    break
                k += 1
                assert k < 40, (name, "no scale reaches the top regime")
    sh = check_regime(regime, ref["J_stages"], name)
    out = _REFS[key] = {"k": k, "spec": sp, "terminal": term, "stages": stages, "ref": ref, "shares": sh}
    return out


# ---- the identity stage ----------------------------------------------------------------------------------------------------------
IDENTITY_N = (257, 249)                    # 256 x 248 = 63,488 states that are not the last point of an axis


def identity_problem(storage):
    """D = 2, integer knots 0 .. n - 1, the next state is the knot itself (one term per axis over its own dim: t = 0 everywhere but
    at the last point of an axis), one control, one cost term that is -0.0: fma(0, v1 - v0, v0) + (-0) = v0."""
    import hjbdp
    from hjbdp import Term
    dtype = np.float64 if storage == "f64" else np.float32
    knots = [np.arange(n, dtype=np.float64) for n in IDENTITY_N]
    nxt = [[Term((a,), knots[a].copy())] for a in range(2)]
    cost = [Term((2,), np.array([-0.0]))]
    return hjbdp.ProblemSpec(knots, (1,), nxt, cost, dtype=dtype, index_base=1, j_storage=np.float16 if storage == "f16s" else None)


def identity_patterns(storage, seed=3):
    """The 63,488 values of the interior, positive half first and its mirror image second.  binary16: every finite half.  float32 /
    float64: 31,744 magnitudes - zero, then 15,871 subnormals spread over all binades of the subnormal range (its smallest and
    largest value among them), then normals from the smallest normal up to below 2^126 / 2^1022 with the exponent drawn uniformly."""
    if storage == "f16s":
        return finite_halves().view(np.float16)
    ft, ut, mbits, ebias = {"f32": (np.float32, np.uint32, 23, 127), "f64": (np.float64, np.uint64, 52, 1023)}[storage]
    rng = np.random.default_rng(seed)
    half = 0x7c00
    n_sub = half // 2 - 1
    binade = np.arange(n_sub) % mbits                                # the subnormal binades in turn
    lo = (np.uint64(1) << binade.astype(np.uint64))
    sub = lo + (rng.integers(0, 1 << 62, n_sub).astype(np.uint64) % lo)
    sub[0], sub[1] = 1, (1 << mbits) - 1
    n_nor = half - 1 - n_sub
    e = rng.integers(1, ebias + 126 if storage == "f32" else ebias + 1022, n_nor).astype(np.uint64)      # |v| < 2^126 / 2^1022
    nor = (e << np.uint64(mbits)) | (rng.integers(0, 1 << 62, n_nor).astype(np.uint64) & np.uint64((1 << mbits) - 1))
    nor[0] = 1 << mbits                                              # the smallest normal
    mag = np.concatenate([[np.uint64(0)], sub, nor]).astype(ut)
    sign = ut(1) << ut(8 * np.dtype(ut).itemsize - 1)
    return np.concatenate([mag, mag | sign]).view(ft)


def identity_input(storage, values=None):
    """The census on the interior of the 257 x 249 grid (column-major, 256 values per grid row), 0 at the last point of either
    axis.  -0 is the first value of the negative half: state (0, 124), whose upper neighbours along both axes are negative, which
    the claim needs: fma(+0, d, -0) is -0 only for d < 0 (for d > 0 the product is +0 and +0 + -0 = +0)."""
    v = identity_patterns(storage) if values is None else values
    n0, n1 = IDENTITY_N
    J = np.zeros((n0, n1), dtype=v.dtype, order="F")
    J[:n0 - 1, :n1 - 1] = v.reshape(n0 - 1, n1 - 1, order="F")
    if values is None:
        assert bits(J[0:1, 124])[0] == bits(np.array([-0.0], dtype=v.dtype))[0] and J[1, 124] < 0 and J[0, 125] < 0
    return J.reshape(-1, order="F")


def interior_mask(margin=1):
    """States further than `margin` - 1 points from the upper face of both axes (margin 1: not the last point of an axis)."""
    n0, n1 = IDENTITY_N
    m = np.zeros((n0, n1), dtype=bool, order="F")
    m[:n0 - margin, :n1 - margin] = True
    return m.reshape(-1, order="F")


def monitor_values(storage):
    """{name: values} - the census as the monitor's sums read it.  The whole census sums to zero exactly (every value has its mirror
    image), which a kernel that dropped the subnormals would also find, so it goes with a second array of magnitudes only, cut to
    the subnormals and the two lowest normal binades (larger magnitudes replaced by +0), where the subnormals carry a good part of the sum.
    binary16 `signed`: every finite half - the double sum of any part of it is exact (below 2^27 in units of 2^-24).  float32 /
    float64 `signed`: cut in the same way, so that every partial sum of the double monitor is exact whatever its order (the oracle
    states an order for the float32 tree and for float64 only) and no tree overflows."""
    v = identity_patterns(storage)
    low = v.copy()
    low[np.abs(low.astype(np.float64)) >= float(np.finfo(v.dtype).smallest_normal) * 4] = 0.0
    mag = np.abs(low)
    return {"signed": v if storage == "f16s" else low, "magnitudes": mag}


# ---- the corpus ------------------------------------------------------------------------------------------------------------------
class Case:
    """One handle form of the sweeps: the problem (by name, so that forms share the oracle's sweep), the variant and options to
    set after hjb_create, and the (kernel_variant, form, storage) triple it stands for."""

    def __init__(self, name, spec, variant, options=(), form="", check=None):
        self.name, self.spec, self.variant, self.options, self.form, self.check = name, spec, variant, tuple(options), form, check

    @property
    def storage(self):
        return {np.dtype(np.float16): "f16s", np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}[np.dtype(self.spec.j_dtype)]

    @property
    def id(self):
        return "%s-v%d%s" % (self.name, self.variant, ("-" + self.form) if self.form else "")

    @property
    def triple(self):
        return (self.variant, self.form, self.storage)


def respec(spec, **kw):
    import hjbdp
    args = dict(dtype=spec.dtype, index_base=spec.index_base, j_storage=None if spec.j_dtype == spec.dtype else spec.j_dtype,
                idx_dtype=spec.idx_dtype, table_dtype=spec.table_dtype, cost_dtype=spec.cost_dtype, model=spec.model)
    args.update(kw)
    return hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, **args)


def k15_problem(storage):
    from problems import rate_shared_problem
    return rate_shared_problem(31, (140,), (4, 3, 4), m=(3, 4, 11), gain=(0.3, 0.2, 0.25),
                               j_storage=np.float16 if storage == "f16s" else None)


_CASES = None


def sweep_cases():
    """Every family and form of the stage kernels with each storage type it is built for (the list of the module docstring of
    tests/test_gpu_value_range.py).  The three K15 entries of the launch corpus with 1,331 controls are left out: their oracle
    sweeps take minutes."""
    global _CASES
    if _CASES is not None:
        return _CASES
    import hjbdp
    from test_gpu_launch_choice import _corpus
    from problems import random_problem
    corpus = {name: spec for name, spec, slab in _corpus(hjbdp) if slab is None}
    f16 = lambda s: respec(s, dtype=np.float32, j_storage=np.float16)
    out = []
    # variant 0 (one state per thread) on every rand entry; variant 5 in both index forms on the C = 2 entries
    for name in sorted(n for n in corpus if n.startswith("rand_")):
        out.append(Case(name, corpus[name], 0))
        if "c2_" in name:
            for i32 in (1, 0):
                out.append(Case(name, corpus[name], 5, [("tabled_i32", i32)], "i32=%d" % i32))
    out.append(Case("tab64_rand", corpus["tab64_rand"], 5, [("tabled_i32", 1)], "tab64"))
    base = random_problem(32, (9, 8, 7), (4, 3), dtype=np.float64, index_base=1)
    out.append(Case("cost64_rand", respec(base, dtype=np.float32, cost_dtype=np.float64), 5, [("tabled_i32", 1)], "cost64"))
    # variant 3 (one wave per state): Kirk in both precisions, the smallest and the largest block
    for prec in ("single", "double"):
        for block in (256, 1024):
            out.append(Case("kirk_" + prec, corpus["kirk_" + prec], 3, [("temporal", 0), ("block", block)], "block=%d" % block))
    # variants 2 and 4: the packed modes 0, 1 / 4, 2 and 5, each problem also in binary16 storage (variant 2 is not built for it)
    for name in ("nested_c2", "nested_c2ctrl", "nested_mixed", "nested_win", "nested_win_mono"):
        for storage, spec in (("f32", corpus[name]), ("f16s", f16(corpus[name]))):
            nm = name if storage == "f32" else name + "_f16s"
            out.append(Case(nm, spec, 4, [], "mode"))
            if storage == "f32" and name != "nested_mixed":
                out.append(Case(nm, spec, 2, [], "mode"))
    # K15 (packed2_mode 7)
    for storage in ("f32", "f16s"):
        out.append(Case("k15_" + storage, k15_problem(storage), 4, [], "mode", check=lambda bk: bk.get_option("packed2_mode") == 7))
    # variant 6 (one wave per 64 states of a grid row), both forms
    for storage, spec in (("f32", corpus["posatt_ref_terms"]), ("f16s", f16(corpus["posatt_ref_terms"]))):
        for lean in (0, 1):
            out.append(Case("posatt_ref_terms" + ("" if storage == "f32" else "_f16s"), spec, 6, [("row_lean", lean)], "lean=%d" % lean))
    for lean in (0, 1):
        out.append(Case("cs_g3_f16s", corpus["cs_g3_f16s"], 6, [("row_lean", lean)], "lean=%d" % lean))
    # variant 7, the column sweep
    for name in ("cs_g3_fast", "cs_g2_fast", "cs_g3_multi", "cs_g3_step01", "cs_g3_f16s", "cs_cost64", "cs_cost64_step01"):
        out.append(Case(name, corpus[name], 7, [], "plan"))
    for name in ("cs_cost64", "cs_cost64_step01"):
        out.append(Case(name + "_f16s", f16(corpus[name]), 7, [], "plan"))
    for dpp in (0, 1):
        out.append(Case("cs_g3_fast", corpus["cs_g3_fast"], 7, [("cs_dpp", dpp)], "dpp=%d" % dpp))
    # the cooperative form, asked for on the corpus's entry (axis 1 moves with axis 3) and on its twin whose axis 1 moves with axis 2:
    # the host check admits the one whose axis is the group axis the plan picks (the form in effect is read back on the device)
    from problems import colsweep_problem
    twin = colsweep_problem(5, (128, 9, 8, 11), nU=9, gax=3, cost="fast", a1_axis=2, a1_amp=0.3)
    for name, base in (("cs_coop", corpus["cs_coop"]), ("cs_coop_a2", twin)):
        for storage, spec in (("f32", base), ("f16s", f16(base))):
            assert spec.n[0] == 128
            out.append(Case(name + ("" if storage == "f32" else "_f16s"), spec, 7, [("cs_coop", 1)], "coop"))
    _CASES = out
    return out


def slab_cases():
    """The two slab entries of the launch corpus: (name, spec, slab).  Their planes [begin, end) are the corpus's; the halos are
    what a stage needs (hjbdp.sharded.required_halo, clipped to the grid) - the corpus's own handles are never swept."""
    import hjbdp
    from hjbdp.sharded import required_halo
    from test_gpu_launch_choice import _corpus
    out = []
    for name, spec, slab in _corpus(hjbdp):
        if slab is not None:
            b, e = slab[:2]
            lo, hi = required_halo(spec)
            out.append((name, spec, (b, e, min(lo, b), min(hi, spec.n[-1] - e))))
    return out


def slab_input(spec, slab, term):
    """The haloed sub-array of a whole-grid terminal that a slab handle reads, and the slice of its owned planes."""
    b, e, hl, hh = slab
    inner = spec.nS // spec.n[-1]
    sub = np.asfortranarray(term.reshape(inner, -1, order="F")[:, b - hl:e + hh]).reshape(-1, order="F")
    return sub, slice(hl * inner, (hl + e - b) * inner)


def slab_ref(abi, c_oracle, name, regime):
    """{spec, slab, input, own, J, idx} of one slab entry in one regime: the regime's scaled problem and terminal (found on the
    whole grid), the haloed input of the slab and the oracle's stage of it, whose owned planes are asserted to be in the regime."""
    spec, slab = next((s, sl) for n, s, sl in slab_cases() if n == name)
    r = regime_ref(abi, c_oracle, name, spec, regime)
    sub, own = slab_input(r["spec"], slab, r["terminal"])
    Jr, ir = c_oracle.backup_stage(abi, r["spec"], sub, slab=slab)
    sh = shares(Jr[own])
    assert sh["nan"] == sh["inf"] == 0 and sh["sub"] >= (0.7 if regime == "sub" else 0.1), (name, regime, sh)
    return {"spec0": spec, "spec": r["spec"], "slab": slab, "input": sub, "own": own, "J": Jr, "idx": ir}


# (the batched column sweep is built for float32 storage only)
BATCHES = [("rand_d3c2_f32", 5), ("rand_d3c2_f16s", 5), ("rand_d3c2_f64", 5), ("cs_g3_fast", 7)]


def batch_members(abi, c_oracle, name):
    """[(n_stages, [(spec, terminal, oracle_sweep)] x 3)]: batches of the same problem in three different regimes - sub, edge and
    the unscaled problem over three stages; with binary16 storage also sub, top and the unscaled problem over one stage.  Each
    member is asserted to be in its regime (the last stage of `edge` alone may lie on either side: its share is one of three stages)."""
    spec = next(c.spec for c in sweep_cases() if c.name == name)
    groups = [(STAGES, ("sub", "edge", "unit"))] + ([(1, ("sub", "top", "unit"))] if spec.j_dtype == np.float16 else [])
    out = []
    for n_st, regimes in groups:
        members = []
        for regime in regimes:
            if regime == "unit":
                sp, term = spec, range_terminal(spec, 1.0, 11)
            else:
                r = regime_ref(abi, c_oracle, name, spec, regime)
                sp, term = r["spec"], r["terminal"]
            o = oracle_sweep(abi, c_oracle, sp, n_st, term)
            sh = shares(o["J_stages"])
            assert sh["nan"] == 0, (name, regime, sh)
            if regime == "unit":
                assert sh["sub"] == 0 and sh["inf"] == 0, (name, regime, sh)
            else:
                check_regime(regime, o["J_stages"], name)
            members.append((sp, term, o))
        out.append((n_st, members))
    return out


# ---- the other readers and writers of stored J: the fixed-label stage, the disturbed stage, the lookup --------------------------
def one_stage_scale(regime, j_dtype, J_unit):
    """log2 of the scale of a one-stage case: the regime's fixed scale for `sub`; for `edge` the power of two that puts the median
    |J| of the reference's own unscaled output on the smallest normal (J is linear in the scale)."""
    jd = np.dtype(j_dtype)
    if regime == "sub":
        return SUB_SCALE_LOG2[jd]
    a = np.abs(np.asarray(J_unit, dtype=np.float64))
    return int(round(np.log2(float(np.finfo(jd).smallest_normal) / np.median(a[a > 0]))))


def stored(J, j_dtype):
    """J of the arithmetic type as the kernels store it: binary16 through half_rne (not numpy's conversion)."""
    return half_rne(J).view(np.float16) if np.dtype(j_dtype) == np.float16 else np.asarray(J, dtype=j_dtype)


_ONE_STAGE = {}


def _one_stage(key, regime, spec, ref_of, seed):
    """ref_of(scaled spec, terminal) -> (J in the arithmetic type, labels or None).  The scaled spec, its terminal and the stored
    reference of one regime, the regime's predicate asserted; shared through _ONE_STAGE."""
    if (key, regime) not in _ONE_STAGE:
        def at(k):
            sp = scaled(spec, 2.0 ** k)
            term = range_terminal(sp, 2.0 ** k, seed)
            J, lab = ref_of(sp, term)
            return {"k": k, "spec": sp, "terminal": term, "J": stored(J, spec.j_dtype), "labels": lab}
        k = one_stage_scale(regime, spec.j_dtype, ref_of(spec, range_terminal(spec, 1.0, seed))[0])
        if regime == "edge":                           # the neighbouring powers of two as well: the one nearest a 50 % share
            c = min((at(k + d) for d in (0, -1, 1, -2, 2)), key=lambda c: abs(shares(c["J"])["sub"] - 0.5))
        else:
            c = at(k)
        c["shares"] = check_regime(regime, c["J"], key)
        _ONE_STAGE[(key, regime)] = c
    return _ONE_STAGE[(key, regime)]


def k22_case(storage, regime):
    """The fixed-label stage on the smallest problem of tests/test_gpu_evaluate.py's random-label cases (9 x 7 x 6 states, 4
    controls), seeded random labels, held to evaluate_refs.evaluate_ref(lerp="fma"): the exact fma (float32: repaired double
    rounding; float64: rationals), which rounds correctly into the subnormals."""
    from evaluate_refs import evaluate_ref, oracle_problem
    from problems import random_problem
    dtype = np.float64 if storage == "f64" else np.float32
    spec = respec(random_problem(903, (9, 7, 6), (4,), dtype=dtype, index_base=1), idx_dtype="auto",
                  j_storage=np.float16 if storage == "f16s" else None)
    lab0 = np.random.default_rng(77).integers(0, spec.nU, spec.nS)

    def ref_of(sp, term):
        return evaluate_ref(oracle_problem(sp), term.astype(dtype), lab0, lerp="fma").reshape(-1, order="F"), None
    out = dict(_one_stage(("k22", storage), regime, spec, ref_of, 9))
    out["labels"] = (lab0 + 1).astype(spec.idx_np_dtype)
    return out


K24_TYPINGS = {"f16": 8, "f32": 2, "f64": 5, "q64_f16": 12, "q64_f32": 9}          # kernel stage_disturb_<key>: row of REF_CASES


def k24_case(kernel, mode, regime):
    """The disturbed stage on the smallest case of tests/test_gpu_disturbance.py::REF_CASES for each of its five kernels, held to
    disturbance_refs.DisturbedRef.  float64: the reference's fma goes through rationals (evaluate_refs._fma64) - its
    error-free-transformation form is stated for values that do not underflow."""
    import hjbdp
    from disturbance_refs import DisturbedRef
    from evaluate_refs import _fma64
    from test_gpu_disturbance import REF_CASES, _offsets, _ref_spec, _weights
    typing, n, m, nonuniform, axes, W, seed = REF_CASES[K24_TYPINGS[kernel]]
    assert typing == {"f16": "f16", "f32": "f32", "f64": "f64", "q64_f16": "tab64+f16", "q64_f32": "tab64"}[kernel]
    spec = _ref_spec(hjbdp, typing, n, m, nonuniform, seed)
    off = _offsets(spec, tuple(range(spec.D)) if axes is None else axes, W, seed)
    w = _weights(W, seed) if mode == "expect" and W > 1 else None

    def ref_of(sp, term):
        ref = DisturbedRef(sp, off, w, mode)
        if sp.dtype == np.float64:
            ref.fma = lambda a, b, c: _fma64(*(np.ascontiguousarray(np.broadcast_to(x, np.broadcast(a, b, c).shape)) for x in (a, b, c)))
        J, lab = ref.backup(term)
        return J.astype(sp.dtype), lab
    out = dict(_one_stage(("k24", kernel, mode), regime, spec, ref_of, seed))
    out.update(offsets=off, weights=w, mode=mode)
    return out


def lookup_case(dt, regime, seed=5):
    """A 3-D value table (2 x 5 x 3 knots, as tests/test_gpu_aux_kernels.py builds it) of subnormal values (`sub`: standard normal
    values times the regime's scale) or of values on both sides of the smallest normal (`edge`: times the smallest normal), with
    points in, on and around the grid -> (knots, V, points)."""
    from test_gpu_aux_kernels import _lookup_grid, _lookup_points
    dtype = np.dtype({"f32": np.float32, "f64": np.float64}[dt])
    rng = np.random.default_rng(seed)
    knots, V = _lookup_grid(rng, 3, dtype)
    pts = _lookup_points(rng, knots, dtype, n_random=500)
    s = 2.0 ** SUB_SCALE_LOG2[dtype] if regime == "sub" else float(np.finfo(dtype).smallest_normal)
    V = (V * dtype.type(s)).astype(dtype)
    check_regime(regime, V, ("lookup", dt))
    return knots, V, pts


def lookup_tol(dtype, D, V, w):
    """float64_refs.linear_tol with the value scale max|V| replaced by max(max|V|, the smallest normal): below the normals a
    rounding is an absolute step of the smallest subnormal, eps times the smallest normal, not eps times the value."""
    from float64_refs import linear_tol
    return linear_tol(dtype, D, max(float(np.max(np.abs(V))), float(np.finfo(dtype).smallest_normal)), w)
