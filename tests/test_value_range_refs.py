"""CPU tests of tests/value_range.py: the references and regimes that tests/test_gpu_value_range.py holds the kernels to.

* half_rne (binary16 rounding written on the float32 bit pattern) equals numpy's conversion on the whole census: every finite half,
  every midpoint between neighbouring halves and the midpoints' float32 neighbours, the tie at 2^-25, 65519.996 / 65520 / 65536 and
  FLT_MAX, both signs - and on the cases named one by one.
* scaled() changes the cost terms only; range_terminal() carries both zeros.
* every regime is one: for each problem the GPU file sweeps, the oracle's stored stages at the regime's scale satisfy the regime's
  predicate (value_range.check_regime) and hold no NaN.  A regime that stops being one fails here, on the CPU, not silently on the
  GPU.  The figures are printed (-s shows them).
* the identity problem's census holds what the GPU test says it holds, and the oracle returns it bit for bit."""
import numpy as np
import pytest

import value_range as vr


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    return hjbdp, _abi, c_oracle


# ---- half_rne --------------------------------------------------------------------------------------------------------------------
def test_half_rne_equals_numpy_on_the_census():
    x = vr.census32()
    assert 2.5e5 < x.size < 2.7e5 and x.dtype == np.float32
    with np.errstate(over="ignore"):
        ref = x.astype(np.float16).view(np.uint16)
    got = vr.half_rne(x)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (bad.size, x[bad[:8]], got[bad[:8]], ref[bad[:8]])
    # the census reaches what it is for
    assert set(np.unique(ref)) == set(range(0x7c01)) | set(range(0x8000, 0xfc01))             # every finite half and both infinities
    sub = (ref & 0x7c00) == 0
    assert (sub & ((ref & 0x3ff) != 0)).sum() > 4000 and (x[sub] != x[sub].astype(np.float16)).any()      # subnormal results, rounded ones


def test_half_rne_named_cases():
    f = lambda v: int(vr.half_rne(np.float32([v]))[0])
    t = np.float32(2.0 ** -25)
    assert f(t) == 0x0000 and f(-t) == 0x8000                                  # the tie between 0 and the smallest subnormal: even
    assert f(np.nextafter(t, np.float32(1))) == 0x0001 and f(np.nextafter(t, np.float32(0))) == 0x0000
    assert f(3 * t) == 0x0002                                                   # the tie between 1 and 2 units: even
    assert f(0.0) == 0x0000 and f(-0.0) == 0x8000
    assert f(2.0 ** -14) == 0x0400 and f(np.nextafter(np.float32(2.0 ** -14), np.float32(0))) == 0x0400     # rounds up into the normals
    assert f(2.0 ** -14 - 2.0 ** -25) == 0x0400 and f(2.0 ** -14 - 2.0 ** -24) == 0x03ff
    assert f(65504.0) == 0x7bff and f(65519.996) == 0x7bff and f(65520.0) == 0x7c00 and f(-65520.0) == 0xfc00
    assert f(65536.0) == 0x7c00 and f(np.finfo(np.float32).max) == 0x7c00 and f(np.inf) == 0x7c00
    assert f(1e-45) == 0x0000 and f(np.float32(2.0 ** -126)) == 0x0000          # float32 subnormals and tiny normals vanish
    assert (f(np.nan) & 0x7c00) == 0x7c00 and (f(np.nan) & 0x3ff) != 0
    rng = np.random.default_rng(0)
    x = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = x[~np.isnan(x)]
    with np.errstate(over="ignore"):
        assert np.array_equal(vr.half_rne(x), x.astype(np.float16).view(np.uint16))


# ---- scaled / range_terminal -----------------------------------------------------------------------------------------------------
def test_scaled_changes_the_cost_terms_only(env):
    from problems import colsweep_problem
    spec = vr.respec(colsweep_problem(6, (70, 9, 8, 11), nU=9, gax=3, cost="fast", dtype=np.float64), dtype=np.float32,
                     cost_dtype=np.float64, j_storage=np.float16, idx_dtype="auto")
    s = 2.0 ** -20
    sp = vr.scaled(spec, s)
    for f in ("dtype", "j_dtype", "cost_dtype", "table_dtype", "idx_dtype", "index_base", "n", "m", "model", "disturbance"):
        assert getattr(sp, f) == getattr(spec, f), f
    assert all(np.array_equal(a, b) for a, b in zip(sp.knots, spec.knots))
    for ta, tb in zip(sum(sp.next_terms, []), sum(spec.next_terms, [])):
        assert ta.dims == tb.dims and ta.data.dtype == tb.data.dtype and np.array_equal(ta.data, tb.data)
    assert len(sp.cost_terms) == len(spec.cost_terms)
    for ta, tb in zip(sp.cost_terms, spec.cost_terms):
        assert ta.dims == tb.dims and ta.data.dtype == tb.data.dtype == np.float64 and np.array_equal(ta.data, tb.data * s)
    with pytest.raises(AssertionError):
        vr.scaled(spec, 3.0)


def test_range_terminal_carries_both_zeros(env):
    from problems import random_problem, random_terminal
    for kw, k in ((dict(dtype=np.float32, j_storage=np.float16), -20), (dict(dtype=np.float32), -140), (dict(dtype=np.float64), -1060)):
        spec = vr.respec(random_problem(1, (12, 10), (5,), dtype=np.float64), **kw)
        t = vr.range_terminal(spec, 2.0 ** k, 4)
        assert t.dtype == spec.j_dtype and t.size == spec.nS
        b, sign = vr.bits(t), vr.bits(np.array([-0.0], dtype=t.dtype))[0]
        i = np.arange(t.size)
        assert (b[i % 10 == 0] == 0).all() and (b[i % 20 == 5] == sign).all()
        rest = (i % 10 != 0) & (i % 20 != 5)
        want = (random_terminal(spec, 4) * spec.dtype.type(2.0 ** k)).astype(spec.j_dtype)
        assert np.array_equal(t[rest], want[rest])
        sh = vr.shares(t[rest])
        assert sh["sub"] > 0.9 and sh["nan"] == sh["inf"] == 0, sh


# ---- the regimes -----------------------------------------------------------------------------------------------------------------
def _problems():
    seen, out = set(), []
    for c in vr.sweep_cases():
        if c.name not in seen:
            seen.add(c.name)
            out.append((c.name, c.spec))
    for name, spec, slab in vr.slab_cases():
        out.append((name, spec))
    return out


def test_every_regime_is_one_on_every_problem_the_gpu_file_sweeps(env):
    """One test over the whole corpus (the sweeps are shared through value_range.regime_ref; the K15 entries with 1,331 controls are
    not in it).  Every failing (problem, regime) is reported, not the first only."""
    _, _abi, c_oracle = env
    bad, rows = [], []
    for name, spec in _problems():
        for regime in vr.regimes_of(spec, name):
            try:
                r = vr.regime_ref(_abi, c_oracle, name, spec, regime)
            except AssertionError as e:
                bad.append((name, regime, str(e)[:300]))
                continue
            sh = r["shares"]
            rows.append("%-24s %-5s 2^%-6d sub %5.1f %%  inf %5.1f %%  top %5.1f %%" % (name, regime, r["k"], 100 * sh["sub"], 100 * sh["inf"],
                                                                                  100 * sh["top"]))
            assert r["ref"]["stages_done"] == r["stages"] and not r["ref"]["stopped_early"]
            assert len(r["ref"]["events"]) == r["stages"]
            if regime == "edge":
                assert r["k"] != vr.SUB_SCALE_LOG2[np.dtype(spec.j_dtype)]
    print("\n" + "\n".join(rows))
    assert not bad, "\n".join(map(str, bad))
    ks = {(np.dtype(spec.j_dtype).name, regime): set() for name, spec in _problems() for regime in vr.regimes_of(spec, name)}
    for name, spec in _problems():
        for regime in vr.regimes_of(spec, name):
            ks[(np.dtype(spec.j_dtype).name, regime)].add(vr.regime_ref(_abi, c_oracle, name, spec, regime)["k"])
    print(sorted((k, sorted(v)) for k, v in ks.items()))
    assert len(ks[("float16", "edge")]) > 1                              # one fixed scale does not do


def test_slab_and_batch_members_are_in_their_regimes(env):
    """The conditions the GPU file's slab and batch cases stand for (asserted inside the helpers)."""
    _, _abi, c_oracle = env
    for name, spec, slab in vr.slab_cases():
        for regime in vr.regimes_of(spec, name):
            s = vr.slab_ref(_abi, c_oracle, name, regime)
            assert s["input"].size > s["J"][s["own"]].size > 0
    for name, variant in vr.BATCHES:
        groups = vr.batch_members(_abi, c_oracle, name)
        assert len(groups) == (2 if name.endswith("f16s") else 1)
        for n_st, members in groups:
            assert len(members) == 3 and len({vr.bits(term).tobytes() for _, term, _ in members}) == 3


def test_the_regimes_reach_signed_zeros(env):
    """The terminal's -0 and +0 entries are read by the first stage, and the `sub` regime of binary16 stores zeros and the smallest
    subnormal (values that underflow in the store)."""
    _, _abi, c_oracle = env
    name, spec = next((n, s) for n, s in _problems() if n == "rand_d3c2_f16s")
    r = vr.regime_ref(_abi, c_oracle, name, spec, "sub")
    b = vr.bits(r["ref"]["J_stages"])
    assert (vr.bits(r["terminal"]) == 0x8000).any() and (vr.bits(r["terminal"]) == 0).any()
    assert ((b & 0x7fff) < 0x0400).mean() > 0.7 and np.unique(b).size > 50


# ---- the identity stage ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f16s", "f32", "f64"])
def test_identity_census_and_the_oracle(env, storage):
    _, _abi, c_oracle = env
    v = vr.identity_patterns(storage)
    assert v.size == 256 * 248 == 63488 and np.isfinite(v.astype(np.float64)).all()
    b = vr.bits(v)
    sign = vr.bits(np.array([-0.0], dtype=v.dtype))[0]
    assert (b == 0).sum() == 1 and (b == sign).sum() == 1
    fi = np.finfo(v.dtype)
    a = np.abs(v.astype(np.float64))
    if storage == "f16s":
        assert np.array_equal(np.sort(b), np.sort(vr.finite_halves()))
    else:
        subn = (a > 0) & (a < float(fi.smallest_normal))
        assert subn.sum() == 2 * 15871 and a.max() < 2.0 ** (126 if storage == "f32" else 1022)
        binades = np.unique(np.frexp(a[subn])[1])
        assert binades.size == fi.nmant and float(fi.smallest_subnormal) in a and float(fi.smallest_normal) in a
    spec = vr.identity_problem(storage)
    J_in = vr.identity_input(storage)
    Jo, idx = c_oracle.backup_stage(_abi, spec, J_in)
    m = vr.interior_mask()
    assert m.sum() == 63488 and np.array_equal(vr.bits(Jo)[m], vr.bits(J_in)[m])
    assert np.isfinite(Jo.astype(np.float64)).all() and (idx == 1).all()
    # +0 as the cost instead loses the -0 pattern (and nothing else): what the -0.0 cost is for
    from hjbdp import Term
    import hjbdp
    plus = hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, [Term((2,), np.array([0.0]))], dtype=spec.dtype, index_base=1,
                             j_storage=None if storage != "f16s" else np.float16)
    Jp, _ = c_oracle.backup_stage(_abi, plus, J_in)
    diff = np.flatnonzero((vr.bits(Jp) != vr.bits(J_in)) & m)
    assert diff.size == 1 and vr.bits(J_in)[diff[0]] == sign and vr.bits(Jp)[diff[0]] == 0
    # the monitor's census: finite sums in either precision, zero for the signed one, carried by the subnormals for the magnitudes
    for name, vals in vr.monitor_values(storage).items():
        w = vr.identity_input(storage, vals)
        for single in (False, True):
            s, _ = c_oracle.monitor_sums(_abi, spec, w, np.ones(w.size, dtype=np.int32), single=single)
            assert np.isfinite(s) and (s > 0 or name == "signed"), (name, single, s)
        if name == "magnitudes":
            a = np.abs(w.astype(np.float64))
            assert a[a < float(fi.smallest_normal)].sum() > 0.05 * a.sum()


# ---- the other readers and writers of stored J -----------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["sub", "edge"])
def test_one_stage_references_are_in_their_regimes(env, regime):
    """The references of the fixed-label stage, the disturbed stage and the lookup at the scales the GPU file uses (the predicates
    are asserted where the cases are built)."""
    for storage in ("f16s", "f32", "f64"):
        c = vr.k22_case(storage, regime)
        assert c["J"].dtype == c["spec"].j_dtype and c["labels"].min() >= 1
    for kernel in vr.K24_TYPINGS:
        for mode in ("expect", "worst"):
            c = vr.k24_case(kernel, mode, regime)
            assert c["J"].dtype == c["spec"].j_dtype and c["labels"].dtype == c["spec"].idx_np_dtype
    for dt in ("f32", "f64"):
        knots, V, pts = vr.lookup_case(dt, regime)
        from float64_refs import linear_ref
        ref, w = linear_ref(knots, V, pts)
        assert np.isfinite(ref).all() and (ref != 0).mean() > 0.9
        assert np.all(vr.lookup_tol(V.dtype, 3, V, w) < 1e-4 * float(np.finfo(V.dtype).smallest_normal) * w)


def test_rational_fma_equals_the_error_free_one_where_both_hold(env):
    """evaluate_refs._fma64 (what the float64 disturbed reference uses here) against disturbance_refs.fma64 on normal values."""
    from disturbance_refs import fma64
    from evaluate_refs import _fma64
    rng = np.random.default_rng(1)
    a, b, c = rng.standard_normal(500), rng.standard_normal(500), rng.standard_normal(500) * 1e-3
    assert np.array_equal(_fma64(a, b, c), fma64(a, b, c))
    t, d, v0 = np.float64(0.3), np.float64(3e-320), np.float64(1e-320)               # and into the subnormals: one rounding
    from fractions import Fraction
    assert _fma64(np.array([t]), np.array([d]), np.array([v0]))[0] == float(Fraction(t) * Fraction(d) + Fraction(v0))
