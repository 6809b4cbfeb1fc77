"""GPU tests (-m gpu) of K15's own dispatch (csrc/kernels_uniwin.h, variant 4 mode 7): every sweep-shape copy of the loop nest, every
level-1 row-pair form, the lone step of an odd level-1 count, the slow path and the edges of the chunk walk - on the constructed
problems of tests/uniwin_shapes.py, whose coverage tests/test_uniwin_shapes.py asserts without a device.

Per case, with float32 and with binary16 storage of the cost-to-go:
  * the device plan agrees with the restatement: uniwin_ok and uniwin_slow_points == plan_of(spec).slow.sum();
  * two stages equal the C twin's sweep bit for bit - K15 with the default walk, with the fixed stride (uw_claim 0), with 64-state
    chunks, with tiles of 1 x 2 x 1, 2 x 2 x 1 and 8 x 8 x 8 points, and K3's mode 5 on the same handle;
  * the first stage stays within the float32 bound of the float64 reference (oracle/hjb_oracle.py backup_stage on float64 terms) and
    takes its label wherever that reference decides it (uniwin_shapes.case_reference, bound_of).
No timing is asserted.

Largest error / bound against the float64 reference and the share of states left out of the label comparison, as measured on an
MI355X (float32 storage | binary16 storage; the binary16 bound is its half-ulp rounding, which some state nearly reaches):
    shapes-11        0.002  0.11 % | 0.960  2.26 %      cost-std          0.002  0.22 % | 0.958  3.97 %
    shapes-11-down   0.003  0.12 % | 0.972  2.45 %      cost-l0_first     0.002  0.22 % | 0.911  2.82 %
    shapes-12        0.011  0.17 % | 0.959  3.42 %      cost-l1_first     0.002  0.11 % | 0.921  2.15 %
    shapes-12-down   0.005  0.15 % | 0.974  3.39 %      cost-inner_first  0.002  0.22 % | 0.960  2.58 %
    shapes-12-knot   0.005  0.17 % | 0.974  5.03 %      cost-l1_per_o0    0.002  0.20 % | 0.937  2.26 %
    rows-12          0.007  0.35 % | 0.961  3.36 %      walk-128          0.004  0.16 % | 0.972  3.27 %
    rows-11          0.006  0.36 % | 0.966  5.96 %      walk-257          0.000  0.08 % | 0.978  2.52 %
    counts-1-1       0.000  0.15 % | 0.976  3.08 %      walk-300          0.001  0.13 % | 0.975  2.57 %
    counts-16-2      0.003  0.65 % | 0.943  7.88 %      walk-d5           0.006  0.12 % | 0.968  3.00 %
    counts-1-15      0.003  0.43 % | 0.952  4.82 %      walk-d6           0.005  0.16 % | 0.960  2.27 %
    counts-16-16     0.004  0.52 % | 0.895  2.95 %      ends              0.003  0.13 % | 0.959  2.33 %
    counts-3-17      0.006  0.67 % | 0.941  8.33 %      slow-mix-2 / -3   0.003  0.12 / 0.14 % | 0.972 / 0.957  3.08 / 2.01 %"""
import numpy as np
import pytest

import uniwin_shapes as US

pytestmark = pytest.mark.gpu

TILE_1x2x1, TILE_2x2x1, TILE_8x8x8 = 8, 9, 3 + 8 * 3 + 64 * 3
STORAGE = {"f32": None, "f16": np.float16}


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi, c_oracle


_TWIN = {}


def _twin(env, name, storage, stages=2):
    """The C twin's sweep of a case from its lattice terminal, once per module."""
    key = (name, storage, stages)
    if key not in _TWIN:
        _, _abi, c_oracle = env
        spec, term = US.case_reference(name, STORAGE[storage])[:2]
        _TWIN[key] = c_oracle.sweep(_abi, spec, stages, terminal=term, keep_J=True, keep_idx=True)
    return _TWIN[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(out, ref, what):
    assert out["J_stages"].dtype == ref["J_stages"].dtype
    for k in range(ref["J_stages"].shape[1] - 1, -1, -1):
        bad = np.flatnonzero(_bits(out["J_stages"][:, k]) != _bits(ref["J_stages"][:, k]))
        assert bad.size == 0, (what, "J", "stage column", k, bad.size, bad[:8].tolist())
        bad = np.flatnonzero(out["idx_stages"][:, k].astype(np.int64) != ref["idx_stages"][:, k])
        assert bad.size == 0, (what, "labels", "stage column", k, bad.size, bad[:8].tolist())


def _force_k15(bk, plan):
    """The automatic choice is K15 when at most 2 % of the points are slow (asserted either way); then K15 is forced on."""
    auto = int(plan["slow"].sum()) * 50 <= plan["slow"].size
    assert bk.get_option("uniwin") == (1 if auto else 0) and bk.get_option("packed2_mode") == (7 if auto else 5)
    bk.set_option("uniwin", 1)
    assert bk.get_option("packed2_mode") == 7 and bk.get_option("uniwin") == 1


_RATIOS = {}


def _against_float64(name, storage, J, idx):
    """One stage against the float64 reference: the value within the bound at every state, the label equal wherever the reference's
    runner-up is more than twice the bound above its minimum.  The bound comes from the formats and the reference alone."""
    spec, term, J64, lab64, bound, decided = US.case_reference(name, STORAGE[storage])
    err = np.abs(J.astype(np.float64) - J64)
    ratio = float((err / bound).max())
    left_out = 1.0 - float(decided.mean())
    _RATIOS[(name, storage)] = (ratio, left_out)
    print("%-18s %s  largest error / bound %.3f   left out of the label comparison %.2f %%" % (name, storage, ratio, 100 * left_out))
    assert left_out <= 0.10, (name, storage, left_out)
    worst = int(np.argmax(err / bound))
    assert ratio <= 1.0, (name, storage, ratio, worst, float(J[worst]), float(J64[worst]), float(bound[worst]))
    bad = np.flatnonzero(decided & (idx.astype(np.int64) != lab64))
    assert bad.size == 0, (name, storage, "labels against float64", bad.size, bad[:8].tolist())


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("name", US.RUN_CASES)
def test_case_every_walk_form_bit_exact_and_within_the_float64_bound(env, name, storage):
    hjbdp = env[0]
    spec, term = US.case_reference(name, STORAGE[storage])[:2]
    plan = US.plan_of(spec)
    assert int(plan["slow"].sum()) == US.CASES[name].slow and plan["exact"]
    ref = _twin(env, name, storage)
    solve = lambda bk: bk.solve(2, terminal=term, keep_J=True, keep_idx=True)
    with hjbdp.Backup(spec, variant=4) as bk:
        assert bk.info()["kernel_variant"] == 4
        assert bk.get_option("uniwin_ok") == 1
        assert bk.get_option("uniwin_slow_points") == int(plan["slow"].sum())
        _force_k15(bk, plan)
        assert bk.get_option("uw_claim") == 1 and bk.get_option("uw_block") == 256
        out = solve(bk)
        _same(out, ref, (name, storage, "K15, default walk"))
        bk.set_option("uw_claim", 0)
        assert bk.get_option("uw_claim") == 0 and bk.get_option("packed2_mode") == 7
        _same(solve(bk), ref, (name, storage, "K15, fixed stride"))
        bk.set_option("uw_claim", 1)
        bk.set_option("uw_block", 64)
        assert bk.get_option("uw_block") == 64 and bk.get_option("packed2_mode") == 7
        _same(solve(bk), ref, (name, storage, "K15, 64-state chunks"))
        bk.set_option("uw_block", 256)
        assert bk.get_option("uw_block") == 256
        for tile in (TILE_1x2x1, TILE_2x2x1, TILE_8x8x8):
            bk.set_option("uw_tile", tile)
            assert bk.get_option("packed2_mode") == 7
            _same(solve(bk), ref, (name, storage, "K15, uw_tile %d" % tile))
        bk.set_option("uw_tile", 0)
        bk.set_option("uniwin", 0)
        assert bk.get_option("packed2_mode") == 5 and bk.get_option("uniwin") == 0
        _same(solve(bk), ref, (name, storage, "mode 5"))
    _against_float64(name, storage, out["J_stages"][:, 1], out["idx_stages"][:, 1])


def test_cost_term_over_both_outer_control_dims_is_admitted(env):
    """The level-1 cost term of cost-l1_per_o0 has dims (D, D + 1): the host set-up admits it to K15 (cl1_per_o0: the term is
    reloaded per level-0 step) - mode 7 by the automatic choice, asserted here; the case itself runs with the others above."""
    hjbdp = env[0]
    spec = US.case_reference("cost-l1_per_o0")[0]
    assert any(t.dims == (spec.D, spec.D + 1) for t in spec.cost_terms)
    with hjbdp.Backup(spec, variant=4) as bk:
        assert bk.get_option("uniwin_ok") == 1 and bk.get_option("packed2_mode") == 7


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_seventeen_levels_are_not_admitted_and_mode_5_serves(env, storage):
    """counts-3-17: one level more than a plan record holds.  uniwin_ok == 0, forcing K15 on is refused, K3's mode 5 runs and equals
    the twin and the float64 reference."""
    hjbdp, _abi, c_oracle = env
    name = "counts-3-17"
    spec, term = US.case_reference(name, STORAGE[storage])[:2]
    assert not US.admitted(spec)
    ref = _twin(env, name, storage)
    with hjbdp.Backup(spec, variant=4) as bk:
        assert bk.info()["kernel_variant"] == 4
        assert bk.get_option("uniwin_ok") == 0 and bk.get_option("uniwin") == 0 and bk.get_option("packed2_mode") == 5
        with pytest.raises(hjbdp.HjbError) as e:
            bk.set_option("uniwin", 1)
        assert e.value.status == _abi.HJB_E_UNSUPPORTED
        assert bk.get_option("packed2_mode") == 5
        out = bk.solve(2, terminal=term, keep_J=True, keep_idx=True)
    _same(out, ref, (name, storage, "mode 5"))
    _against_float64(name, storage, out["J_stages"][:, 1], out["idx_stages"][:, 1])


@pytest.mark.parametrize("k", [2, 3])
def test_slow_mix_the_two_percent_rule(env, k):
    """100 points (5 x 5 x 4) of which exactly k take the slow path: 2 are 2 % - K15 by default; 3 are more - mode 5 by default
    (uniwin_auto, csrc/hjbdp_packed.hip).  Either way K15 forced on equals the twin (the case test above runs every walk form)."""
    hjbdp = env[0]
    name = "slow-mix-%d" % k
    spec, term = US.case_reference(name)[:2]
    plan = US.plan_of(spec)
    assert plan["slow"].size == 100 and int(plan["slow"].sum()) == k
    with hjbdp.Backup(spec) as bk:
        assert bk.info()["kernel_variant"] == 4 and bk.get_option("uniwin_ok") == 1 and bk.get_option("uniwin_slow_points") == k
        assert bk.get_option("uniwin") == (1 if k == 2 else 0) and bk.get_option("packed2_mode") == (7 if k == 2 else 5)
        auto = bk.solve(2, terminal=term, keep_J=True, keep_idx=True)
        bk.set_option("uniwin", 1)
        assert bk.get_option("packed2_mode") == 7
        forced = bk.solve(2, terminal=term, keep_J=True, keep_idx=True)
    _same(auto, _twin(env, name, "f32"), (name, "automatic"))
    _same(forced, _twin(env, name, "f32"), (name, "K15 forced on"))


@pytest.mark.parametrize("name", ["shapes-12", "ends"])
def test_slabs_with_and_without_a_halo_on_either_side(env, name):
    """The first slab (no halo below), the last (no halo above) and a middle one of the last axis: the owned planes equal the
    whole-grid stage bit for bit, labels included, and the handle reports mode 7.  The halos are one plane where the slab has a
    neighbour - two where the sweeps need them (an ascending sweep from plane l reads planes l + 1 and l + 2; halo_needed_lo / _hi
    of the whole-grid handle), never more planes than the grid has."""
    hjbdp, _abi, c_oracle = env
    spec, term = US.case_reference(name)[:2]
    nl = spec.n[-1]
    inner = spec.nS // nl
    whole = _twin(env, name, "f32")
    Jw, iw = whole["J_stages"][:, 1].reshape(inner, nl, order="F"), whole["idx_stages"][:, 1].reshape(inner, nl, order="F")
    T2 = term.reshape(inner, nl, order="F")
    with hjbdp.Backup(spec, variant=4) as bk:
        need = bk.info()
    for b, e, lo, hi in ((0, 2, 0, 1), (nl - 2, nl, 1, 0), (2, 4, 1, 1)):
        lo = min(max(lo, need["halo_needed_lo"]), b) if lo else 0
        hi = min(max(hi, need["halo_needed_hi"]), nl - e) if hi else 0
        with hjbdp.Backup(spec, slab=(b, e, lo, hi), variant=4) as bk:
            assert bk.get_option("uniwin_ok") == 1
            bk.set_option("uniwin", 1)
            assert bk.get_option("packed2_mode") == 7
            Jo, io = bk.backup_stage(np.asfortranarray(T2[:, b - lo:e + hi]).reshape(-1, order="F"))
        got = np.ascontiguousarray(Jo.reshape(inner, -1, order="F")[:, lo:lo + e - b])
        assert np.array_equal(_bits(got), _bits(np.ascontiguousarray(Jw[:, b:e]))), (name, b, e, lo, hi)
        bad = np.flatnonzero(io.astype(np.int64) != iw[:, b:e].reshape(-1, order="F"))
        assert bad.size == 0, (name, b, e, lo, hi, bad.size, bad[:8].tolist())


def test_long_sweep_on_a_walk_case_with_and_without_graph_replay(env):
    """Twelve stages of walk-257 (partial tiles, a last chunk of one state) through solve - the claim counters are reset by a memset
    node of the replayed graph every stage - each stage equal to the twin; then the same with graph 0."""
    hjbdp = env[0]
    name = "walk-257"
    spec, term = US.case_reference(name)[:2]
    ref = _twin(env, name, "f32", stages=12)
    with hjbdp.Backup(spec, variant=4) as bk:
        assert bk.get_option("packed2_mode") == 7 and bk.get_option("uw_claim") == 1
        _same(bk.solve(12, terminal=term, keep_J=True, keep_idx=True), ref, (name, "12 stages, graph replay"))
        bk.set_option("graph", 0)
        assert bk.get_option("packed2_mode") == 7
        _same(bk.solve(12, terminal=term, keep_J=True, keep_idx=True), ref, (name, "12 stages, graph 0"))
    assert len(np.unique(ref["idx_stages"][:, 0])) > 5 and np.all(np.isfinite(ref["J_stages"].astype(np.float64)))


def test_float64_figures_of_every_case_were_taken():
    """Runs after the cases above: the table of largest error-to-bound ratios and excluded shares, one line per case and storage."""
    want = {(n, s) for n in list(US.RUN_CASES) + ["counts-3-17"] for s in STORAGE}
    assert set(_RATIOS) == want, sorted(want - set(_RATIOS))
    for (n, s), (ratio, left_out) in sorted(_RATIOS.items()):
        print("%-18s %s  ratio %.3f  left out %.2f %%" % (n, s, ratio, 100 * left_out))
