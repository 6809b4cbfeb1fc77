"""The placement generators of tests/problems.py meet their own conditions (no GPU, no library call beyond ProblemSpec): every
next-state query is recomputed in numpy - the terms' ordered sum in the type the queries are formed in - and classified against the
knots.  tests/test_gpu_placements.py runs the stage kernels on exactly these problems; what is asserted here is what makes those
runs mean something: queries ON knots, one unit in the last place beside them, on the first and the last knot, beyond either end,
and queries whose arithmetic first guess (find_cell, csrc/hjbdp_canon.h) is short of the cell or past it."""
import numpy as np
import pytest

import problems as P
from float64_refs import ordered_sum


@pytest.mark.parametrize("dtype,want", [
    (np.float32, dict(on_knot=45, ulp_below=7, ulp_above=7, first_knot=3, last_knot=3, outside=6, guess_short=7, guess_far=4)),
    (np.float64, dict(on_knot=27, ulp_below=6, ulp_above=8, first_knot=3, last_knot=1, outside=6, guess_short=10, guess_far=7)),
])
def test_the_thirteen_knot_grid_gives_the_recorded_counts(dtype, want):
    """linspace(-1, 1, 13) and the 65 sums fl(k_i + fl(s h)), s in -2 .. 2: the counts the grid was chosen for.  Another grid must
    come with the same table (linspace(-1, 1, 11) in float32 never guesses far, linspace(-0.7, 0.9, 14) in float64 never short)."""
    k = P.placement_knots(dtype)
    h = (k[-1] - k[0]) / 12
    q = ordered_sum([np.broadcast_to(k[:, None], (13, 5)), np.broadcast_to((np.array(P.PLACEMENT_STEPS) * h)[None, :], (13, 5))], dtype)
    got = P.placement_counts(k, q, dtype)
    assert {name: got[name] for name in want} == want
    assert got["guess_short2"] == 0 and got["guess_far2"] == 0          # an even grid's guess is never two cells off


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_nearly_uniform_grids_sit_either_side_of_the_hosts_rule(dtype):
    """'near' is flagged uniform by upload_axes (deviation <= 1.5 mean steps) with the guess two cells off either way; 'far' is not."""
    for grid, lo, hi in (("near", 1.3, 1.5), ("far", 1.5, 1.7)):
        k = P.placement_knots(dtype, grid)
        assert lo < P.placement_deviation(k) < hi
        assert np.array_equal(k, k.astype(dtype).astype(np.float64)) and np.all(np.diff(k) > 0)
        assert k[0] == -1.0 and k[-1] == 1.0
    k = P.placement_knots(dtype, "near")
    cells = P.placement_cells(k, k)
    guess = P.placement_guess(k, k, dtype)
    assert np.min(guess - cells[np.arange(13)]) <= -2              # on the knots themselves the guess is already two short


def test_queries_are_the_ordered_sum_in_the_locate_type():
    """placement_queries is float64_refs.ordered_sum over the terms as the spec holds them."""
    for name in ("free-4-float32", "free-2-tab64", "nested-3-float64-dec", "rates-even", "local2d-f32-u4"):
        spec = P.PLACEMENT_CASES[name][0]()
        g = spec.n + spec.m
        dt = P.locate_dtype(spec)
        for a in range(spec.D):
            parts = [np.broadcast_to(np.asarray(t.data).reshape([g[d] if d in t.dims else 1 for d in range(len(g))]), g)
                     for t in spec.next_terms[a]]
            assert np.array_equal(P.placement_queries(spec, a), ordered_sum(parts, dt)), (name, a)


@pytest.mark.parametrize("name", sorted(P.PLACEMENT_CASES))
def test_every_registered_problem_meets_its_conditions(name):
    """Per located axis and type: every class occurs (even grid); the guess is two or more cells off in each direction (near
    grid); the monotone variants decide a one-sided crossing at equality - increasing: the cell changes with the query exactly on
    the new cell's lower knot; decreasing: the query comes down onto a knot and must stay in that knot's cell."""
    spec, counts = P.placement_case(name)
    build, axes, grid, mono, classes = P.PLACEMENT_CASES[name]
    assert axes and all(spec.n[a] == P.PLACEMENT_N for a in axes)
    assert all(n <= P.PLACEMENT_N for n in spec.n[1:]) and (spec.n[0] <= P.PLACEMENT_N or name.startswith("row"))
    if mono:
        assert counts["crossings"] >= 1


def test_identity_problems_return_every_node_to_itself():
    """One control, displacement +0 on every axis: every query IS its state's knot, bit for bit."""
    for name in sorted(P.PLACEMENT_CASES):
        if not name.startswith("identity"):
            continue
        spec = P.PLACEMENT_CASES[name][0]()
        assert spec.nU == 1
        for a in range(spec.D):
            q = P.placement_queries(spec, a)[..., 0]
            k = spec.knots[a].astype(spec.dtype).reshape([-1 if d == a else 1 for d in range(spec.D)])
            assert np.array_equal(q, np.broadcast_to(k, spec.n))
            assert not np.signbit(np.asarray(spec.next_terms[a][1].data)).any()


def test_local_problems_are_local():
    """K9's rule (examine_tile2d): every query's cell is the state's own or the one below, on both axes."""
    for name in sorted(P.PLACEMENT_CASES):
        if not name.startswith("local2d"):
            continue
        spec = P.PLACEMENT_CASES[name][0]()
        dt = P.locate_dtype(spec).type
        for a in range(2):
            k = spec.knots[a].astype(dt)
            c = P.placement_cells(k, np.asarray(P.placement_queries(spec, a)).astype(dt))
            i = np.arange(spec.n[a]).reshape([-1 if d == a else 1 for d in range(c.ndim)])
            assert np.all((c >= np.maximum(i - 1, 0)) & (c <= np.minimum(i, spec.n[a] - 2))), (name, a)


def test_old_generators_are_untouched():
    """The default arguments of the generators that were here before keep producing the same problems (a digest of their terms)."""
    import hashlib

    def digest(spec):
        h = hashlib.sha256()
        for k in spec.knots:
            h.update(np.ascontiguousarray(k).tobytes())
        for ts in spec.next_terms + [spec.cost_terms]:
            for t in ts:
                h.update(repr(t.dims).encode() + np.ascontiguousarray(t.data).tobytes())
        return h.hexdigest()[:16]

    got = {"random": digest(P.random_problem(1, (5, 4), (3,))), "nested": digest(P.nested_problem(1, (5, 4), (3,))),
           "colsweep": digest(P.colsweep_problem(1, (6, 5, 4, 5))), "rates": digest(P.rate_shared_problem(1, (4,), (4, 3, 4), m=(3, 3, 3)))}
    assert got == OLD_DIGESTS, got


OLD_DIGESTS = {'random': 'd04d83a4b5fd3db6', 'nested': '987cc05763b171d3', 'colsweep': '3da2ab56de6e4e37', 'rates': 'c2c1e393821db9d8'}
