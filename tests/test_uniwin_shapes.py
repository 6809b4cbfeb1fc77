"""The constructed K15 problems of tests/uniwin_shapes.py meet their own conditions (no GPU).

Everything here is a condition on the INPUTS, asserted from plan_of - the numpy restatement of k_uniwin_plan - and from the float64
reference alone: which of the kernel's 23 sweep-shape copies, four level-1 row-pair forms, lone-step rows, window clamps and walk
edges the registered cases reach.  tests/test_gpu_uniwin_shapes.py ties the device plan to the restatement (slow-point counts) and
runs the same cases, so the coverage asserted here is the coverage that ran.  If a case cannot meet a condition the case changes,
not the condition."""
import numpy as np
import pytest

import uniwin_shapes as US

_PLANS = {}


def _plan(name):
    if name not in _PLANS:
        spec = US.CASES[name].build()
        _PLANS[name] = (spec, US.plan_of(spec))
    return _PLANS[name]


def _group(group):
    return [name for name, c in US.CASES.items() if c.group == group]


def _cov(names):
    out = {}
    for name in names:
        for k, v in US.coverage(_plan(name)[1]).items():
            if k != "slow":
                out.setdefault(k, set()).update(v)
    return out


def test_the_kernel_lists_the_23_sweep_shapes_the_formula_gives():
    assert US.kernel_sweep_shapes() == US.ALL_SWEEP_SHAPES and len(US.ALL_SWEEP_SHAPES) == 23


def test_shapes_cases_reach_every_sweep_shape_on_points_of_the_usual_shape():
    names = _group("shapes")
    assert set(names) == {"shapes-11", "shapes-12", "shapes-11-down", "shapes-12-down", "shapes-12-knot"}
    assert _cov(names)["shapes"] == US.kernel_sweep_shapes()
    # ... and each direction on its own: the ascending and the descending cases reach all of their inner count's shapes
    for name in names:
        spec, plan = _plan(name)
        want = {US.sweep_shape(spec.m[2], jc) for jc in range(1, spec.m[2] + 1)}
        assert US.coverage(plan)["shapes"] == want, name
        assert US.coverage(plan)["dirs"] == ({0, -1} if name.endswith("down") else {0, 1}), name


def test_every_shape_is_reached_by_the_removal_of_no_single_case_unnoticed():
    """Taking the 11-control (12-control) cases out loses shapes: the union is not carried by one inner count."""
    for m_in in US.K_IN:
        rest = [n for n in _group("shapes") if _plan(n)[0].m[2] != m_in]
        assert _cov(rest)["shapes"] != US.kernel_sweep_shapes()


def test_knot_case_puts_a_control_on_the_knot_that_opens_the_new_cell_with_weight_zero():
    spec, plan = _plan("shapes-12-knot")
    assert len(set(np.diff(spec.knots[-1]))) == 3                            # spacings 1/2, 1, 2
    ok = ~plan["slow"] & (plan["nchange"] == 1)
    t_at_change = np.take_along_axis(plan["tL"], np.minimum(plan["jc"], spec.m[2] - 1)[..., None], axis=-1)[..., 0]
    assert np.count_nonzero(ok & (t_at_change == 0.0)) >= 20


def test_rows_cases_reach_every_row_pair_form_and_both_lone_rows():
    for name in _group("rows"):
        cov = US.coverage(_plan(name)[1])
        assert cov["pairs"] == {(0, 0), (0, 1), (1, 0), (1, 1)}, name
        assert cov["rowsA"] == {0, 1} and cov["clamps"] >= {"clampA", "clampB"}, name
    assert US.coverage(_plan("rows-11")[1])["lone"] == {0, 1}
    assert _plan("rows-11")[0].m[1] % 2 == 1 and _plan("rows-12")[0].m[1] % 2 == 0


def test_both_directions_and_every_clamp_occur():
    cov = _cov(US.RUN_CASES)
    assert cov["dirs"] == {-1, 0, 1}
    assert cov["clamps"] == {"clampA", "clampB", "clampP"}
    ends = US.coverage(_plan("ends")[1])
    assert ends["dirs"] == {-1, 0, 1} and "clampP" in ends["clamps"]
    # ends: sweeps leave the grid below the first and above the last knot (extrapolation: weights outside [0, 1])
    spec, plan = _plan("ends")
    assert np.any(plan["tL"][:, :, 0, :] < 0) and np.any(plan["tL"][:, :, -1, :] > 1)


def test_counts_cases_hold_the_level_counts_at_their_ends():
    ms = {_plan(n)[0].m[:2] for n in _group("counts") if US.CASES[n].admitted}
    assert {m[1] for m in ms} == {1, 2, 15, 16} and {m[0] for m in ms} == {1, 16}
    assert US.coverage(_plan("counts-1-1")[1])["pairs"] == set()            # one level-1 step: no trip at all
    assert US.coverage(_plan("counts-1-15")[1])["lone"] == {0, 1}


def test_slow_point_counts_are_what_the_construction_says():
    for name, case in US.CASES.items():
        spec, plan = _plan(name)
        assert int(plan["slow"].sum()) == case.slow, name
    for k in (2, 3):
        spec, plan = _plan("slow-mix-%d" % k)
        assert plan["slow"].size == 100 and (plan["slow"].sum() * 50 <= plan["slow"].size) == (k == 2)


def test_queries_cells_and_weights_are_the_same_numbers_in_float32_and_float64():
    for name in US.CASES:
        spec, plan = _plan(name)
        assert plan["exact"] and US.so_exact(spec), name


def test_admission_rule():
    for name, case in US.CASES.items():
        assert US.admitted(_plan(name)[0]) == case.admitted, name
    assert _plan("counts-3-17")[0].m[1] == 17 and not US.CASES["counts-3-17"].admitted


def test_cost_forms():
    orders = {n[5:] for n in _group("cost-forms")}
    assert orders == set(US.COST_ORDERS)
    spec = _plan("cost-l1_per_o0")[0]
    D = spec.D
    assert any(t.dims == (D, D + 1) for t in spec.cost_terms)
    assert _plan("cost-l0_first")[0].cost_terms[0].dims == (D,) and _plan("cost-l1_first")[0].cost_terms[0].dims == (D + 1,)


def test_walk_cases_hold_partial_tiles_on_every_axis_and_a_last_chunk_of_one_state():
    names = _group("walk")
    walks = {n: US.walk_of(_plan(n)[0]) for n in names}
    assert {int(np.prod(_plan(n)[0].n[:-3])) for n in names} >= {128, 257, 300}
    assert {_plan(n)[0].D for n in names} == {4, 5, 6}
    for axis in range(3):
        assert any(w["partial"][axis] for w in walks.values()), axis
    assert all(walks[n]["partial"] == (True, True, True) for n in ("walk-128", "walk-300", "walk-d6"))
    assert walks["walk-257"]["last_chunk"] == 1 and walks["walk-257"]["cpp"] == 2
    assert US.walk_of(_plan("walk-257")[0], block=64)["last_chunk"] == 1
    assert walks["walk-128"]["cpp"] == 1 and walks["walk-128"]["last_chunk"] == 128
    for n in names:
        spec = _plan(n)[0]
        # the tilings the GPU test sets: 1 x 2 x 1, 2 x 2 x 1 and one larger than the axes (clamped)
        assert US.walk_of(spec, uw_tile=8)["log2"] == (0, 1, 0) and US.walk_of(spec, uw_tile=9)["log2"] == (1, 1, 0)
        big = US.walk_of(spec, uw_tile=3 + 8 * 3 + 64 * 3)
        assert big["tiles"][1:] == (1, 1), n                                  # one tile spans the level-1 and the last axis
    # ... and where an axis is shorter than half the tile asked for, uniwin_tiles' clamp takes a smaller one
    assert US.walk_of(_plan("walk-257")[0], uw_tile=3 + 8 * 3 + 64 * 3)["clamped"] == (False, True, False)


def test_the_float64_reference_does_not_depend_on_its_slices():
    """oracle.hjb_oracle.backup_stage in slices of the first axis (chunk_states) returns what the whole grid at once returns, and
    its runner-up is the second smallest total."""
    from oracle import hjb_oracle as O
    spec = US.CASES["counts-1-15"].build()
    term = US.lattice_terminal(spec, 3)
    conv = lambda ts: [O.Term(t.dims, np.asarray(t.data, dtype=np.float64)) for t in ts]
    p = O.Problem(spec.knots, spec.m, [conv(ts) for ts in spec.next_terms], conv(spec.cost_terms), dtype=np.float64)
    Jn = term.astype(np.float64).reshape(spec.n, order="F")
    J, idx = O.backup_stage(p, Jn)
    for chunk in (1, 1000, spec.nS):
        Jc, ic, second = O.backup_stage(p, Jn, chunk_states=chunk, runner_up=True)
        assert np.array_equal(J, Jc) and np.array_equal(idx, ic) and np.all(second >= Jc), chunk
    J64, lab, sec = US.reference64(spec, term)
    assert np.array_equal(J64, J.reshape(-1, order="F")) and np.array_equal(lab, idx.reshape(-1, order="F") + spec.index_base)
    assert np.array_equal(sec, second.reshape(-1, order="F"))


@pytest.mark.parametrize("storage", [None, np.float16])
@pytest.mark.parametrize("name", US.RUN_CASES)
def test_label_gap_condition(name, storage):
    """The float64 reference decides the label (runner-up more than twice the bound above the minimum) at 90 % of a case's states or
    more, and the minimisers spread over the controls."""
    spec, term, J64, lab, bound, decided = US.case_reference(name, storage)
    left_out = 1.0 - decided.mean()
    print(name, storage, "left out of the label comparison: %.2f %%" % (100 * left_out), "labels in use:", len(np.unique(lab)))
    assert left_out <= 0.10, (name, left_out)
    assert np.all(np.isfinite(J64)) and np.all(bound > 0)
    assert len(np.unique(lab)) >= min(8, spec.nU // 2)
