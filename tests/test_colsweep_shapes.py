"""No device: the constructed problems of tests/colsweep_shapes.py reach every condition K10 (k_backup_colsweep, variant 7) branches on,
each asserted by name - its 144 single-launch instantiations, every entry of the two counted-wait tables, padded groups in either
half of the group sequence, every path of the plan builder, of the one-load test, of the split and XCD rules and of the cost record -
and the restatement of the host plan is self-consistent.  tests/test_gpu_colsweep_shapes.py runs the same cases on the device."""
import numpy as np
import pytest

import colsweep_shapes as CS


@pytest.fixture(scope="module")
def reached():
    """name -> (spec, coverage), every registered case built once."""
    out = {}
    for name, case in CS.CASES.items():
        spec = case.build()
        out[name] = (spec, CS.coverage(spec, case.splits, case.xcd_mods))
    return out


def _need(reached, names):
    """Every named condition is REGISTERED by a case - and test_case_reaches_what_it_is_registered_for holds every case to what it
    registers - so none is reached by accident alone."""
    missing = []
    for c in sorted(names):
        by = [n for n, case in CS.CASES.items() if c in case.reaches]
        print("%-28s %s" % (c, ", ".join(by)[:150]))
        if not by or not all(c in reached[n][1] for n in by):
            missing.append(c)
    assert not missing, missing


@pytest.mark.parametrize("name", list(CS.CASES))
def test_case_reaches_what_it_is_registered_for(reached, name):
    """Case by case, not only in the union: a condition that moves to another case, or stays only where it is incidental, fails here."""
    case = CS.CASES[name]
    assert case.reaches, name
    missing = sorted(set(case.reaches) - reached[name][1])
    assert not missing, (name, missing)


def test_every_registered_instantiation_is_one_of_the_144():
    registered = {c for case in CS.CASES.values() for c in case.reaches if c.startswith("inst:")}
    want = {"inst:%s:g%d:ng%d:c%d:dpp%d" % (s, g, ng, f, int(d)) for (s, g, ng, f, d) in CS.ALL_INSTANTIATIONS}
    assert registered == want, sorted(want ^ registered)[:8]


def test_every_instantiation_is_reached(reached):
    """(storage, GAX, NG, cost form, DPP): 2 x 2 x 6 x 3 x 2; cs_dpp 0 forced on an admitted case is that case's DPP = false twin."""
    got = set()
    for name in CS.RUN_CASES:
        spec = reached[name][0]
        for cs_dpp in (0, 1):
            got.add(CS.instantiation_of(spec, cs_dpp))
    assert len(CS.ALL_INSTANTIATIONS) == 144
    assert got == CS.ALL_INSTANTIATIONS, sorted(CS.ALL_INSTANTIATIONS - got)
    for gax in (2, 3):                   # the matrix cases are what their names say
        for ng in range(1, 7):
            for storage in ("f32", "f16"):
                for form in (0, 1, 2):
                    assert CS.instantiation_of(reached["g%d-ng%d-%s-c%d" % (gax, ng, storage, form)][0]) == (storage, gax, ng, form, True)


def test_host_refuses_the_one_load_form_per_axis_and_storage(reached):
    _need(reached, ["dpp_refused:g%d:%s" % (g, s) for g in (2, 3) for s in ("f32", "f16")])


def test_every_counted_wait_entry_is_reached(reached):
    _need(reached, ["nH1:%d" % k for k in range(10)] + ["nH0:%d" % k for k in range(2, 10)])


def test_padded_groups_in_either_half(reached):
    """NG = 2 has one group in its first half - group 0, which every column has: its padded group can only be in the second."""
    _need(reached, ["ng_full:%d" % k for k in range(2, 7)] + ["pad_second:%d" % k for k in range(2, 7)] + ["pad_first:%d" % k for k in range(3, 7)])


def test_used_bits_and_member_counts(reached):
    _need(reached, ["used:p0_only", "used:p1_only", "used:both", "members:1", "members:2", "members:3"])


def test_plan_builder_paths(reached):
    _need(reached, ["plan:split_full_pair", "plan:two_windows", "plan:wmin_clamped", "plan:nwk3", "plan:late_p0", "plan:late_p1", "plan:order_differs"])
    for name in CS.LATE_CASES:
        assert {"plan:late_p0", "plan:late_p1"} & reached[name][1], name


def test_control_counts(reached):
    _need(reached, ["nU:1", "nU:16", "nU:17"])
    assert "refused:controls" in reached["nu17"][1] and not CS.admitted(reached["nu17"][0])


def test_pick_rule(reached):
    _need(reached, ["pick:3_refused", "pick:2_refused", "pick:rows_decide", "pick:both_refused"])
    assert not CS.admitted(reached["pick-none"][0])


def test_one_load_form_conditions(reached):
    _need(reached, ["dpp:odd_lane0", "dpp:odd_lane59", "dpp:odd_mid", "dpp:odd_last_partial", "dpp:kb_flip", "dpp:two_state_tie",
                    "dpp:last_chunk_one", "dpp:n0_60", "dpp:kb=-2", "dpp:kb=-1", "dpp:kb=0", "dpp:kb=1", "dpp:kb_differs"])


def test_steps_and_parts(reached):
    _need(reached, ["step:repeat_mid", "step:repeat_last", "step:jump2", "step:part_on_repeat", "step:part_on_jump", "step:one_step_parts",
                    "step:uneven_parts", "step:split_above_n1"])


def test_xcd_shares(reached):
    _need(reached, ["xcd:%d:%d" % (a, k) for a in (0, 1) for k in (3, 7, 8, 9)] + ["xcd_mod:1", "xcd_mod:3", "xcd_mod:-1"])
    spec = reached["g3-ng1-f32-c1"][0]           # three indices on the split axis: five XCDs have no column
    assert CS.xcd_of(spec, 3)[0] == [0, 0, 1, 0, 0, 1, 0, 1]
    assert sorted(CS.xcd_of(spec, 3, mod=3)[1]) == [0, 1, 2]


def test_cost_shapes(reached):
    _need(reached, ["cost:form0", "cost:form1", "cost:form2", "cost:npre_col0", "cost:npre_col1", "cost:npre_col3", "cost:npre_col4", "cost:has_su0",
                    "cost:has_su1", "cost:step_nonuniform", "cost:two_step_terms", "cost:ncu0", "cost:ncu2", "cost:ncu%d" % CS.K_MAXCU, "cost:npre0",
                    "cost:c64_npre_col4"])
    assert "refused:control terms" in reached["cost-cu5"][1] and "refused:cost64 shape" in reached["cost-c64-general"][1]


def test_label_widths_and_bases(reached):
    _need(reached, ["labels:%d:%d" % (w, b) for w in (1, 2, 4) for b in (0, 1)])


def test_refused_cases_are_refused_and_the_others_admitted(reached):
    for name, (spec, _) in reached.items():
        assert CS.admitted(spec) == CS.CASES[name].admitted, name
        assert spec.nS <= 100000, (name, spec.nS)


def test_plan_restatement_is_self_consistent(reached):
    """Every control in exactly one slot, at most three per pair, every window inside the knots present, the control's window cell
    the one its pair says, at most K_GMAX groups, and the handle's totals the sums over the columns."""
    for name in CS.RUN_CASES:
        spec = reached[name][0]
        gax, plans, _ = CS.pick_of(spec)
        plan = plans[gax]
        wax = 5 - gax
        cw, _ = CS.axis_cells(spec, wax)
        cgc, _ = CS.axis_cells(spec, gax)
        cw = np.broadcast_to(cw, (1, 1, spec.n[2], spec.n[3], spec.nU))[0, 0]
        cgc = np.broadcast_to(cgc, (1, 1, spec.n[2], spec.n[3], spec.nU))[0, 0]
        rows = 0
        for (i2, i3), col in plan["cols"].items():
            seen = []
            assert 1 <= col["ng"] <= CS.K_GMAX and col["ng"] <= plan["ng_max"]
            for G in col["groups"]:
                assert 0 <= G["wmin"] and G["wmin"] + 2 <= spec.n[wax] - 1, (name, i2, i3, G)
                assert 0 <= G["cell"] <= spec.n[gax] - 2
                for p in (0, 1):
                    m = len(G["slots"][p])
                    assert m <= CS.K_PS and (G["used"] >> (3 * p)) & 7 == (1 << m) - 1          # a prefix of the pair
                    assert list(G["slots"][p]) == sorted(G["slots"][p])
                    for u in G["slots"][p]:
                        assert cw[i2, i3, u] == G["wmin"] + p and cgc[i2, i3, u] == G["cell"], (name, i2, i3, u)
                        seen.append(u)
                assert G["late"] & ~G["used"] == 0
            assert sorted(seen) == list(range(spec.nU)), (name, i2, i3)
            rows += 6 * col["ng"]
        assert rows == plan["rows_total"] and plan["ng_max"] == max(c["ng"] for c in plan["cols"].values())


def test_cells_and_weights_equal_in_float32_and_float64(reached):
    for name, (spec, _) in reached.items():
        assert CS.tables_exact(spec), name


def test_one_stage_is_exact_for_every_case():
    """The argument of colsweep_shapes.one_stage_exact holds for every case that runs (no float64 reference is computed here)."""
    for name in CS.RUN_CASES:
        spec = CS.CASES[name].build()
        assert CS.one_stage_exact(spec, CS.lattice_terminal(spec, 3)), name


def test_split_rule_values():
    """colsweep_split restated, at values worked out by hand from its three loops."""
    spec = CS.CASES["g3-ng1-f32-c1"].build()          # 8 x 9 x 7 x 3: 21 waves, nine steps
    assert CS.split_of(spec, True, 0)[0] == 4         # n1 / 2 = 4 parts fit three quarters of the wave slots
    assert CS.split_of(spec, True, 12) == (9, [(k, k + 1) for k in range(9)])
    assert CS.split_of(spec, True, 2)[1] == [(0, 4), (4, 9)]
