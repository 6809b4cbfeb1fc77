"""GPU tests (-m gpu) of K10 (k_backup_colsweep, variant 7) on the constructed problems of tests/colsweep_shapes.py, whose coverage
tests/test_colsweep_shapes.py asserts without a device: every single-launch instantiation, every entry of the counted-wait tables,
padded groups in either half, every plan-builder path, the one-load form's odd-state placements, parts and re-priming, XCD shares of
zero columns, the cost record's shapes and the label widths.

Per case:
  * the device's decisions equal the numpy restatement: the automatic variant, cs_group_axis, cs_groups, cs_rows, cs_dpp,
    cs_cost_form, cs_split (automatic and forced, the forced one reading back the value in effect) and the grid of info();
  * every stage of a 3-stage sweep equals oracle/c_oracle.sweep bit for bit (J by its bits, labels) - under the defaults, under
    cs_dpp 0, under every cs_split the case registers, under both cs_xcd_axis values and the case's cs_xcd_mod values, with variant 5
    forced on the same handle, and once more under the defaults, where the handle must give its first bits back;
  * one stage from the lattice terminal equals oracle/hjb_oracle.py in float64 EXACTLY (binary16 storage: that value rounded once) -
    no tolerance: colsweep_shapes.one_stage_exact proves the stage exact in float32.
Then: the late-bit cases' tie twins (every control in turn the first of a tie), three slabs with halos, one batched run of two
NG = 6 problems, the refusals - and, last, the set of instantiations actually launched, from the readbacks: all 144."""
import numpy as np
import pytest

import colsweep_shapes as CS

pytestmark = pytest.mark.gpu

_LAUNCHED = set()


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi, c_oracle


_TWIN = {}


def _twin(env, name):
    """The C twin's 3-stage sweep of a case from its lattice terminal, once per module."""
    if name not in _TWIN:
        _, _abi, c_oracle = env
        spec, term = CS.case_reference(name)[:2]
        _TWIN[name] = c_oracle.sweep(_abi, spec, 3, terminal=term, keep_J=True, keep_idx=True)
    return _TWIN[name]


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


def _record(bk, out):
    """What the launch that produced `out` was, from the handle's readbacks and the result's own type."""
    assert bk.info()["kernel_variant"] == 7
    _LAUNCHED.add(("f16" if out["J"].dtype == np.float16 else "f32", bk.get_option("cs_group_axis"), bk.get_option("cs_groups"),
                   bk.get_option("cs_cost_form"), bool(bk.get_option("cs_dpp"))))


@pytest.mark.parametrize("name", CS.RUN_CASES)
def test_case_decisions_and_every_stage_bit_exact(env, name):
    hjbdp = env[0]
    case = CS.CASES[name]
    spec, term, J64, lab64, exact = CS.case_reference(name)
    gax, plans, _ = CS.pick_of(spec)
    plan, dpp, form = plans[gax], CS.dpp_of(spec)["ok"], CS.cost_form_of(spec)
    n1 = spec.n[1]
    ref = _twin(env, name)
    solve = lambda bk: bk.solve(3, terminal=term, keep_J=True, keep_idx=True)

    def decided(bk, on, cs_split=0, axis=0):
        S = CS.split_of(spec, on, cs_split)[0]
        assert bk.get_option("cs_dpp") == int(on) and bk.get_option("cs_split") == S, (name, on, cs_split)
        assert bk.info()["grid"] == CS.grid_of(spec, gax, on, S, axis), (name, on, cs_split, axis)

    with hjbdp.Backup(spec) as bk:
        assert bk.info()["kernel_variant"] == CS.auto_variant_of(spec)
        bk.set_option("variant", 7)
        assert bk.info()["kernel_variant"] == 7 and bk.info()["idx_bytes"] == spec.idx_np_dtype.itemsize
        assert bk.get_option("cs_group_axis") == gax and bk.get_option("cs_groups") == plan["ng_max"]
        assert bk.get_option("cs_rows") == plan["mid_rows"] and bk.get_option("cs_cost_form") == form
        decided(bk, dpp)
        first = solve(bk)
        _same(first, ref, (name, "defaults"))
        _record(bk, first)
        # one stage against float64, independent of the C twin: exact
        assert exact, name
        one = bk.solve(1, terminal=term)
        if spec.j_dtype == np.float16:
            assert np.array_equal(_bits(one["J"]), _bits(J64.astype(np.float16))), (name, "float64 rounded once to binary16")
        else:
            assert np.array_equal(one["J"].astype(np.float64), J64), (name, "float64")
        assert np.array_equal(one["idx"].astype(np.int64), lab64), (name, "labels against float64")
        # the two-loads form on the same handle
        bk.set_option("cs_dpp", 0)
        decided(bk, False)
        out = solve(bk)
        _same(out, ref, (name, "cs_dpp 0"))
        _record(bk, out)
        bk.set_option("cs_dpp", 1)
        for s in case.splits:
            bk.set_option("cs_split", s)
            assert bk.get_option("cs_split") == min(s, n1)
            decided(bk, dpp, s)
            _same(solve(bk), ref, (name, "cs_split", s))
        bk.set_option("cs_split", 0)
        decided(bk, dpp)
        for axis, mods in ((0, case.xcd_mods), (1, (0,))):
            bk.set_option("cs_xcd_axis", axis)
            for mod in mods:
                bk.set_option("cs_xcd_mod", mod)
                decided(bk, dpp, 0, axis)
                _same(solve(bk), ref, (name, "cs_xcd_axis", axis, "cs_xcd_mod", mod))
        bk.set_option("cs_xcd_axis", 0)
        bk.set_option("cs_xcd_mod", 0)
        bk.set_option("variant", 5)                    # a second device witness on the same handle
        assert bk.info()["kernel_variant"] == 5 and bk.get_option("cs_cost_form") == -1
        _same(solve(bk), ref, (name, "variant 5"))
        bk.set_option("variant", 7)
        decided(bk, dpp)
        again = solve(bk)
        assert np.array_equal(_bits(again["J_stages"]), _bits(first["J_stages"])), (name, "defaults again", "J")
        assert np.array_equal(again["idx_stages"], first["idx_stages"]), (name, "defaults again", "labels")


@pytest.mark.parametrize("name", CS.LATE_CASES)
def test_ties_through_the_late_bits(env, name):
    """Constant control cost from control w on, one more below it, a zero terminal: w and every later control tie at every state, and
    w - whichever slot of whichever pair the plan gave it, visited before or after the others - must be returned.  w = 0 is the
    all-tie twin: every label is index_base."""
    hjbdp = env[0]
    base = CS.CASES[name].build()
    gax, plans, _ = CS.pick_of(base)
    late = set()
    for col in plans[gax]["cols"].values():
        for G in col["groups"]:
            for p in (0, 1):
                late |= {(p, u) for s, u in enumerate(G["slots"][p]) if G["late"] & (1 << (3 * p + s))}
    assert {p for p, _ in late}, (name, "no late slot")
    for w in range(base.nU):
        spec = CS.tie_twin(base, w)
        with hjbdp.Backup(spec, variant=7) as bk:
            for on in (1, 0):
                bk.set_option("cs_dpp", on)
                assert bk.info()["kernel_variant"] == 7 and bk.get_option("cs_dpp") == on
                out = bk.solve(1)
                bad = np.flatnonzero(out["idx"].astype(np.int64) != w + spec.index_base)
                assert bad.size == 0, (name, "winner", w, "cs_dpp", on, bad.size, bad[:8].tolist(), out["idx"][bad[:8]].tolist())
                assert np.array_equal(out["J"].astype(np.float64), np.zeros(spec.nS)), (name, w, on)
                _record(bk, out)


SLABS = [
    # case, slab (begin, end) of the last axis, the group axis the slab's plan must pick, what is therefore sharded
    ("nu16", (5, 9), 3, "the group axis"),                # (planes 3 .. 6 of this case would be grouped by axis 2: five groups against six)
    ("natural-g2", (2, 4), 2, "the window axis"),
    ("natural-g2", (2, 3), 2, "the window axis, three planes present"),
]


@pytest.mark.parametrize("name,owned,want_gax,what", SLABS)
def test_slab_with_halos(env, name, owned, want_gax, what):
    """The last axis sharded, the J buffers beginning at plane begin - halo_lo > 0.  Grouped by axis 3, the group-axis CELLS are taken
    relative to that plane and the groups' row offsets count from it; grouped by axis 2, the window knots present are the slab's."""
    hjbdp, _abi, c_oracle = env
    spec, term = CS.case_reference(name)[:2]
    with hjbdp.Backup(spec, variant=7) as bk:
        need = bk.info()
    b, e = owned
    hl, hh = min(need["halo_needed_lo"], b), min(need["halo_needed_hi"], spec.n[3] - e)
    planes = (b, e, hl, hh)
    if "three planes" in what:
        assert (e - b) + hl + hh == 3
    gax, plans, _ = CS.pick_of(spec, planes)
    assert gax == want_gax and b - hl > 0, (name, what, gax, planes)
    inner = spec.nS // spec.n[3]
    sub = np.asfortranarray(term.reshape(inner, -1, order="F")[:, b - hl:e + hh]).reshape(-1, order="F")
    Jr, ir = c_oracle.backup_stage(_abi, spec, sub, slab=planes)
    with hjbdp.Backup(spec, slab=planes, variant=7) as bk:
        assert bk.info()["kernel_variant"] == 7
        assert bk.get_option("cs_group_axis") == gax and bk.get_option("cs_groups") == plans[gax]["ng_max"]
        assert bk.get_option("cs_rows") == plans[gax]["mid_rows"]
        assert not any(col["halo"] for col in plans[gax]["cols"].values())
        for on in (1, 0):
            bk.set_option("cs_dpp", on)
            Jg, ig = bk.backup_stage(sub)
            assert np.array_equal(_bits(Jg), _bits(Jr)) and np.array_equal(ig, ir), (name, what, on)


def test_two_ng6_problems_in_one_batched_launch(env):
    """The batch entry runs the same body: two problems of six groups, group axis 3, float32 cost terms, through solve_batch - each
    must equal its own hjb_solve, and that the C twin."""
    import ctypes as C
    hjbdp, _abi, c_oracle = env
    from hjbdp.core import _sweep_args, _sweep_result
    names = ["g3-ng6-f32-c1", "plan-paths-g3"]
    specs = [CS.case_reference(n)[0] for n in names]
    terms = [CS.case_reference(n)[1] for n in names]
    for s in specs:
        assert CS.instantiation_of(s) == ("f32", 3, 6, 1, True)
    lib = hjbdp.load_library()
    bks = [hjbdp.Backup(s, variant=7) for s in specs]
    try:
        own = [bk.solve(3, terminal=t) for bk, t in zip(bks, terms)]
        built = [_sweep_args(s, 3, terminal=t) for s, t in zip(specs, terms)]       # alive until hjb_solve_batch has returned
        ress = [_abi.hjb_result() for _ in names]
        hs = (C.c_void_p * 2)(*[bk._h for bk in bks])
        optp = (C.POINTER(_abi.hjb_solve_opts) * 2)(*[C.pointer(o) for o, _, _ in built])
        resp = (C.POINTER(_abi.hjb_result) * 2)(*[C.pointer(r) for r in ress])
        st = lib.hjb_solve_batch(2, hs, optp, resp)
        assert st == _abi.HJB_OK, st
        for name, (_, out, _), r, mine in zip(names, built, ress, own):
            got = _sweep_result(out, r)
            ref = _twin(env, name)
            assert np.array_equal(_bits(got["J"]), _bits(mine["J"])) and np.array_equal(got["idx"], mine["idx"]), (name, "batch against its own solve")
            assert np.array_equal(_bits(got["J"]), _bits(ref["J"])) and np.array_equal(got["idx"], ref["idx"]), (name, "batch against the C twin")
    finally:
        for bk in bks:
            bk.close()


@pytest.mark.parametrize("name", CS.REFUSED_CASES)
def test_refused_where_variant_7_does_not_serve(env, name):
    hjbdp, _abi, c_oracle = env
    spec = CS.CASES[name].build()
    assert not CS.admitted(spec)
    shape_or_plan = CS.shape_admitted(spec) is not None or CS.pick_of(spec)[0] is None
    term = CS.lattice_terminal(spec, 3)
    ref = c_oracle.sweep(_abi, spec, 1, terminal=term)
    with hjbdp.Backup(spec) as bk:
        assert bk.info()["kernel_variant"] == CS.auto_variant_of(spec) == 5
        with pytest.raises(hjbdp.HjbError) as ei:
            bk.set_option("variant", 7)
        assert ei.value.status == _abi.HJB_E_UNSUPPORTED
        assert ("variant 7 (column sweep) needs" if shape_or_plan else "float64 cost terms") in str(ei.value), str(ei.value)
        assert bk.info()["kernel_variant"] == 5 and bk.get_option("cs_groups") == 0 and bk.get_option("cs_cost_form") == -1
        out = bk.solve(1, terminal=term)                 # the handle still serves, on the table kernel
        assert np.array_equal(_bits(out["J"]), _bits(ref["J"])) and np.array_equal(out["idx"], ref["idx"])


def test_every_instantiation_was_launched():
    """Runs after the parametrised cases.  From the readbacks of the launches made above, not from the registry: all 144."""
    missing = sorted(CS.ALL_INSTANTIATIONS - _LAUNCHED)
    print("%d of %d instantiations launched" % (len(CS.ALL_INSTANTIATIONS & _LAUNCHED), len(CS.ALL_INSTANTIATIONS)))
    assert not missing, (len(missing), missing[:12])
