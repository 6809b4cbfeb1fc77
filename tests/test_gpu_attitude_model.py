"""GPU parity tests (-m gpu) of HJB_MODEL_QUAT_EULER321 at its branch points, in every launch form that evaluates it: K3 modes 3 and 6
(csrc/kernels_packed2.h) and K15 mode 8 (csrc/kernels_uniwin.h).  The edge problems of tests/attitude_model_refs.py put >= 20 states
in every branch of canon_atan2f / canon_asinf - swapped arguments, the tan(pi/8) reduction, both reflections, zeros of either sign,
both arguments zero, asin's sqrt branch, pitch argument +-1 and beyond (the clamp) - which the reference's own narrow grid never
reaches.  Bars: J and labels equal to the twin's bit for bit, and J finite everywhere (a pitch knot at +-90 degrees is valid input)."""
import numpy as np
import pytest

import attitude_model_refs as amr

pytestmark = pytest.mark.gpu
FORMS = tuple(amr.FORMS)


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi, c_oracle


_CASES = {}


def _case(env, form, j_storage=None):
    """Of an edge problem: its spec, a random terminal cost, the twin's two-stage sweep and one-stage backup of it, the zero-cost
    spec and the twin's three read-out stages - the input condition asserted, the twin run once per module, nothing written to."""
    key = (form, j_storage)
    if key not in _CASES:
        _, _abi, c_oracle = env
        spec = amr.edge_model_problem(form, j_storage=j_storage)
        amr.assert_classes(spec)
        term = (np.random.default_rng(len(form)).random(spec.nS) * 3).astype(spec.j_dtype)
        ref = c_oracle.sweep(_abi, spec, 2, terminal=term, keep_J=True, keep_idx=True)
        case = {"spec": spec, "term": term, "ref": ref, "mode": amr.FORMS[form]["mode"]}
        if j_storage is None:
            case["one"] = (ref["J_stages"][:, -1], ref["idx_stages"][:, -1])        # the first stage computed: one backup of `term`
            z = amr.edge_model_problem(form, costs=False)
            case["zspec"] = z
            case["readouts"] = [c_oracle.backup_stage(_abi, z, amr.readout_terminal(z, a)) for a in range(3)]
        for a in [term, ref["J_stages"], ref["idx_stages"], ref["J"], ref["idx"]] + [x for p in case.get("readouts", []) for x in p]:
            a.setflags(write=False)
        _CASES[key] = case
    return _CASES[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _assert_same(got, ref, idx_got=None, idx_ref=None, what=""):
    """J (and the labels) equal to the twin's, bit for bit, wherever the twin's J is finite.  Where it is not, neither side is held
    to anything here: every test ends on _assert_finite of BOTH sides, so a non-finite J fails there, by name, and on a tree
    that passes this comparison has covered every state."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    held = np.isfinite(ref)
    bad = np.argwhere(held & (_bits(got) != _bits(ref)))
    assert bad.shape[0] == 0, (what, "J", bad.shape[0], bad[:6].tolist())
    if idx_got is not None:
        bad = np.argwhere(held & (np.asarray(idx_got).astype(np.int64).reshape(ref.shape) != np.asarray(idx_ref).reshape(ref.shape)))
        assert bad.shape[0] == 0, (what, "labels", bad.shape[0], bad[:6].tolist())


def _assert_finite(J, spec, what):
    """`J`: whole grids (one or several stages), the GPU's or the twin's."""
    bad = np.flatnonzero(~np.isfinite(np.asarray(J, dtype=np.float32).reshape(-1, order="F")))
    planes = np.unique(np.unravel_index(bad % spec.nS, spec.n, order="F")[1]) if bad.size else []
    assert bad.size == 0, (what, "non-finite J at %d states, pitch planes %s of %d" % (bad.size, [int(p) for p in planes], spec.n[1]))


def _assert_sweep(out, ref, spec, what):
    """A kept sweep, stage by stage in the order computed (column k holds stage k + 1: the last column comes first): equal to the
    twin, then finite on both sides - a stage is only compared when the cost-to-go it was computed from has been found finite
    (what either side makes of a NaN J_next is outside the contract)."""
    n_st = ref["J_stages"].shape[1]
    assert out["J_stages"].shape == ref["J_stages"].shape and out["idx_stages"].shape == ref["idx_stages"].shape
    for k in range(n_st - 1, -1, -1):
        _assert_same(out["J_stages"][:, k], ref["J_stages"][:, k], out["idx_stages"][:, k], ref["idx_stages"][:, k], (what, "stage", k + 1))
        _assert_finite(ref["J_stages"][:, k], spec, ("the twin's " + what, "stage", k + 1))
        _assert_finite(out["J_stages"][:, k], spec, (what, "stage", k + 1))
    _assert_same(out["J"], ref["J"], out["idx"], ref["idx"], (what, "final"))
    _assert_same(out["J"], out["J_stages"][:, 0], out["idx"], out["idx_stages"][:, 0], (what, "final = stage 1"))


@pytest.mark.parametrize("form", FORMS)
def test_model_edges_bit_equal_and_finite(env, form):
    """Two stages from a random terminal cost, then the three read-out stages (zero costs, J_next = the knot of one angle axis: J is
    the model's next angle up to one lerp), in the launch form asked for: equal to the twin bit for bit and finite everywhere."""
    hjbdp = env[0]
    c = _case(env, form)
    spec, ref = c["spec"], c["ref"]
    with hjbdp.Backup(spec) as bk:
        assert bk.info()["kernel_variant"] == 4 and bk.get_option("packed2_mode") == c["mode"]
        out = bk.solve(2, terminal=c["term"], keep_J=True, keep_idx=True)
    _assert_sweep(out, ref, spec, "sweep")
    assert len(np.unique(out["idx_stages"])) > spec.nU // 2                 # a real argmin: most torque triples win somewhere
    with hjbdp.Backup(c["zspec"]) as bk:
        assert bk.get_option("packed2_mode") == c["mode"]
        for a in range(3):
            Jg, ig = bk.backup_stage(amr.readout_terminal(c["zspec"], a))
            _assert_same(Jg, c["readouts"][a][0], ig, c["readouts"][a][1], ("read-out", a))
            _assert_finite(c["readouts"][a][0], spec, ("the twin's read-out", a))
            _assert_finite(Jg, spec, ("read-out", a))


def test_model_edges_float16_storage(env):
    """The K3 window form once more with float16 cost-to-go storage (tables float32, as always)."""
    hjbdp = env[0]
    c = _case(env, "k3w", "float16")
    spec, ref = c["spec"], c["ref"]
    assert spec.j_dtype == np.float16 and all(np.asarray(t).dtype == np.float32 for t in spec.model["tables"])
    with hjbdp.Backup(spec) as bk:
        assert bk.get_option("packed2_mode") == c["mode"]
        out = bk.solve(2, terminal=c["term"], keep_J=True, keep_idx=True)
    _assert_sweep(out, ref, spec, "float16 sweep")


def test_model_edges_slab_with_halos(env):
    """K15's form once more as a slab: planes 1 .. 2 of w3 with one halo plane each way, against the whole-grid twin."""
    hjbdp = env[0]
    c = _case(env, "k15")
    spec, term = c["spec"], c["term"]
    Jw, iw = c["one"]
    nl = spec.n[-1]
    inner = spec.nS // nl
    b, e, lo, hi = 1, 3, 1, 1
    T2 = term.reshape(inner, nl, order="F")
    with hjbdp.Backup(spec, slab=(b, e, lo, hi)) as bk:
        assert bk.get_option("packed2_mode") == c["mode"]
        Jo, io = bk.backup_stage(np.asfortranarray(T2[:, b - lo:e + hi]).reshape(-1, order="F"))
    Jo = Jo.reshape(inner, -1, order="F")[:, lo:lo + e - b]
    _assert_same(Jo, Jw.reshape(inner, nl, order="F")[:, b:e], io.reshape(inner, e - b, order="F"), iw.reshape(inner, nl, order="F")[:, b:e], "the slab")
    _assert_finite(Jw, spec, "the twin's stage")
    assert np.all(np.isfinite(Jo)), ("non-finite J in the slab", np.count_nonzero(~np.isfinite(Jo)))
