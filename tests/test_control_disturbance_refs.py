"""CPU tests of the control-dependent disturbance's interface (hjb_set_control_disturbance) and of the reference the GPU tests
compare with (tests/control_disturbance_refs.py): the subclass against DisturbedRef, the prototype in both headers and the ctypes
table, the Python side's checks, the actuator_nodes helper and the axis relabelling.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from control_disturbance_refs import ControlDisturbedRef
from disturbance_refs import DisturbedRef

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib(built):
    import hjbdp
    return hjbdp.load_library()


def _bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["expect", "worst"])
@pytest.mark.parametrize("typing", ["f32", "f64", "tab64"])
def test_a_table_constant_along_the_label_is_the_additive_reference(typing, mode):
    import hjbdp
    from problems import random_problem, random_terminal
    spec = random_problem(4, (6, 5, 4), (3, 2), dtype=np.float64 if typing == "f64" else np.float32, nonuniform=True, index_base=1)
    if typing == "tab64":
        spec = hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, dtype=np.float32, index_base=1, table_dtype=np.float64)
    rng = np.random.default_rng(2)
    off = np.zeros((3, 5))
    off[0], off[2] = 0.4 * rng.standard_normal(5), 0.3 * rng.standard_normal(5)
    w = None if mode == "worst" else rng.uniform(0.1, 1.0, 5)
    Jn = random_terminal(spec, 1)
    a = DisturbedRef(spec, off, w, mode)
    b = ControlDisturbedRef(spec, np.repeat(off[:, :, None], spec.nU, axis=2), w, mode)
    assert a.axes_mask == b.axes_mask == 0b101 and a.coverage() == b.coverage()
    (Ja, la), (Jb, lb) = a.backup(Jn), b.backup(Jn)
    assert np.array_equal(_bits(Ja), _bits(Jb)) and np.array_equal(la, lb)
    lab = rng.integers(1, spec.nU + 1, spec.nS)
    assert np.array_equal(a.evaluate(Jn, lab), b.evaluate(Jn, lab))
    # ... and the [D, W, *m] shape is the same table
    c = ControlDisturbedRef(spec, np.repeat(off[:, :, None], spec.nU, axis=2).reshape((3, 5) + spec.m, order="F"), w, mode)
    assert np.array_equal(c.off, b.off)


def test_a_slice_of_the_table_is_that_labels_node_set():
    """Consequence (iii), in the reference: all labels l0 under the table = all labels l0 under the node set offsets[:, :, l0]; and
    the mask is the union over (w, l)."""
    from problems import random_problem, random_terminal
    spec = random_problem(6, (6, 5, 4), (3, 2), dtype=np.float32, nonuniform=True)
    rng = np.random.default_rng(3)
    off = np.zeros((3, 4, spec.nU))
    off[1] = 0.5 * rng.standard_normal((4, spec.nU))
    off[2, :, 4] = 0.25                                           # axis 2 is offset under one control only
    ref = ControlDisturbedRef(spec, off, None, "expect")
    assert ref.axes_mask == 0b110
    Jn = random_terminal(spec, 2)
    for l0 in range(spec.nU):
        lab = np.full(spec.nS, l0)
        assert np.array_equal(ref.evaluate(Jn, lab), DisturbedRef(spec, off[:, :, l0], None, "expect").evaluate(Jn, lab)), l0


# ---- the C interface -----------------------------------------------------------------------------------------------------------
def test_prototype_agrees_between_the_headers_and_the_ctypes_table(lib):
    from hjbdp import _abi
    from test_abi import _matlab_calllibs, _prototypes
    header = (ROOT / "include" / "hjbdp.h").read_text()
    full = _prototypes(header)
    flat = _prototypes((ROOT / "include" / "hjbdp_matlab.h").read_text())
    name = "hjb_set_control_disturbance"
    assert full[name] == ["void*", "int32_t", "int32_t", "int32_t", "double*", "double*"]
    assert flat[name] == full[name]
    assert _abi.SYMBOLS[name] == (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)])
    assert hasattr(lib, name)
    assert int(re.search(r"#define HJB_CTRL_DIST_MAX_ENTRIES (\d+)", header).group(1)) == _abi.HJB_CTRL_DIST_MAX_ENTRIES == 2 ** 26
    mdir = ROOT / "optimal-control-dynamic-programming_amd" / "matlab"
    calls = {f.name: n for f in sorted(mdir.glob("*.m")) for nm, n in _matlab_calllibs(f.read_text()) if nm == name}
    assert calls == {"hjbdp_set_control_disturbance.m": 6}      # its own shim; hjbdp_solve.m does not call it


def test_a_null_handle_is_invalid_without_a_device(lib):
    from hjbdp import _abi
    off = (C.c_double * 2)(0.0, 0.0)
    assert lib.hjb_set_control_disturbance(None, _abi.HJB_DIST_EXPECT, 1, 1, off, None) == _abi.HJB_E_INVALID
    assert b"null handle" in lib.hjb_last_error(None)
    assert lib.hjb_set_control_disturbance(None, _abi.HJB_DIST_EXPECT, 0, 0, None, None) == _abi.HJB_E_INVALID


# ---- the Python side's checks ------------------------------------------------------------------------------------------------------
def test_check_control_disturbance_states_the_refusals():
    import hjbdp
    from hjbdp.problem import check_control_disturbance
    from problems import random_problem
    D, m = 3, (3, 2)
    off = np.arange(3 * 4 * 6, dtype=np.float64).reshape(3, 4, 6)
    got, w, mode = check_control_disturbance(D, m, off, [0.1, 0.2, 0.3, 0.4], "expect")
    assert np.array_equal(got, off) and np.array_equal(w, [0.1, 0.2, 0.3, 0.4]) and mode == "expect"
    shaped = off.reshape((3, 4, 3, 2), order="F")                 # [D, W, *m]: flattened column-major, label = j0 + 3 j1
    assert np.array_equal(check_control_disturbance(D, m, shaped, None, "worst")[0], off)
    assert shaped[1, 2, 2, 1] == off[1, 2, 2 + 3 * 1]
    bad_inf = off.copy()
    bad_inf[2, 3, 5] = np.inf
    for bad in ((off[:2], None, "expect"),                        # rows != D
                (off[:, :, :5], None, "expect"),                  # nU of another problem
                (off[:, :, 0], None, "expect"),                   # an additive [D, W] set is not a table
                (off.reshape((3, 4, 2, 3), order="F"), None, "expect"),      # control dims in the wrong order
                (off, None, "average"),                           # unknown mode
                (off, [0.25] * 4, "worst"),                       # the worst case takes no weights
                (off, [0.5, 0.5], "expect"),                      # weights != W
                (off, [0.5, 0.5, -0.1, 0.1], "expect"),           # a negative weight
                (off, [0.5, 0.5, np.nan, 0.1], "expect"),         # a weight that is not finite
                (bad_inf, None, "expect"),                        # a non-finite offset
                (np.zeros((3, 129, 6)), None, "worst")):          # more nodes than one disturbance holds
        with pytest.raises(ValueError):
            check_control_disturbance(D, m, *bad)
    # more entries than one table holds - refused by the size alone (no such array is made: a broadcast view)
    big = np.broadcast_to(0.0, (6, 128, 90000))
    with pytest.raises(ValueError, match="entries"):
        check_control_disturbance(6, (300, 300), big, None, "worst")
    # ProblemSpec: a field of its own, exclusive with `disturbance`, refused with a state model
    base = random_problem(5, (4, 3, 5), (3, 2), dtype=np.float32)

    def make(**kw):
        return hjbdp.ProblemSpec(base.knots, base.m, base.next_terms, base.cost_terms, dtype=np.float32, **kw)
    assert make().control_disturbance is None
    spec = make(control_disturbance=(off, None, "worst"))
    assert spec.disturbance is None and np.array_equal(spec.control_disturbance[0], off) and spec.control_disturbance[2] == "worst"
    with pytest.raises(ValueError, match="not both"):
        make(control_disturbance=(off, None, "worst"), disturbance=(off[:, :, 0], None, "worst"))
    sa = hjbdp.Solver_attitude(n_mesh_w=5, n_mesh_q=4)
    sa.U_vector = np.linspace(-0.1, 0.1, 3)
    ms = sa.build_spec_model()
    with pytest.raises(ValueError, match="model"):
        hjbdp.ProblemSpec(ms.knots, ms.m, ms.next_terms, ms.cost_terms, dtype=np.float32, model=ms.model,
                          control_disturbance=(np.zeros((6, 1, ms.nU)), None, "expect"))


def test_permute_state_axes_moves_the_rows_of_the_table():
    import hjbdp
    from problems import random_problem
    base = random_problem(5, (4, 3, 5), (3, 2), dtype=np.float32)
    off = np.arange(3 * 4 * 6, dtype=np.float64).reshape(3, 4, 6)
    spec = hjbdp.ProblemSpec(base.knots, base.m, base.next_terms, base.cost_terms, dtype=np.float32,
                             control_disturbance=(off, [0.1, 0.2, 0.3, 0.4], "expect"))
    order = (2, 0, 1)
    new, _ = hjbdp.permute_state_axes(spec, order)
    assert new.disturbance is None
    assert np.array_equal(new.control_disturbance[0], off[list(order)])       # new axis i carries old axis order[i]'s rows
    assert np.array_equal(new.control_disturbance[1], spec.control_disturbance[1]) and new.control_disturbance[2] == "expect"
    plain = hjbdp.ProblemSpec(base.knots, base.m, base.next_terms, base.cost_terms, dtype=np.float32)
    assert hjbdp.permute_state_axes(plain, order)[0].control_disturbance is None


# ---- the helper --------------------------------------------------------------------------------------------------------------------
def test_actuator_nodes_on_dyadic_inputs_is_exact():
    import hjbdp
    B = np.array([[0.5, -0.25], [2.0, 0.0], [0.0, 1.5]])                     # [D = 3, n_u = 2]
    u = np.array([[-2.0, 0.5], [0.0, 0.0], [1.0, -0.75], [4.0, 0.25]])        # [nU = 4, n_u]
    eps = np.array([-0.25, 0.0, 0.125])
    off, w = hjbdp.actuator_nodes(B, u, eps)
    assert w is None and off.shape == (3, 3, 4) and off.dtype == np.float64
    for wi in range(3):
        for l in range(4):
            assert np.array_equal(off[:, wi, l], B @ (u[l] * eps[wi])), (wi, l)
    assert not off[:, :, 1].any() and not off[:, 1, :].any()                  # no control, or no error: noise-free
    # a relative error per input, weights passed through, an additive base on top
    eps2 = np.array([[0.5, 0.0], [0.0, -0.5]])
    base = np.array([[0.125, -0.125], [0.0, 0.0], [1.0, 2.0]])
    off2, w2 = hjbdp.actuator_nodes(B, u, eps2, weights=[0.25, 0.75], base=base)
    assert w2 == [0.25, 0.75]
    for wi in range(2):
        for l in range(4):
            assert np.array_equal(off2[:, wi, l], B @ (u[l] * eps2[wi]) + base[:, wi]), (wi, l)
    # one input given flat
    o1, _ = hjbdp.actuator_nodes([[0.5], [2.0]], [1.0, -3.0], [0.25])
    assert np.array_equal(o1[:, 0, :], [[0.125, -0.375], [0.5, -1.5]])
    from hjbdp import _abi
    with pytest.raises(ValueError, match="nodes"):
        hjbdp.actuator_nodes(B, u, np.zeros(_abi.HJB_DIST_MAX_NODES + 1))
    with pytest.raises(ValueError):
        hjbdp.actuator_nodes(B, u[:, :1], eps)                                # n_u of B and of the table differ
    with pytest.raises(ValueError):
        hjbdp.actuator_nodes(B, u, eps, base=np.zeros((3, 2)))                # a base of another W
    with pytest.raises(ValueError):
        hjbdp.actuator_nodes(B, u, [np.nan])


def test_dynamic_solver_carries_the_actuator_noise_into_its_spec():
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.dx, ds.du = 9, 5
    assert ds.actuator_noise is None and ds.build_spec().control_disturbance is None
    ds.actuator_noise = ([-0.25, 0.0, 0.25], [0.25, 0.5, 0.25], "expect")
    spec = ds.build_spec()
    off = spec.control_disturbance[0]
    assert spec.disturbance is None and off.shape == (2, 3, 5)
    U = np.asarray(ds._U_mesh, dtype=np.float64)
    assert np.array_equal(off, ds.B[:, :1, None] * (np.array([-0.25, 0.0, 0.25])[None, :, None] * U[None, None, :]))
    ds.disturbance = (np.zeros((2, 1)), None, "expect")
    with pytest.raises(ValueError, match="not both"):
        ds.build_spec()
    ds.disturbance = None
    ds.u_star_idxs = np.ones((9, 9, 3), dtype=np.int32)           # as if run() had been: the flights refuse before any device work
    ds.J_star = np.zeros((9, 9, 4))
    for fly in (lambda: ds.get_noisy_paths(np.zeros((2, 1)), 2), lambda: ds.get_lookahead_paths(np.zeros((2, 1))),
                lambda: ds.get_noisy_cost_statistics(np.zeros((2, 1)), 2)):
        with pytest.raises(RuntimeError, match="control-dependent noise"):
            fly()
