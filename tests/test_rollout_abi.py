"""CPU tests of hjb_rollout_* (include/hjbdp.h): every refusal of hjb_rollout_create is decided before any device work and
named in hjb_rollout_last_error(NULL); valid arguments without a GPU are HJB_E_DEVICE; the prototypes agree in both headers;
and the numpy restatement the GPU tests hold the kernel to (tests/rollout_refs.py) agrees with the host rollout."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
ROLLOUT_FNS = ("hjb_rollout_create", "hjb_rollout_set_model", "hjb_rollout_set_option", "hjb_rollout_run", "hjb_rollout_destroy",
               "hjb_rollout_last_error")


@pytest.fixture(scope="module")
def lib(built):
    import hjbdp
    return hjbdp.load_library()


def _create(lib, knots, labels, u_table, idx_dtype, index_base=1, n_planes=None, n_labels=None, n_u=None, D=None):
    from hjbdp import _abi
    ks = [np.asarray(k, dtype=np.float64) for k in knots]
    kcat = np.ascontiguousarray(np.concatenate(ks))
    n = (C.c_int32 * 8)(*[len(k) for k in ks])
    nS = int(np.prod([len(k) for k in ks]))
    lab = np.ascontiguousarray(labels)
    ut = np.ascontiguousarray(np.asarray(u_table, dtype=np.float64))
    n_planes = lab.size // nS if n_planes is None else n_planes
    n_labels = ut.shape[0] if n_labels is None else n_labels
    n_u = (ut.shape[1] if ut.ndim == 2 else 1) if n_u is None else n_u
    out = C.c_void_p()
    st = lib.hjb_rollout_create(0, len(ks) if D is None else D, n, kcat.ctypes.data_as(C.POINTER(C.c_double)), idx_dtype,
                                index_base, n_planes, lab.ctypes.data, n_labels, n_u,
                                ut.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out))
    if st == _abi.HJB_OK:
        lib.hjb_rollout_destroy(out)
    return st, lib.hjb_rollout_last_error(None).decode()


def _no_device_status():
    import hjbdp
    from hjbdp import _abi
    return _abi.HJB_OK if hjbdp.device_count() > 0 else _abi.HJB_E_DEVICE


def test_rollout_prototypes_are_identical_in_both_headers(lib):
    from test_abi import _prototypes
    full = _prototypes((ROOT / "include" / "hjbdp.h").read_text())
    flat = _prototypes((ROOT / "include" / "hjbdp_matlab.h").read_text())
    for name in ROLLOUT_FNS:
        assert name in full and name in flat, name
        assert full[name] == flat[name], (name, full[name], flat[name])
        assert hasattr(lib, name), name
    # the handle is spelled void * in both headers (no new typedef for test_abi's normaliser to miss)
    assert full["hjb_rollout_run"][0] == "void*" and full["hjb_rollout_create"][-1] == "void**"
    assert "#define HJB_ROLLOUT_MAX_U 4" in (ROOT / "include" / "hjbdp.h").read_text()


def test_rollout_create_refusals_without_a_device(lib):
    from hjbdp import _abi
    k = np.linspace(-1.0, 1.0, 4)
    lab = np.ones((16, 3), dtype=np.int32, order="F")
    ut = np.array([[0.5], [-0.5]])
    U8, U16, I32 = _abi.HJB_IDX_U8, _abi.HJB_IDX_U16, _abi.HJB_IDX_I32
    assert _create(lib, [k, k], lab, ut, I32) == (_no_device_status(), _create(lib, [k, k], lab, ut, I32)[1])
    # D outside 1..6, n_u outside 1..4: unsupported
    st, msg = _create(lib, [k, k], lab, ut, I32, D=7)
    assert st == _abi.HJB_E_UNSUPPORTED and "D=7" in msg
    st, msg = _create(lib, [k, k], lab, ut, I32, D=0)
    assert st == _abi.HJB_E_UNSUPPORTED
    for nu in (0, 5):
        st, msg = _create(lib, [k, k], lab, np.zeros((2, 5)), I32, n_u=nu)
        assert st == _abi.HJB_E_UNSUPPORTED and "n_u=%d" % nu in msg, (nu, msg)
    # invalid arguments
    for idt in (_abi.HJB_IDX_AUTO, 7, -1):
        st, msg = _create(lib, [k, k], lab, ut, idt)
        assert st == _abi.HJB_E_INVALID and "idx_dtype" in msg
    for base in (2, -1):
        st, msg = _create(lib, [k, k], lab, ut, I32, index_base=base)
        assert st == _abi.HJB_E_INVALID and "index_base" in msg
    st, msg = _create(lib, [k, np.array([0.5])], np.ones(4, np.int32), ut, I32)
    assert st == _abi.HJB_E_INVALID and "knots" in msg
    for bad in (np.array([0.0, 1.0, 1.0, 2.0]), np.array([0.0, 2.0, 1.0, 3.0]), np.array([0.0, np.nan, 1.0, 2.0])):
        st, msg = _create(lib, [k, bad], lab, ut, I32)
        assert st == _abi.HJB_E_INVALID and "axis 1" in msg, msg
    st, msg = _create(lib, [k, k], lab, ut, I32, n_planes=0)
    assert st == _abi.HJB_E_INVALID and "n_planes" in msg
    for v in (np.nan, np.inf):
        st, msg = _create(lib, [k, k], lab, np.array([[0.5], [v]]), I32)
        assert st == _abi.HJB_E_INVALID and "u_table element 1" in msg
    # size overflow: 2^21 knots on each of two axes is more states than the library accepts, refused before any label is read
    big = np.arange(1 << 21, dtype=np.float64)
    st, msg = _create(lib, [big, big], lab, ut, I32, n_planes=1)
    assert st == _abi.HJB_E_INVALID and "overflow" in msg
    st, msg = _create(lib, [big, big[:1 << 18]], lab, ut, I32, n_planes=1 << 20)
    assert st == _abi.HJB_E_INVALID and "overflow" in msg


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
@pytest.mark.parametrize("base", [0, 1])
def test_rollout_create_refuses_a_label_outside_the_table(lib, dtype, base):
    from hjbdp import _abi
    idt = {np.uint8: _abi.HJB_IDX_U8, np.uint16: _abi.HJB_IDX_U16, np.int32: _abi.HJB_IDX_I32}[dtype]
    k = np.linspace(0.0, 1.0, 3)
    n_labels = 5
    lab = np.full(9 * 4, base, dtype=dtype)
    ut = np.arange(n_labels, dtype=np.float64).reshape(-1, 1)
    assert _create(lib, [k, k], lab, ut, idt, index_base=base)[0] == _no_device_status()
    hi = lab.copy()
    hi[9 * 2 + 7] = base + n_labels                       # one past the table: state 7 of plane 2
    st, msg = _create(lib, [k, k], hi, ut, idt, index_base=base)
    assert st == _abi.HJB_E_INVALID, msg
    assert "flat position 25" in msg and "plane 2" in msg and "[%d, %d)" % (base, base + n_labels) in msg, msg
    if base == 1:
        lo = lab.copy()
        lo[31] = 0                                         # below a 1-based table
        st, msg = _create(lib, [k, k], lo, ut, idt, index_base=base)
        assert st == _abi.HJB_E_INVALID and "flat position 31" in msg, msg
    if dtype == np.int32:
        neg = lab.copy()
        neg[3] = -1
        st, msg = _create(lib, [k, k], neg, ut, idt, index_base=base)
        assert st == _abi.HJB_E_INVALID and "flat position 3" in msg and "label -1" in msg, msg


def test_rollout_calls_on_a_null_object_are_statuses(lib):
    from hjbdp import _abi
    A = np.eye(2)
    p = A.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.hjb_rollout_set_model(None, p, p, None, None, None) == _abi.HJB_E_INVALID
    assert lib.hjb_rollout_set_option(None, b"chunk", 64) == _abi.HJB_E_INVALID
    assert lib.hjb_rollout_set_option(None, b"lds", 0) == _abi.HJB_E_INVALID
    X = np.zeros(2)
    xp = X.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.hjb_rollout_run(None, 1, 0, None, 1, xp, xp, None, None, None, None) == _abi.HJB_E_INVALID
    assert b"null" in lib.hjb_rollout_last_error(None)
    assert lib.hjb_rollout_destroy(None) == _abi.HJB_OK


def test_python_rollout_without_a_device_is_a_loud_failure(lib):
    import hjbdp
    from hjbdp import _abi
    if hjbdp.device_count() > 0:
        pytest.skip("a GPU is visible")
    k = np.linspace(0.0, 1.0, 3)
    with pytest.raises(hjbdp.HjbError) as ei:
        hjbdp.Rollout([k, k], np.ones((9, 2), np.uint8), [[1.0]])
    assert ei.value.status == _abi.HJB_E_DEVICE
    with pytest.raises(hjbdp.HjbError) as ei:
        hjbdp.Rollout([k, k], np.full((9, 2), 3, np.uint8), [[1.0], [2.0]])
    assert ei.value.status == _abi.HJB_E_INVALID and "flat position 0" in str(ei.value)


def test_reference_restatement_follows_the_host_rollout(built):
    """rollout_refs on the Kirk model agrees with Dynamic_Solver.get_optimal_path's arithmetic (a host interpolation of its own,
    numpy's A @ x) to rounding, on a policy table built here without a GPU."""
    import rollout_refs
    from hjbdp.matlab_compat import interp_linear_point
    rng = np.random.default_rng(5)
    k = np.linspace(-2.5, 3.0, 35)
    U_mesh = np.linspace(-40.0, 10.0, 100)
    lab = rng.integers(1, 101, size=(35 * 35, 6)).astype(np.int32)
    A = np.array([[0.9974, 0.0539], [-0.1078, 1.1591]])
    B = np.array([[0.0013], [0.0539]])
    X0 = np.array([[2.0, -1.0], [1.0, 0.5]])
    planes = [0, 1, 2, 3, 4, 5, 5]
    Xf, cost, Xp, Up = rollout_refs.rollout([k, k], lab, U_mesh, 1, A, B, X0, planes, "linear", q=[0.25, 0.05], r=[0.05])
    for t in range(2):
        x = X0[:, t].copy()
        J = 0.0
        for s, p in enumerate(planes):
            u = interp_linear_point([k, k], U_mesh[lab[:, p] - 1].reshape(35, 35, order="F"), x)
            assert abs(u - Up[t, 0, s]) <= 1e-9 * max(1.0, abs(u))
            J += 0.25 * x[0] ** 2 + 0.05 * x[1] ** 2 + 0.05 * u * u
            x = A @ x + B[:, 0] * u
            assert np.allclose(x, Xp[t, :, s + 1], rtol=1e-9, atol=1e-12)
        assert np.allclose(x, Xf[:, t], rtol=1e-9) and abs(J - cost[t]) <= 1e-9 * J
