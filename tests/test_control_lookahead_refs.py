"""CPU tests of the lookahead under a control-dependent node set (hjb_rollout_set_control_lookahead /
hjb_rollout_run_control_lookahead / hjb_rollout_control_lookahead_host / hjb_rollout_run_control_lookahead_campaign,
csrc/hjbdp_ctrl_lookahead.h: K35, K36): the host twin - the functions the kernels call - bit for bit against
tests/control_lookahead_rollout_refs.py, its identities with the K27 and K26 twins, the restatement's plant against
tests/actuator_rollout_refs.py's, the prototypes in both headers and the ctypes table, the refusals that need no object, the
marshalling of hjbdp.ControlLookaheadRollout on test_rollout_run_marshalling.py's recording stand-in, and the header as a plain C++
program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import actuator_rollout_refs as arefs
import control_lookahead_rollout_refs as refs
import greedy_rollout_refs as grefs
from test_rollout_lookahead_abi import NAMES, _same, check_bits

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CTRL_FNS = {"hjb_rollout_set_control_lookahead": 6, "hjb_rollout_run_control_lookahead": 16, "hjb_rollout_control_lookahead_host": 33,
            "hjb_rollout_run_control_lookahead_campaign": 12}
FOUR = {"set_control_lookahead", "clear_control_lookahead", "run_control_lookahead", "run_control_lookahead_campaign"}


@pytest.fixture(scope="module")
def lib(built):
    import hjbdp
    return hjbdp.load_library()


# ---- the host twin against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["expect", "worst"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_host_twin_equals_the_restatement_bit_for_bit(lib, D, dtype, mode):
    import hjbdp
    rng = np.random.default_rng(3500 + 10 * D + np.dtype(dtype).itemsize + (100 if mode == "worst" else 0))
    planes = [2, 0, 0, -1, 1]                              # a repeated plane, the zero function
    for W, nu, nl, with_c in ((1, 1, 5, True), (2, 4, 2, False), (5, 2, 5, True)):
        knots, ut, A, B, c, q, r, V = grefs.random_problem(rng, D, nu, nl, 3, dtype)
        if nu > 1:
            B[D - 1, 0] = 0.0                              # a term of the plant that does not exist
        X0 = grefs.starts(rng, knots, 12)
        axes = sorted({0, D - 1}) if D > 2 else [D - 1]    # a proper subset of the axes from D = 2 on
        E, P = refs.control_table(rng, D, W, nl, axes, with_weights=(mode == "expect" and W != 2))
        cc = c if with_c else None
        eps, base, _ = refs.actuator_set(rng, D, nu, with_base=with_c)
        nodes = rng.integers(0, 3, size=(12, len(planes))).astype(np.int32)
        for kw in ({}, dict(nodes=nodes, eps=eps, base=base)):
            ref = refs.rollout(knots, ut, A, B, V, X0, planes, E, P, mode, c=cc, q=q, r=r, index_base=1, **kw)
            out = hjbdp.control_lookahead_host(knots, ut, A, B, V, X0, planes, E, P, mode, c=cc, q=q, r=r, index_base=1, keep_path=True, **kw)
            check_bits(out, ref, (D, W, nu, nl, bool(kw)))
        lean = hjbdp.control_lookahead_host(knots, ut, A, B, V, X0, planes, E, P, mode, c=cc, q=q, r=r, nodes=nodes, eps=eps, base=base)
        assert lean["X_path"] is None and lean["V_path"] is None
        assert _same(lean["X_final"], ref[0]) and _same(lean["cost"], ref[1])
        nominal = refs.rollout(knots, ut, A, B, V, X0, planes, E, P, mode, c=cc, q=q, r=r, index_base=1)
        assert not _same(nominal[0], ref[0])               # (the plant did move the flight)


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_a_table_constant_along_l_is_the_lookahead_twin_and_one_zero_node_the_greedy_twin(lib, D):
    import hjbdp
    import lookahead_rollout_refs as lrefs
    rng = np.random.default_rng(3560 + D)
    for dtype in (np.float32, np.float64):
        knots, ut, A, B, c, q, r, V = grefs.random_problem(rng, D, 1 + D % 4, 5, 3, dtype)
        X0 = grefs.starts(rng, knots, 24)
        planes = [2, 0, -1, 1, 1]
        axes = sorted({0, D - 1}) if D > 2 else [D - 1]
        for mode in ("expect", "worst"):
            E, P = lrefs.node_sets(rng, D, 3, axes, with_weights=(mode == "expect"))
            want = hjbdp.lookahead_host(knots, ut, A, B, V, X0, planes, E, P, mode, c=c, q=q, r=r, keep_path=True)
            got = hjbdp.control_lookahead_host(knots, ut, A, B, V, X0, planes, np.repeat(E[:, :, None], 5, axis=2), P, mode, c=c, q=q, r=r,
                                               keep_path=True)
            for name in NAMES:
                assert _same(got[name], want[name]), (D, dtype, mode, name)
        want = hjbdp.greedy_host(knots, ut, A, B, V, X0, planes, c=c, q=q, r=r, keep_path=True)
        zero = np.zeros((D, 1, 5))
        zero[D - 1, 0, 3] = -0.0
        for mode, P in (("expect", [1.0]), ("expect", None), ("worst", None)):
            out = hjbdp.control_lookahead_host(knots, ut, A, B, V, X0, planes, zero, P, mode, c=c, q=q, r=r, keep_path=True)
            for name in NAMES:
                assert _same(out[name], want[name]), (D, dtype, mode, name)


def test_the_per_candidate_read_is_live(lib):
    """with the table of the first label alone for every candidate the values differ: the rows of label l are read for label l"""
    import hjbdp
    rng = np.random.default_rng(3570)
    knots, ut, A, B, c, q, r, V = grefs.random_problem(rng, 2, 1, 5, 2, np.float64)
    X0 = grefs.starts(rng, knots, 16)
    E, P = refs.control_table(rng, 2, 3, 5, [0, 1])
    own = hjbdp.control_lookahead_host(knots, ut, A, B, V, X0, [1, 0], E, P, c=c, q=q, r=r, keep_path=True)
    first = hjbdp.control_lookahead_host(knots, ut, A, B, V, X0, [1, 0], np.repeat(E[:, :, :1], 5, axis=2), P, c=c, q=q, r=r, keep_path=True)
    assert not _same(own["V_path"], first["V_path"])


def test_the_restatements_plant_is_actuator_rollout_refs(lib):
    """one step of tests/actuator_rollout_refs.py's loop under a policy of one label everywhere, against the restatement's plant on
    that label's affine update: the same x+ bit for bit, for every label and node, with a dead input, a missing term and a base"""
    rng = np.random.default_rng(3580)
    D, nu, nl, n = 3, 3, 4, 10
    knots, ut, A, B, c, _, _, _ = grefs.random_problem(rng, D, nu, nl, 1, np.float64)
    B[2, 0] = 0.0
    eps, base, _ = refs.actuator_set(rng, D, nu)
    X0 = grefs.starts(rng, knots, n)
    nS = int(np.prod([len(k) for k in knots]))
    for l in range(nl):
        nodes = rng.integers(0, 3, size=(n, 1))
        want = arefs.rollout(knots, np.full((nS, 1), l), ut, 0, A, B, X0, [0], eps, None, base, method="nearest", c=c, nodes=nodes)[0]
        u = np.repeat(ut[l][:, None], n, axis=1)
        xn = np.empty_like(X0)
        for a in range(D):
            acc = A[a, 0] * X0[0]
            for b in range(1, D):
                acc = acc + A[a, b] * X0[b]
            for j in range(nu):
                acc = acc + B[a, j] * u[j]
            xn[a] = acc + c[a]
        got = refs.actuator_plant(xn, u, B, eps, base, nodes[:, 0])
        assert _same(got, want), l
        assert not _same(got, xn)


@pytest.mark.parametrize("mode", ["expect", "worst"])
def test_the_lattice_flights_stay_on_knots_inside_the_grid_and_the_twin_flies_the_stored_labels(lib, mode):
    """What the GPU tests on the exactly posed lattice (tests/actuator_rollout_refs.py) rely on, checked here without a device:
    under the lattice's exact policy all 3^6 node sequences from all 9 starts visit only integer knots with |x| <= 4 (the grid is
    +-16: no flight leaves it and 'nearest' reads the stored label exactly), and the host twin on the exact J under the
    actuator_nodes table, flown on those sequences, is the stored labels' flight bit for bit."""
    import hjbdp
    exact = arefs.lattice_exact(mode)[::-1]                                     # plane k = step k: the stage computed last first
    labels = np.array([lab for _, lab in exact]).T                              # [33, 6]
    J = np.array([[float(v) for v in Jn] for Jn, _ in exact]).T                 # exact: dyadic rationals far inside double
    costs, prob, Xp = arefs.lattice_enumeration(labels)
    assert np.array_equal(Xp, np.round(Xp)) and np.abs(Xp).max() <= 4
    starts = (arefs.LATTICE_STARTS + 16).astype(np.int64)
    promised = (costs @ prob) if mode == "expect" else costs.max(axis=1)
    assert np.array_equal(promised, J[starts, 0])
    seqs, _ = arefs.lattice_sequences()
    off, _ = hjbdp.actuator_nodes([[1.0]], arefs.LATTICE_U, arefs.LATTICE_EPS)
    K = arefs.LATTICE_STAGES
    X0 = np.repeat(arefs.LATTICE_STARTS, seqs.shape[0]).reshape(1, -1)
    out = hjbdp.control_lookahead_host([arefs.LATTICE_KNOTS], arefs.LATTICE_U, [[1.0]], [[1.0]], J, X0, list(range(1, K)) + [-1], off,
                                       arefs.LATTICE_P if mode == "expect" else None, mode, q=[1.0], r=[arefs.LATTICE_R],
                                       nodes=np.tile(seqs, (9, 1)), eps=arefs.LATTICE_EPS, keep_path=True)
    assert _same(out["cost"].reshape(9, -1), costs) and _same(out["X_path"][:, 0, :].reshape(9, -1, K + 1), Xp)
    node = out["X_path"][:, 0, :].astype(np.int64) + 16
    for k in range(K):
        assert np.array_equal(out["L_path"][:, k], labels[node[:, k], k]) and _same(out["V_path"][:, k], J[node[:, k], k]), k


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_prototypes_are_identical_in_both_headers_and_the_ctypes_table(lib):
    from hjbdp import _abi
    from test_abi import _prototypes
    full = _prototypes((ROOT / "include" / "hjbdp.h").read_text())
    flat = _prototypes((ROOT / "include" / "hjbdp_matlab.h").read_text())
    for name, arity in CTRL_FNS.items():
        assert name in full and name in flat and name in _abi.SYMBOLS, name
        assert full[name] == flat[name], (name, full[name], flat[name])
        assert len(full[name]) == arity and len(_abi.SYMBOLS[name][1]) == arity, (name, full[name])
        assert hasattr(lib, name), name
    # the run functions take hjb_rollout_run_lookahead's and hjb_rollout_run_lookahead_campaign's arguments exactly
    assert full["hjb_rollout_run_control_lookahead"] == full["hjb_rollout_run_lookahead"]
    assert full["hjb_rollout_run_control_lookahead_campaign"] == full["hjb_rollout_run_lookahead_campaign"]
    assert _abi.SYMBOLS["hjb_rollout_run_control_lookahead"] == _abi.SYMBOLS["hjb_rollout_run_lookahead"]
    assert _abi.SYMBOLS["hjb_rollout_run_control_lookahead_campaign"] == _abi.SYMBOLS["hjb_rollout_run_lookahead_campaign"]
    # the setter is hjb_rollout_set_lookahead's with n_controls behind n_nodes, as hjb_set_control_disturbance is hjb_set_disturbance's
    a, b = full["hjb_rollout_set_control_lookahead"], full["hjb_rollout_set_lookahead"]
    assert a[:3] == b[:3] and a[4:] == b[3:] and a[3] == full["hjb_set_control_disturbance"][3]
    # the twin: hjb_rollout_greedy_host's 24 arguments first
    assert full["hjb_rollout_control_lookahead_host"][:24] == full["hjb_rollout_greedy_host"]
    shim = (ROOT / "optimal-control-dynamic-programming_amd" / "matlab" / "Dynamic_Solver_hjbdp_actuator_lookahead_cost_map.m").read_text()
    for name in ("hjb_rollout_set_control_lookahead", "hjb_rollout_set_actuator_noise", "hjb_rollout_run_control_lookahead_campaign"):
        assert name in shim, name


def _err(lib):
    return lib.hjb_rollout_last_error(None).decode()


def test_refusals_that_need_no_object(lib):
    from hjbdp import _abi
    d = (C.c_double * 8)(*([0.5] * 8))
    bad_w = (C.c_double * 2)(0.5, -0.5)
    E, Wo = _abi.HJB_DIST_EXPECT, _abi.HJB_DIST_WORST
    who = "hjb_rollout_set_control_lookahead"
    for args, text in (((2, 1, 1, d, None), "mode 2 is not"), ((E, -1, 1, d, None), "n_nodes=-1 not in 0..128"),
                       ((E, 129, 1, d, None), "n_nodes=129 not in 0..128"), ((E, 2, 1, None, None), "null offsets with n_nodes=2"),
                       ((E, 2, 1, d, bad_w), "weight 1 is not finite or is negative"), ((Wo, 2, 1, d, d), "weights given with HJB_DIST_WORST"),
                       ((E, 2, -1, d, None), "n_controls=-1"), ((E, 1, 1, d, None), "null handle"), ((E, 0, 0, None, None), "null handle")):
        assert lib.hjb_rollout_set_control_lookahead(None, *args) == _abi.HJB_E_INVALID, args
        assert text in _err(lib) and who in _err(lib), (_err(lib), text)
    p = (C.c_int32 * 1)(0)
    out = (C.c_double * 8)(*([7.0] * 8))
    ms = C.c_double(-1.0)
    who = "hjb_rollout_run_control_lookahead"
    for fly, first, wp, text in ((2, 0, None, "fly_noise=2 is not 0 or 1"), (-1, 0, None, "fly_noise=-1"), (0, 0, out, "W_path given with fly_noise=0"),
                                 (1, -1, None, "first_stream=-1 < 0"), (1, 2 ** 63 - 1, None, "first_stream + n_traj overflows")):
        assert lib.hjb_rollout_run_control_lookahead(None, fly, 1, p, 1, d, 0, first, out, out, None, None, None, None, wp,
                                                     C.byref(ms)) == _abi.HJB_E_INVALID
        assert text in _err(lib) and who in _err(lib), (_err(lib), text)
    for fly in (0, 1):
        assert lib.hjb_rollout_run_control_lookahead(None, fly, 1, p, 1, d, 0, 0, out, out, None, None, None, None, None,
                                                     C.byref(ms)) == _abi.HJB_E_INVALID
        assert "null handle" in _err(lib)
    who = "hjb_rollout_run_control_lookahead_campaign"
    for args, text in (((1, 1, d, 0, -1), "first_stream=-1 < 0"), ((1, 0, d, 0, 0), "n_samples=0 < 1"),
                       ((2 ** 40, 2 ** 40, d, 0, 0), "n_starts * n_samples overflows"), ((1, 1, d, 0, 0), "null handle")):
        assert lib.hjb_rollout_run_control_lookahead_campaign(None, 1, p, *args, None, None, out, C.byref(ms)) == _abi.HJB_E_INVALID
        assert text in _err(lib), (_err(lib), text)
        if "null handle" not in text:
            assert who in _err(lib)
    assert list(out) == [7.0] * 8 and ms.value == -1.0


def test_host_twin_refusals(lib):
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(3)
    knots, ut, A, B, c, q, r, V = grefs.random_problem(rng, 2, 2, 3, 2, np.float64)
    X0 = grefs.starts(rng, knots, 4)
    E = np.zeros((2, 2, 3))
    E[0, 1, 2] = 0.1
    for planes, text in (([2], "outside [-1, 2)"), ([0, 1, 5], "value_plane_of_step[2] = 5")):
        with pytest.raises(hjbdp.HjbError) as ei:
            hjbdp.control_lookahead_host(knots, ut, A, B, V, X0, planes, E)
        assert text in str(ei.value) and "hjb_rollout_control_lookahead_host" in str(ei.value), str(ei.value)
    with pytest.raises(hjbdp.HjbError) as ei:
        hjbdp.control_lookahead_host(knots, ut, A, B, V, X0, [0, 0], E, nodes=np.array([[0, 1]] * 3 + [[0, 2]]), eps=[0.1, -0.1])
    assert "nodes element 7 = 2 outside [0, 2)" in str(ei.value)
    for bad in (dict(offsets=E[:, :, :2]), dict(offsets=E, weights=[0.5, 0.5], mode="worst"), dict(offsets=np.where(E > 0, np.inf, E)),
                dict(offsets=E, nodes=np.zeros((4, 1), dtype=np.int32)), dict(offsets=E, nodes=np.zeros((4, 1), dtype=np.int32), eps=[[0.1]])):
        with pytest.raises(ValueError):
            hjbdp.control_lookahead_host(knots, ut, A, B, V, X0, [0], **bad)
    # the library's own refusals of the set, past the Python checks
    n = (C.c_int32 * 2)(len(knots[0]), len(knots[1]))
    kc = np.concatenate(knots)
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    utc, Ac, Bc, X, Xf = (np.ascontiguousarray(a, dtype=np.float64) for a in (ut.reshape(-1, order="F"), A.reshape(-1, order="F"),
                                                                              B.reshape(-1, order="F"), X0.T, np.full((4, 2), 7.0)))
    p = (C.c_int32 * 1)(0)
    nd = (C.c_int32 * 4)(0, 1, 0, 1)

    def call(mode, W, nc, off, w, nodes=None, Wf=0, eps=None, base=None):
        return lib.hjb_rollout_control_lookahead_host(2, n, f(kc), 3, 2, f(utc), f(Ac), f(Bc), None, None, None, _abi.HJB_F64, 2, V.ctypes.data, 1,
                                                      p, 4, f(X), f(Xf), None, None, None, None, None, mode, W, nc, f(off), f(w), nodes, Wf,
                                                      f(eps), f(base))
    off = np.zeros(12)
    off[9] = np.nan                                        # axis 1, node 0, control 2
    for args, status, text in (((0, 0, 3, off, None), _abi.HJB_E_INVALID, "n_nodes=0 < 1"),
                               ((0, 2, 2, off, None), _abi.HJB_E_INVALID, "n_controls=2, the problem has 3 labels"),
                               ((0, 2, 3, off, None), _abi.HJB_E_INVALID, "offset of axis 1, node 0, control 2 is not finite"),
                               ((3, 2, 3, off, None), _abi.HJB_E_INVALID, "mode 3"),
                               ((1, 2, 3, np.zeros(12), np.ones(2)), _abi.HJB_E_INVALID, "weights given with HJB_DIST_WORST"),
                               ((0, 2, 3, np.zeros(12), None, nd, 0, np.zeros(4)), _abi.HJB_E_INVALID, "n_flight_nodes=0 not in 1..128"),
                               ((0, 2, 3, np.zeros(12), None, nd, 2, None), _abi.HJB_E_INVALID, "nodes given with null eps"),
                               ((0, 2, 3, np.zeros(12), None, nd, 2, np.array([0.1, np.inf, 0, 0])), _abi.HJB_E_INVALID, "eps is not finite"),
                               ((0, 2, 3, np.zeros(12), None, nd, 2, np.zeros(4), np.array([0.1, np.nan, 0, 0])), _abi.HJB_E_INVALID,
                                "base is not finite")):
        assert call(*args) == status and text in _err(lib) and "hjb_rollout_control_lookahead_host" in _err(lib), (args, _err(lib))
        assert np.all(Xf == 7.0)
    assert call(0, 2, 3, np.zeros(12), None, nd, 2, np.zeros(4)) == _abi.HJB_OK and not np.any(Xf == 7.0)


# ---- marshalling: hjbdp.ControlLookaheadRollout on a recording stand-in for the library ---------------------------------------------
@pytest.fixture
def fake_ro():
    import hjbdp
    from test_rollout_run_marshalling import D, NU, FakeLib
    r = object.__new__(hjbdp.ControlLookaheadRollout)
    r.lib, r._ro = FakeLib(), C.c_void_p(0x1234)
    r.D, r.n_u, r.n, r.n_labels = D, NU, [3, 3], 3
    yield r
    r._ro = C.c_void_p()                                                        # nothing to destroy


def test_control_lookahead_rollout_is_an_actuator_rollout_with_four_more_methods():
    import hjbdp
    assert issubclass(hjbdp.ControlLookaheadRollout, hjbdp.ActuatorRollout)
    assert set(dir(hjbdp.ControlLookaheadRollout)) - set(dir(hjbdp.ActuatorRollout)) == FOUR
    assert "ControlLookaheadRollout" in hjbdp.__all__ and "control_lookahead_host" in hjbdp.__all__


@pytest.mark.parametrize("actuator", [False, True], ids=["nominal", "actuator"])
@pytest.mark.parametrize("keep", [False, True], ids=["no_path", "keep_path"])
def test_run_control_lookahead_hands_run_lookaheads_arguments_over(fake_ro, keep, actuator):
    from hjbdp import _abi
    from test_rollout_run_marshalling import D, FIRST, K, NT, NU, SEED, VPLANES, _arr, _filled, _x0
    ro = fake_ro
    types = _abi.SYMBOLS["hjb_rollout_run_control_lookahead"][1]
    ro.lib.outs = range(8, 15)                                                  # X_final, cost, X_path, U_path, L_path, V_path, W_path
    X0 = _x0(D)
    out = ro.run_control_lookahead(X0, VPLANES, actuator=actuator, seed=SEED, first_stream=FIRST, keep_path=keep)
    (called, args), = ro.lib.calls
    assert called == "hjb_rollout_run_control_lookahead" and len(args) == len(types) == 16
    assert args[0] is ro._ro and args[1:3] == (int(actuator), K) and args[4] == NT
    assert _arr(args[3]).dtype == np.int32 and _arr(args[3]).tolist() == VPLANES.tolist()
    assert _arr(args[5]).flags.c_contiguous and np.array_equal(_arr(args[5]), X0.T)      # [n_traj, D]
    assert args[6:8] == (SEED % 2 ** 64, FIRST)                                 # the seed reduced to 64 bits
    assert set(out) == {"X_final", "cost", "X_path", "U_path", "L_path", "V_path", "W_path", "device_ms"} and out["device_ms"] == 1.5
    assert np.array_equal(out["X_final"], _filled(8, NT * D).reshape(NT, D).T)
    assert np.array_equal(out["cost"], _filled(9, NT))
    if keep:
        assert out["X_path"].shape == (NT, D, K + 1) and out["U_path"].shape == (NT, NU, K)
        assert out["L_path"].dtype == np.int32 and out["L_path"].shape == (NT, K) and out["V_path"].shape == (NT, K)
        assert np.array_equal(out["V_path"].reshape(-1, order="F"), _filled(13, NT * K))
        if actuator:
            assert out["W_path"].dtype == np.int32 and np.array_equal(out["W_path"].reshape(-1, order="F"), _filled(14, NT * K).astype(np.int32))
        else:
            assert args[14] is None and out["W_path"] is None                   # a nominal plant draws no node
    else:
        assert all(a is None for a in args[10:15])
        assert all(out[k] is None for k in ("X_path", "U_path", "L_path", "V_path", "W_path"))


def test_set_control_lookahead_and_the_campaign_hand_their_arguments_over(fake_ro):
    from hjbdp import _abi
    from test_rollout_run_marshalling import D, FIRST, K, NT, SEED, VPLANES, _arr, _x0
    ro = fake_ro
    E = np.arange(12.0).reshape(D, 2, 3)                                        # [D, W = 2, n_labels = 3]
    ro.set_control_lookahead(E, [0.25, 0.75])
    ro.set_control_lookahead(E, mode="worst")
    ro.clear_control_lookahead()
    (n1, a1), (n2, a2), (n3, a3) = ro.lib.calls
    assert n1 == n2 == n3 == "hjb_rollout_set_control_lookahead" and len(a1) == len(_abi.SYMBOLS[n1][1]) == 6
    assert a1[1:4] == (_abi.HJB_DIST_EXPECT, 2, 3) and _arr(a1[5]).tolist() == [0.25, 0.75]
    assert _arr(a1[4]).tolist() == [E[a, w, l] for l in range(3) for w in range(2) for a in range(D)]      # offsets[a + D * (w + W * l)]
    assert a2[1:4] == (_abi.HJB_DIST_WORST, 2, 3) and a2[5] is None
    assert a3[1:] == (_abi.HJB_DIST_EXPECT, 0, 0, None, None)
    for bad in (E[:, :, :2], np.zeros((D, 2)), np.where(E == 5, np.nan, E)):    # a wrong label count, no label axis, not finite
        with pytest.raises(ValueError):
            ro.set_control_lookahead(bad)
    assert len(ro.lib.calls) == 3
    ro.lib.calls.clear()
    ro.lib.outs = (10,)
    out = ro.run_control_lookahead_campaign(_x0(D), VPLANES, 8, seed=SEED, first_stream=FIRST, cost_threshold=2.0, settle_tol=[0.1, 0.2])
    (called, args), = ro.lib.calls
    assert called == "hjb_rollout_run_control_lookahead_campaign" and len(args) == len(_abi.SYMBOLS[called][1]) == 12
    assert args[1] == K and _arr(args[2]).tolist() == VPLANES.tolist() and args[3:5] == (NT, 8) and args[6:8] == (SEED % 2 ** 64, FIRST)
    assert _arr(args[8]).tolist() == [2.0] * NT and _arr(args[9]).tolist() == [0.1, 0.2]
    assert out["stats"].shape == (NT, 8) and out["device_ms"] == 1.5


def test_dynamic_solver_actuator_lookahead_methods_refuse_before_any_device_work(built):
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N, ds.dx, ds.du = 4, 9, 7
    ds.build_spec()
    ds.u_star_idxs = np.ones((9, 9, 3), dtype=np.int32)           # as if run() had been
    ds.J_star = np.zeros((9, 9, 4))
    X0 = np.zeros((2, 1))
    for fly in (lambda: ds.get_actuator_lookahead_paths(X0), lambda: ds.get_actuator_lookahead_paths(X0, 2),
                lambda: ds.get_actuator_lookahead_cost_statistics(X0, 2), lambda: ds.actuator_lookahead_cost_map(2)):
        with pytest.raises(RuntimeError, match="actuator_noise"):
            fly()
    ds.actuator_noise = ([-0.1, 0.0, 0.1], None, "expect")
    for old in (lambda: ds.get_lookahead_paths(X0), lambda: ds.get_noisy_paths(X0, 2), lambda: ds.get_lookahead_cost_statistics(X0, 2)):
        with pytest.raises(RuntimeError, match="control-dependent noise"):      # the additive flights keep refusing
            old()
    with pytest.raises(ValueError, match="n_samples"):
        ds.get_actuator_lookahead_paths(X0, 0)
    ds.u_star_idxs = None
    with pytest.raises(RuntimeError, match="run"):
        ds.get_actuator_lookahead_paths(X0)


# ---- the header as a plain C++ program under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness_out(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ctrl_lookahead") / "ctrl_lookahead_harness"
    # host code only: the program is plain C++ (no device pass), and the sanitizers are kept off any GPU code explicitly
    r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I%s/optimal-control-dynamic-programming_amd/csrc" % ROOT, "-o", str(exe),
                        "%s/tests/ctrl_lookahead_harness.cpp" % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_sanitized_cpp_harness_prints_the_restatements_bits(harness_out):
    knots = [np.array([-1.0, -0.25, 0.5, 1.0]), np.array([-1.0, 0.0, 1.0])]
    ut = np.array([[0.5, -0.125], [-0.75, 0.25], [0.5, -0.125]])
    A = np.array([[0.875, 0.25], [-0.125, 0.75]])
    B = np.array([[0.5, -0.25], [0.125, 0.375]])
    c, q, r = [0.0625, -0.03125], [0.75, 0.3], [0.1, 0.7]
    X0 = np.array([[0.3, -0.4], [-0.25, 0.0], [1.0, 1.0], [1.15, -1.2]]).T
    E = np.zeros((2, 3, 3))
    E[1, :, 0] = [-0.3, 0.0, 0.45]
    E[1, :, 1] = [0.2, -0.35, 0.05]
    eps = np.array([[0.5, 0.0], [-0.25, -0.0]])                                 # [W_f, n_u]: input 1 is dead
    base = np.array([[0.125, -0.0625], [0.0, -0.0]])
    nodes = np.array([0, 1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1]).reshape((4, 3), order="F")
    i = np.arange(24)
    vals = ((i * 37 + 11) % 17) / 16.0 + (i % 3) * 0.1
    assert len(harness_out) == 24, harness_out
    lines = iter(harness_out)
    for ty, dt in (("f32", np.float32), ("f64", np.float64)):
        V = vals.astype(dt).reshape((12, 2), order="F")
        for mode, P in (("expect", [0.25, 0.5, 0.25]), ("worst", None)):
            ref = refs.rollout(knots, ut, A, B, V, X0, [1, 0, -1], E, P, mode, c=c, q=q, r=r, nodes=nodes, eps=eps, base=base)
            for name, want in zip(NAMES, ref):
                want = np.asarray(want, dtype=np.float64)
                flat = want.reshape(-1, order="F") if name != "X_final" else want.T.reshape(-1)
                assert next(lines) == "%s %s %s %s" % (ty, mode, name, " ".join("%016x" % w for w in flat.view(np.uint64))), (ty, mode, name)
