"""CPU tests of the actuator-noise flights' interface (hjb_rollout_set_actuator_noise, hjb_rollout_run_actuator,
hjb_rollout_run_actuator_campaign) and of what the GPU tests stand on (tests/actuator_rollout_refs.py): the lattice problem is
exactly posed - re-asserted here in exact rationals, case by case - the prototypes in both headers and the ctypes table, the
refusals that need no object, how hjbdp.ActuatorRollout hands its arguments to the library (on the recording stand-in of
tests/test_rollout_run_marshalling.py), and Dynamic_Solver's new methods without self.actuator_noise.  No GPU."""
import ctypes as C
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import actuator_rollout_refs as refs

ROOT = Path(__file__).resolve().parent.parent
ACTUATOR_FNS = ("hjb_rollout_set_actuator_noise", "hjb_rollout_run_actuator", "hjb_rollout_run_actuator_campaign")
STARTS = (refs.LATTICE_STARTS + 16).astype(np.int64)                            # the starts' state indices


@pytest.fixture(scope="module")
def lib(built):
    import hjbdp
    return hjbdp.load_library()


def _double_sweep(mode, nominal=False):
    """the backup's restatement in double, the contract's operation order (tests/control_disturbance_refs.py; the nominal
    problem: one zero node) -> (J [33, 6], labels [33, 6]), plane k = step k"""
    from control_disturbance_refs import ControlDisturbedRef
    spec = refs.lattice_spec(mode, nominal=nominal)
    off, wts = (np.zeros((1, 1, refs.LATTICE_U.size)), None) if nominal else spec.control_disturbance[:2]
    sweep = ControlDisturbedRef(spec, off, wts, "expect" if nominal else mode).sweep(refs.LATTICE_STAGES)
    return np.stack([J for J, _ in sweep[::-1]], axis=1), np.stack([lab for _, lab in sweep[::-1]], axis=1)


def _frac(a):
    return [Fraction(float(v)) for v in np.asarray(a).reshape(-1)]


@pytest.mark.parametrize("mode", ["expect", "worst"])
def test_lattice_sweep_is_the_same_in_rationals_and_in_double(built, mode):
    exact = refs.lattice_exact(mode)[::-1]                                      # plane k = step k
    J, labels = _double_sweep(mode)
    for k in range(refs.LATTICE_STAGES):
        assert _frac(J[:, k]) == exact[k][0], (mode, k)
        assert labels[:, k].tolist() == exact[k][1], (mode, k)


@pytest.mark.parametrize("mode", ["expect", "worst"])
def test_lattice_promise_is_the_enumerated_flights_cost(built, mode):
    """flown from every start over all 3^6 node sequences, the expectation ('expect') and the maximum ('worst') equal J at stage 1
    exactly, and the flown states stay within |x| <= 4"""
    J, labels = _double_sweep(mode)
    J1 = refs.lattice_exact(mode)[-1][0]
    costs, prob, X = refs.lattice_enumeration(labels)
    assert costs.shape == (9, 729) and prob.sum() == 1.0
    assert np.abs(X).max() <= 4.0 and np.all(X == np.round(X))
    assert np.all((costs * 2) % 1 == 0)                                         # multiples of 1/2: g = x^2 + u^2 / 8 on u in {0, +-2, +-4}
    pf = _frac(prob)
    for i, s in enumerate(STARTS):
        cf = _frac(costs[i])
        if mode == "expect":
            assert sum(p * c for p, c in zip(pf, cf)) == J1[s], (i, s)
            assert (costs[i] @ prob) == J[s, 0]                                 # and so is the double sum: dyadic rationals throughout
        else:
            assert max(cf) == J1[s] and costs[i].max() == J[s, 0], (i, s)


def test_lattice_policies_differ_from_the_nominal_one(built):
    """'expect': at x = -1 the policy commands 2 where the nominal commands 0; 'worst': it promises 53/2 at x = +-4 where the
    nominal promises 18 - so a flight that ignored eps, or a design that ignored it, would be seen"""
    nominal = refs.lattice_exact("expect", nominal=True)
    nJ, nlab = _double_sweep("expect", nominal=True)
    assert _frac(nJ[:, 0]) == nominal[-1][0] and nlab[:, 0].tolist() == nominal[-1][1]
    expect, worst = refs.lattice_exact("expect"), refs.lattice_exact("worst")
    at = lambda x: int(x) + 16
    assert refs.LATTICE_U[expect[-1][1][at(-1)]] == 2.0 and refs.LATTICE_U[nominal[-1][1][at(-1)]] == 0.0
    for x in (-4, 4):
        assert worst[-1][0][at(x)] == Fraction(53, 2) and nominal[-1][0][at(x)] == 18
    assert any(expect[k][1] != nominal[k][1] for k in range(refs.LATTICE_STAGES))


def test_restatement_with_zero_eps_is_the_additive_and_the_nominal_restatement(built):
    """the restatement's own consistency (consequence (i)): eps all +-0 with a base is tests/noisy_rollout_refs.py's rollout under
    that base; with no base, or a base of +-0, it is tests/rollout_refs.py's"""
    import noisy_rollout_refs
    import rollout_refs
    rng = np.random.default_rng(5)
    knots = [np.linspace(-1, 1, 4), np.linspace(-2, 2, 5)]
    labels = rng.integers(0, 6, size=(20, 3)).astype(np.int32)
    ut = rng.uniform(-1, 1, size=(6, 2))
    A, B = rng.uniform(-0.4, 0.4, size=(2, 2)), rng.uniform(-0.1, 0.1, size=(2, 2))
    X0 = rng.uniform(-1, 1, size=(2, 11))
    planes = [0, 2, 1, 1, 0]
    kw = dict(q=[1.0, 2.0], r=[0.5, 0.25])
    zero = np.array([[0.0, -0.0], [-0.0, 0.0], [0.0, 0.0]])                     # [W = 3, n_u = 2]
    base, p = np.array([[0.0, -0.0, 0.0], [0.25, -0.25, 0.5]]), [1.0, 2.0, 1.0]
    nominal = rollout_refs.rollout(knots, labels, ut, 0, A, B, X0, planes, "linear", **kw)
    for b in (None, np.zeros((2, 3)), -np.zeros((2, 3))):
        got = refs.rollout(knots, labels, ut, 0, A, B, X0, planes, zero, p, b, seed=4, **kw)
        assert all(np.array_equal(g, w) for g, w in zip(got[:4], nominal))
    additive = noisy_rollout_refs.rollout(knots, labels, ut, 0, A, B, X0, planes, base, p, seed=4, **kw)
    got = refs.rollout(knots, labels, ut, 0, A, B, X0, planes, zero, p, base, seed=4, **kw)
    assert all(np.array_equal(g, w) for g, w in zip(got, additive))
    moved = refs.rollout(knots, labels, ut, 0, A, B, X0, planes, [0.5, -0.5, 0.25], p, base, seed=4, **kw)
    assert np.array_equal(moved[4], additive[4]) and not np.array_equal(moved[0], additive[0])     # the same nodes, another plant
    assert np.array_equal(moved[3][:, :, 0], additive[3][:, :, 0])              # the first commanded u is the same: U_path is not the delivered one


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_actuator_prototypes_are_identical_in_both_headers_and_the_table(lib):
    from hjbdp import _abi
    from test_abi import _prototypes
    full = _prototypes((ROOT / "include" / "hjbdp.h").read_text())
    flat = _prototypes((ROOT / "include" / "hjbdp_matlab.h").read_text())
    for name in ACTUATOR_FNS:
        assert name in full and name in flat and name in _abi.SYMBOLS, name
        assert full[name] == flat[name], (name, full[name], flat[name])
        assert len(_abi.SYMBOLS[name][1]) == len(full[name]), name
        assert hasattr(lib, name), name
    # the run functions take hjb_rollout_run_noisy's and hjb_rollout_run_campaign's arguments
    assert full["hjb_rollout_run_actuator"] == full["hjb_rollout_run_noisy"]
    assert full["hjb_rollout_run_actuator_campaign"] == full["hjb_rollout_run_campaign"]
    assert _abi.SYMBOLS["hjb_rollout_run_actuator"] == _abi.SYMBOLS["hjb_rollout_run_noisy"]
    assert _abi.SYMBOLS["hjb_rollout_run_actuator_campaign"] == _abi.SYMBOLS["hjb_rollout_run_campaign"]
    text = (ROOT / "include" / "hjbdp.h").read_text()
    assert "is not built" not in text


def _err(lib):
    return lib.hjb_rollout_last_error(None).decode()


def test_actuator_refusals_that_need_no_object(lib):
    from hjbdp import _abi
    d = (C.c_double * 8)(*([0.5] * 8))
    bad = lambda *v: (C.c_double * len(v))(*v)
    who = "hjb_rollout_set_actuator_noise"
    for args, text in (((-1, d, None, None), "n_nodes=-1 not in 0..128"),
                       ((129, d, None, None), "n_nodes=129 not in 0..128"),
                       ((2, None, None, None), "null eps with n_nodes=2"),
                       ((2, None, d, None), "null eps with n_nodes=2"),
                       ((2, d, None, bad(1.0, float("nan"))), "weight 1 is not finite or is negative"),
                       ((3, d, d, bad(1.0, 1.0, -1e-300)), "weight 2 is not finite or is negative"),
                       ((2, d, None, bad(0.0, 0.0)), "weights sum to 0"),
                       ((1, d, None, None), "null handle"),
                       ((0, None, None, None), "null handle")):
        assert lib.hjb_rollout_set_actuator_noise(None, *args) == _abi.HJB_E_INVALID, args
        assert text in _err(lib) and who in _err(lib), (_err(lib), text)
    out = (C.c_double * 8)(*([7.0] * 8))
    ms = C.c_double(-1.0)
    for first, n_traj, text in ((-1, 1, "first_stream=-1 < 0"), (2 ** 63 - 1, 1, "overflows"), (2 ** 63 - 5, 6, "overflows")):
        assert lib.hjb_rollout_run_actuator(None, 1, 0, None, n_traj, d, 0, first, out, out, None, None, None, C.byref(ms)) == _abi.HJB_E_INVALID
        assert text in _err(lib) and "hjb_rollout_run_actuator" in _err(lib), (_err(lib), text)
    assert lib.hjb_rollout_run_actuator(None, 1, 0, None, 1, d, 0, 0, out, out, None, None, None, C.byref(ms)) == _abi.HJB_E_INVALID
    assert "null handle" in _err(lib)
    for args, text in (((1, 1, d, 0, -1), "first_stream=-1 < 0"), ((1, 0, d, 0, 0), "n_samples=0 < 1"),
                       ((2 ** 40, 2 ** 40, d, 0, 0), "n_starts * n_samples overflows"), ((1, 1, d, 0, 0), "null handle")):
        assert lib.hjb_rollout_run_actuator_campaign(None, 1, 0, None, *args, None, None, out, C.byref(ms)) == _abi.HJB_E_INVALID
        assert text in _err(lib), (_err(lib), text)
        if "null handle" not in text:
            assert "hjb_rollout_run_actuator_campaign" in _err(lib)
    assert list(out) == [7.0] * 8 and ms.value == -1.0


# ---- marshalling: hjbdp.ActuatorRollout on a recording stand-in for the library (tests/test_rollout_run_marshalling.py's) ------
@pytest.fixture
def fake_ro():
    import hjbdp
    from test_rollout_run_marshalling import D, NU, FakeLib
    r = object.__new__(hjbdp.ActuatorRollout)
    r.lib, r._ro = FakeLib(), C.c_void_p(0x1234)
    r.D, r.n_u, r.n = D, NU, [3, 3]
    yield r
    r._ro = C.c_void_p()                                                        # nothing to destroy


def test_actuator_rollout_is_a_rollout_with_four_more_methods():
    import hjbdp
    assert issubclass(hjbdp.ActuatorRollout, hjbdp.Rollout)
    assert set(dir(hjbdp.ActuatorRollout)) - set(dir(hjbdp.Rollout)) == {"set_actuator_noise", "clear_actuator_noise", "run_actuator",
                                                                           "run_actuator_campaign"}


@pytest.mark.parametrize("keep", [False, True], ids=["no_path", "keep_path"])
def test_run_actuator_hands_run_noisys_arguments_over(fake_ro, keep):
    from hjbdp import _abi
    from test_rollout_run_marshalling import D, FIRST, K, NT, NU, PLANES, SEED, _arr, _filled, _x0
    ro = fake_ro
    types = _abi.SYMBOLS["hjb_rollout_run_actuator"][1]
    ro.lib.outs = range(8, 13)                                                  # X_final, cost, X_path, U_path, W_path
    X0 = _x0(D)
    out = ro.run_actuator(X0, PLANES, seed=SEED, first_stream=FIRST, method="nearest", keep_path=keep)
    (called, args), = ro.lib.calls
    assert called == "hjb_rollout_run_actuator" and len(args) == len(types) == 14
    assert args[0] is ro._ro and args[1:3] == (_abi.HJB_LOOKUP_NEAREST, K) and args[4] == NT
    assert _arr(args[3]).dtype == np.int32 and _arr(args[3]).tolist() == PLANES
    assert _arr(args[5]).flags.c_contiguous and np.array_equal(_arr(args[5]), X0.T)      # [n_traj, D]
    assert args[6:8] == (SEED % 2 ** 64, FIRST)                                 # the seed reduced to 64 bits
    assert set(out) == {"X_final", "cost", "X_path", "U_path", "W_path", "device_ms"} and out["device_ms"] == 1.5
    assert np.array_equal(out["X_final"], _filled(8, NT * D).reshape(NT, D).T)
    assert np.array_equal(out["cost"], _filled(9, NT))
    if keep:
        assert out["X_path"].shape == (NT, D, K + 1) and out["U_path"].shape == (NT, NU, K)
        assert out["W_path"].dtype == np.int32 and out["W_path"].shape == (NT, K)
        assert np.array_equal(out["W_path"].reshape(-1, order="F"), _filled(12, NT * K).astype(np.int32))
    else:
        assert args[10] is None and args[11] is None and args[12] is None
        assert out["X_path"] is None and out["U_path"] is None and out["W_path"] is None


def test_set_actuator_noise_and_the_campaign_hand_their_arguments_over(fake_ro):
    from hjbdp import _abi
    from test_rollout_run_marshalling import D, FIRST, K, NT, PLANES, SEED, _arr, _x0
    ro = fake_ro
    ro.n_u = 2
    eps, base, w = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]]), np.arange(6.0).reshape(D, 3), [1.0, 2.0, 3.0]
    ro.set_actuator_noise(eps, w, base)
    ro.set_actuator_noise([0.5, -0.5])
    ro.clear_actuator_noise()
    (n1, a1), (n2, a2), (n3, a3) = ro.lib.calls
    assert n1 == n2 == n3 == "hjb_rollout_set_actuator_noise" and len(a1) == len(_abi.SYMBOLS[n1][1]) == 5
    assert a1[1] == 3 and _arr(a1[2]).tolist() == [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]       # eps[j + n_u * w]
    assert _arr(a1[3]).tolist() == [0.0, 3.0, 1.0, 4.0, 2.0, 5.0] and _arr(a1[4]).tolist() == w   # base[a + D * w]
    assert a2[1] == 2 and _arr(a2[2]).tolist() == [0.5, 0.5, -0.5, -0.5] and a2[3] is None and a2[4] is None   # one error for every input
    assert a3[1:] == (0, None, None, None)
    ro.lib.calls.clear()
    ro.lib.outs = (11,)
    out = ro.run_actuator_campaign(_x0(D), PLANES, 8, seed=SEED, first_stream=FIRST, cost_threshold=2.0, settle_tol=[0.1, 0.2])
    (called, args), = ro.lib.calls
    assert called == "hjb_rollout_run_actuator_campaign" and len(args) == len(_abi.SYMBOLS[called][1]) == 13
    assert args[1:3] == (_abi.HJB_LOOKUP_LINEAR, K) and args[4:6] == (NT, 8) and args[7:9] == (SEED % 2 ** 64, FIRST)
    assert _arr(args[9]).tolist() == [2.0] * NT and _arr(args[10]).tolist() == [0.1, 0.2]
    assert out["stats"].shape == (NT, 8) and out["device_ms"] == 1.5


def test_dynamic_solver_actuator_methods_need_actuator_noise(built):
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N, ds.dx, ds.du = 4, 9, 7
    ds.build_spec()
    ds.u_star_idxs = np.ones((9, 9, 3), dtype=np.int32)           # as if run() had been: the flights refuse before any device work
    ds.J_star = np.zeros((9, 9, 4))
    for fly in (lambda: ds.get_actuator_paths(np.zeros((2, 1)), 2), lambda: ds.get_actuator_cost_statistics(np.zeros((2, 1)), 2),
                lambda: ds.actuator_cost_map(2)):
        with pytest.raises(RuntimeError, match="actuator_noise"):
            fly()
    ds.u_star_idxs = None
    ds.actuator_noise = ([-0.1, 0.0, 0.1], None, "expect")
    with pytest.raises(RuntimeError, match="run"):
        ds.get_actuator_paths(np.zeros((2, 1)), 2)
