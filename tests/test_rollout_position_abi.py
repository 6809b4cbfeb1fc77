"""CPU tests of the position rollout (hjb_rollout_set_position_model / hjb_rollout_run_position, csrc/kernels_rollout_position.h):
rkf45's schedule over the default horizon; the table holds what it says; the host loop on that schedule equals the reference's
RKF45 loop (Solver_position.get_optimal_path, untouched) and the numpy twin the GPU tests hold K19 to
(tests/position_rollout_refs.py) bit for bit; the off-schedule flag; the prototypes agree in both headers and are exported and
bound; null objects and every refusal that needs no object are statuses decided without a device; every K19 instantiation compiles
for gfx950 without spilling."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import position_rollout_refs as pr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "optimal-control-dynamic-programming_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW_FNS = ("hjb_rollout_set_position_model", "hjb_rollout_run_position")
START_A = (-0.3, 0.1, 0.05, 0.0, 0.01, -0.02)
EPS = float(np.finfo(np.float64).eps)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def synthetic_position_solver():
    """A bang-bang policy on the class's own 201 x 201 grid without a sweep, the same for the three channels: per state the argmin
    over U_vector of (v + 0.5 x + 0.5 u / Mass)^2 + 1e-4 u^2; first index on ties; labels 1-based."""
    import hjbdp
    from hjbdp.solver_position import NearestPolicy
    sp = hjbdp.Solver_position()
    _, s_x, s_v = sp.build_spec(0)
    U = np.asarray(sp.U_vector, dtype=np.float64)
    X, V, Uu = s_x[:, None, None], s_v[None, :, None], U[None, None, :]
    idx = (np.argmin((V + 0.5 * X + 0.5 * Uu / sp.Mass) ** 2 + 1e-4 * Uu ** 2, axis=-1) + 1).astype(np.uint8)
    for ch in range(3):
        sp.U_idx[ch] = idx
        setattr(sp, "U%d_Opt" % (ch + 1), NearestPolicy([s_x, s_v], U[idx - 1]))
    return sp


@pytest.fixture(scope="module")
def synthetic_sp():
    return synthetic_position_solver()


def _twin_channels(sp):
    from hjbdp.rollout import position_channels
    return [(k, l, t, 1) for k, l, t in position_channels(sp)]


def test_schedule_over_the_default_horizon():
    """every one of the 5,999 stages of the default horizon takes five sub-steps: formed with H/100, 4H/100, 16H/100, 64H/100 and
    256H/100, the first four applied whole and the last over what is left of the stage (15H/100)"""
    import hjbdp
    from hjbdp.rollout import position_rkf45_schedule
    sp = hjbdp.Solver_position()
    N = sp.N_stage
    assert N == 6000
    for k in range(N - 1):
        t0, tf = k * sp.h, (k + 1) * sp.h
        sched = position_rkf45_schedule(t0, tf)
        assert len(sched) == 5, (k, sched)
        H = tf - t0
        assert sched[0][0] == t0 and sched[0][1] == H / 100.0
        t = t0
        for s, (ts, hf, ha) in enumerate(sched):
            assert ts == t
            if s:
                assert hf == 4.0 * sched[s - 1][1]                   # 1 : 4 : 16 : 64 : 256
            if s < 4:
                assert ha == hf
            else:
                assert ha == tf - t and ha < hf and abs(ha / H - 0.15) < 1e-9
            t = t + ha
        assert not t < tf
    assert position_rkf45_schedule(1.0, 1.0) == []
    # a long stage: growth stops at the interval's end, whatever the count
    long = position_rkf45_schedule(0.0, 3.0)
    assert [s[1] for s in long] == [0.03 * 4 ** i for i in range(len(long))] and long[-1][0] + long[-1][2] >= 3.0


def test_table_holds_the_five_expressions_at_the_stage_times(monkeypatch):
    from hjbdp.orbit import MU_EARTH, propagate_kepler
    from hjbdp.rollout import position_rkf45_schedule, position_rkf45_table, target_R0V0
    a = (0.0, 1.0 / 4, 3.0 / 8, 12.0 / 13, 1.0, 1.0 / 2)
    mu = MU_EARTH
    R1, V1 = np.array([7000.0, 100.0, -50.0]), np.array([0.1, 7.4, 1.0])
    for n_steps, h, orbit in ((7, 0.005, None), (3, 0.25, (R1, V1))):
        R0, V0 = target_R0V0() if orbit is None else orbit
        n_sub, table = position_rkf45_table(n_steps, h) if orbit is None else position_rkf45_table(n_steps, h, R1, V1)
        assert n_sub.dtype == np.int32 and n_sub.shape == (n_steps,) and table.shape == (n_steps, n_sub.max(), 32)
        for k in range(n_steps):
            sched = position_rkf45_schedule(k * h, (k + 1) * h)
            assert n_sub[k] == len(sched)
            for s, (t, hf, ha) in enumerate(sched):
                assert table[k, s, 0] == hf and table[k, s, 1] == ha
                for j in (0, 3, 5) if k else range(6):
                    R, V = propagate_kepler(R0, V0, t + a[j] * hf, mu)
                    nR = float(np.sqrt(R @ R))
                    H = float(np.linalg.norm(np.cross(R, V)))
                    want = [2 * mu / nR ** 3 + H * H / nR ** 4, 2 * float(R @ V) / nR ** 4 * H, 2 * H / nR ** 2,
                            mu / nR ** 3 - H * H / nR ** 4, mu / nR ** 3]
                    assert _bits(table[k, s, 2 + 5 * j:7 + 5 * j], want), (n_steps, h, k, s, j)
            assert not table[k, n_sub[k]:].any()
    n_sub, table = position_rkf45_table(0, 0.005)
    assert n_sub.shape == (0,) and table.shape[0] == 0
    with pytest.raises(ValueError):
        position_rkf45_table(-1, 0.005)
    from hjbdp import rollout
    monkeypatch.setattr(rollout, "POSITION_MAX_SUB", 4)              # the schedule is scale-free (five sub-steps at any h): lower the limit
    with pytest.raises(ValueError, match="5 sub-steps"):
        position_rkf45_table(2, 0.005)


def test_fixed_loop_against_the_rkf45_loop(synthetic_sp):
    """Solver_position.get_optimal_path (orbit.rkf45 per stage, untouched) against position_optimal_path_fixed on the synthetic
    bang-bang policy: start (-0.3, 0.1, 0.05, 0, 0.01, -0.02) over 1,500 stages and the default start over 600.  Every acceleration
    column equal, no stage off schedule, and max |dX| <= 2 N n_sub eps max|X|: worst-case linear round-off accumulation (3.3e-12
    at N = 1,500, n_sub = 5, |X| <= 1; 1.0e-12 and 1.3e-12 for these two runs).  Measured with the explicit operation order:
    1.9e-16 (70 switches) and 6.9e-18 (7 switches) - a few ulp, from the order of the dot products, which rkf45 leaves to
    numpy's matmul.  The cap is not to be widened."""
    from hjbdp.rollout import position_optimal_path_fixed
    sp = synthetic_sp
    for y0, K, min_switches in ((START_A, 1500, 10), (None, 600, 0)):
        T, X, F = sp.get_optimal_path(n_steps=K, y0=y0)
        T2, X2, F2, off = position_optimal_path_fixed(sp, y0=y0, n_steps=K)
        assert X.shape == (6, K + 1) and F.shape == (3, K + 1) and _bits(T, T2) and X2.shape == X.shape and F2.shape == F.shape
        switches = int((np.abs(np.diff(F[:, :K], axis=1)).sum(axis=0) > 0).sum())
        cols_equal = int((F == F2).all(axis=0).sum())
        dX = float(np.abs(X - X2).max())
        cap = 2 * K * 5 * EPS * float(np.abs(X).max())
        print("start %r: %d of %d acceleration columns equal, %d switches, off_schedule %d, max |dX| = %.3g (cap %.3g)"
              % (y0, cols_equal, K + 1, switches, off, dX, cap))
        assert switches >= min_switches, switches
        assert cols_equal == K + 1, cols_equal
        assert off == -1
        assert dX <= cap, (dX, cap)
        assert not F2[:, K].any()


def test_twin_equals_the_fixed_loop_bit_for_bit(synthetic_sp):
    from hjbdp.rollout import position_optimal_path_fixed, position_rkf45_table
    sp = synthetic_sp
    ch = _twin_channels(sp)
    tab = position_rkf45_table(1500, sp.h, *sp.get_target_R0V0())
    for y0, K in ((START_A, 1500), ((-1.0, 0, 0, 0, 0, 0), 600)):
        Xf, Xp, Ap, off = pr.rollout(ch, tab[0], tab[1], 1e-8, np.array(y0, dtype=np.float64).reshape(6, 1), np.zeros(K, int))
        T, X, F, off1 = position_optimal_path_fixed(sp, y0=y0, n_steps=K, table=tab)
        assert _bits(Xp[0], X) and _bits(Ap[0], F[:, :K]) and _bits(Xf[:, 0], X[:, K]) and off[0] == off1 == -1
        assert off.dtype == np.int32
    # a prebuilt table and none give the same loop
    assert _bits(position_optimal_path_fixed(sp, y0=START_A, n_steps=40)[1], position_optimal_path_fixed(sp, y0=START_A, n_steps=40, table=tab)[1])
    # 32 random starts x 200 stages, inside and outside the grid
    rng = np.random.default_rng(19)
    n, K = 32, 200
    X0 = np.concatenate([rng.uniform(-0.6, 0.6, size=(3, n)), rng.uniform(-0.3, 0.3, size=(3, n))])
    Xf, Xp, Ap, off = pr.rollout(ch, tab[0], tab[1], 1e-8, X0, np.zeros(K, int))
    assert len({Ap[i].tobytes() for i in range(n)}) > n // 2                 # the starts do not all fire alike
    for i in range(n):
        T, X, F, off1 = position_optimal_path_fixed(sp, y0=X0[:, i], n_steps=K, table=tab)
        assert _bits(Xp[i], X) and _bits(Ap[i], F[:, :K]) and off[i] == off1 == -1, i


def test_flag_path(synthetic_sp):
    """with tol = 1e-30 no error test leaves room for fourfold growth (allowed = 1e-30 < 1100 eps): the fixed loop and the twin
    flag stage 0 for every start, and still complete on the schedule with the states tol = 1e-8 gives.  A start that overflows in
    stage 0 is flagged there or in the next stage (inf >= inf passes the test once, the NaN that follows does not)."""
    from hjbdp.rollout import position_optimal_path_fixed, position_rkf45_table
    sp = synthetic_sp
    ch = _twin_channels(sp)
    rng = np.random.default_rng(20)
    n, K = 8, 12
    tab = position_rkf45_table(K, sp.h, *sp.get_target_R0V0())
    X0 = np.concatenate([rng.uniform(-0.6, 0.6, size=(3, n)), rng.uniform(-0.3, 0.3, size=(3, n))])
    Xf, Xp, Ap, off = pr.rollout(ch, tab[0], tab[1], 1e-30, X0, np.zeros(K, int))
    Xf8, Xp8, Ap8, off8 = pr.rollout(ch, tab[0], tab[1], 1e-8, X0, np.zeros(K, int))
    assert (off == 0).all() and (off8 == -1).all() and _bits(Xp, Xp8) and _bits(Ap, Ap8)
    for i in range(n):
        T, X, F, off1 = position_optimal_path_fixed(sp, y0=X0[:, i], n_steps=K, tol=1e-30, table=tab)
        assert off1 == 0 and _bits(Xp[i], X) and _bits(Ap[i], F[:, :K]), i
    Xbig = X0[:, :1].copy()
    Xbig[0, 0] = Xbig[3, 0] = 1.7e308                             # x + h v overflows in the first stage
    with np.errstate(all="ignore"):
        Xf, Xp, Ap, off = pr.rollout(ch, tab[0], tab[1], 1e-8, Xbig, np.zeros(K, int))
        T, X, F, off1 = position_optimal_path_fixed(sp, y0=Xbig[:, 0], n_steps=K, table=tab)
    assert 0 <= off[0] <= 1 and off1 == off[0] and not np.isfinite(Xf[:, 0]).all() and not np.isfinite(X[:, 1]).all()
    nan = np.isnan(X)
    assert np.array_equal(nan, np.isnan(Xp[0])) and np.array_equal(X[~nan], Xp[0][~nan])


def test_python_entry_point_without_simplified_run():
    import hjbdp
    from hjbdp.rollout import position_optimal_path_fixed
    sp = hjbdp.Solver_position()
    with pytest.raises(RuntimeError, match=r"simplified_run\(\) first"):
        sp.get_optimal_paths(np.zeros((6, 2)))
    with pytest.raises(RuntimeError, match=r"simplified_run\(\) first"):
        position_optimal_path_fixed(sp)


def test_position_prototypes_are_identical_in_both_headers_and_bound(built):
    import hjbdp
    from hjbdp import _abi
    from test_abi import _prototypes
    lib = hjbdp.load_library()
    full = _prototypes((ROOT / "include" / "hjbdp.h").read_text())
    flat = _prototypes((ROOT / "include" / "hjbdp_matlab.h").read_text())
    for name in NEW_FNS:
        assert name in full and name in flat and full[name] == flat[name], name
        assert name in _abi.SYMBOLS and hasattr(lib, name), name
        assert len(_abi.SYMBOLS[name][1]) == len(full[name]), name
    assert full["hjb_rollout_set_position_model"] == ["void*", "void*", "void*", "double", "int32_t", "int32_t", "int32_t*", "double*"]
    assert full["hjb_rollout_run_position"] == ["void*", "int32_t", "int32_t*", "int64_t", "double*", "double*", "double*", "double*",
                                                "int32_t*"]


def test_position_refusals_without_a_device(built):
    """NULL objects are statuses, and every refusal that depends on the arguments alone (NULL n_sub or table, tol not finite or
    <= 0, no stages, max_sub outside 1..8, n_sub outside 1..max_sub, a non-finite table) is decided before an object is looked at,
    so without a device; the refusals that need an object are in tests/test_gpu_rollout_position.py."""
    import hjbdp
    from hjbdp import _abi
    lib = hjbdp.load_library()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))

    def call(tol=1e-8, n_steps=3, max_sub=5, n_sub=(5, 5, 5), table=None, null=()):
        n_sub = np.ascontiguousarray(n_sub, dtype=np.int32)
        table = np.ones((max(n_steps, 1), max(max_sub, 1), 32)) if table is None else np.ascontiguousarray(table, dtype=np.float64)
        st = lib.hjb_rollout_set_position_model(None, None, None, tol, n_steps, max_sub, None if "n_sub" in null else pi(n_sub),
                                                None if "table" in null else pd(table))
        return st, lib.hjb_rollout_last_error(None).decode()

    st, msg = call()
    assert st == _abi.HJB_E_INVALID and "null handle" in msg, msg
    for null in ("n_sub", "table"):
        st, msg = call(null=(null,))
        assert st == _abi.HJB_E_INVALID and "null argument" in msg, msg
    bad = np.ones((3, 5, 32))
    bad[1, 2, 7] = np.nan
    inf = np.ones((3, 5, 32))
    inf[2, 4, 31] = -np.inf
    for kw, needle in ((dict(tol=0.0), "tol"), (dict(tol=-1e-8), "tol"), (dict(tol=np.nan), "tol"), (dict(tol=np.inf), "tol"),
                       (dict(n_steps=0), "n_steps"), (dict(n_steps=-3), "n_steps"), (dict(max_sub=0), "max_sub"), (dict(max_sub=9), "max_sub"),
                       (dict(n_sub=(5, 0, 5)), "n_sub[1] = 0"), (dict(n_sub=(5, 5, 6)), "n_sub[2] = 6"), (dict(n_sub=(-1, 5, 5)), "n_sub[0] = -1"),
                       (dict(table=bad), "table element %d is not finite" % (32 * (5 * 1 + 2) + 7)),
                       (dict(table=inf), "table element %d is not finite" % (32 * (5 * 2 + 4) + 31))):
        st, msg = call(**kw)
        assert st == _abi.HJB_E_INVALID and needle in msg, (kw, msg)
    st, msg = call(max_sub=8, n_sub=(8, 1, 3))                       # the limits themselves hold: only the objects are missing
    assert st == _abi.HJB_E_INVALID and "null handle" in msg, msg
    X = np.zeros(6)
    off = np.zeros(1, np.int32)
    assert lib.hjb_rollout_run_position(None, 0, None, 1, pd(X), pd(X), None, None, pi(off)) == _abi.HJB_E_INVALID
    assert b"null" in lib.hjb_rollout_last_error(None)


def test_position_kernel_register_budget(tmp_path):
    """every K19 instantiation (label types u8 / u16 / i32, tables in LDS or in global memory) compiled for gfx950: no VGPR spill,
    no private segment and no scratch or buffer access in any of the six, with the 36 stage derivatives in registers.  The VGPR
    count is capped at 168, which on gfx950's 512-entry file is 3 waves per SIMD.  The table rows are read through the scalar
    cache (they are the same for the whole wave): four 16-dword scalar loads per sub-step."""
    import __graft_entry__ as g
    asm = tmp_path / "pos.s"
    r = subprocess.run([HIPCC, *g.HIPCC_FLAGS, "-S", "--cuda-device-only", "-o", str(asm), str(CSRC / "rollout_position.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = asm.read_text()
    got = re.findall(r"\.name:\s+(_ZN3hjb18k_rollout_position\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                     r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(got) == 6, [k[0] for k in got]
    for name, scratch, vgprs, spills in got:
        print(name, "vgprs", vgprs, "private segment", scratch, "vgpr spills", spills)
        assert int(spills) == 0 and int(scratch) == 0, (name, scratch, vgprs, spills)
        assert 72 < int(vgprs) <= 168, (name, vgprs)                  # more than the 36 doubles; 3 waves per SIMD
    bodies = re.findall(r"^(_ZN3hjb18k_rollout_position\S*):.*\n((?:.*\n)*?)\s+s_endpgm", text, flags=re.M)
    assert len(bodies) == 6
    for name, body in bodies:
        assert not re.search(r"\b(scratch_|buffer_(load|store))", body), name
        assert len(re.findall(r"\bs_load_dwordx16\b", body)) >= 4, name
