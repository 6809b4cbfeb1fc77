"""CPU tests of the fixed-label stage's interface (hjb_evaluate_stage, hjb_evaluate_stage_device, hjb_evaluate): the symbols and
their prototypes in both headers, the refusals that need no device, the Python mirror's checks, the MATLAB shim's calls, and the
reference helper the GPU tests compare with (tests/evaluate_refs.py), itself held to the two oracles."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
EVAL_FNS = ("hjb_evaluate_stage", "hjb_evaluate_stage_device", "hjb_evaluate")


@pytest.fixture(scope="module")
def lib(built):
    import hjbdp
    return hjbdp.load_library()


def test_evaluate_symbols_and_prototypes(lib):
    from hjbdp import _abi
    from test_abi import _prototypes
    full = _prototypes((ROOT / "include" / "hjbdp.h").read_text())
    flat = _prototypes((ROOT / "include" / "hjbdp_matlab.h").read_text())
    for name in EVAL_FNS:
        assert name in _abi.SYMBOLS, name
        assert hasattr(lib, name), name
        assert name in full and name in flat, name
        assert full[name] == flat[name], (name, full[name], flat[name])
        assert len(_abi.SYMBOLS[name][1]) == len(full[name]), name
    assert len(full["hjb_evaluate_stage"]) == 4 and len(full["hjb_evaluate_stage_device"]) == 5 and len(full["hjb_evaluate"]) == 8


def test_null_arguments_are_invalid_without_a_device(lib):
    from hjbdp import _abi
    buf = np.zeros(8, dtype=np.float64)
    p = buf.ctypes.data
    # null handle (nothing else can be looked at)
    assert lib.hjb_evaluate_stage(None, p, p, p) == _abi.HJB_E_INVALID
    assert b"null" in lib.hjb_last_error(None)
    assert lib.hjb_evaluate_stage_device(None, p, p, p, None) == _abi.HJB_E_INVALID
    assert lib.hjb_evaluate(None, 3, None, p, 0, p, None, None) == _abi.HJB_E_INVALID
    # ... whatever else is null too (a live handle's null-pointer refusals need a device: tests/test_gpu_evaluate.py)
    assert lib.hjb_evaluate_stage(None, None, None, None) == _abi.HJB_E_INVALID
    assert lib.hjb_evaluate(None, 0, None, None, 7, None, None, None) == _abi.HJB_E_INVALID
    assert hjbdp_status_text(lib, _abi.HJB_E_INVALID) == "invalid argument"


def hjbdp_status_text(lib, st):
    return lib.hjb_status_string(st).decode()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def test_backup_evaluate_checks_labels_before_any_library_call():
    import hjbdp
    from problems import random_problem
    spec = random_problem(3, (4, 5), (3, 2), dtype=np.float32, index_base=1)
    bk = hjbdp.Backup.__new__(hjbdp.Backup)       # no device here: the checks under test need none
    bk.spec, bk.lib, bk._h = spec, _NoLibrary(), C.c_void_p()
    nS = spec.nS
    assert spec.idx_np_dtype == np.int32
    for bad in [np.ones(nS, dtype=np.int64), np.ones(nS, dtype=np.uint8), np.ones(nS, dtype=np.float32)]:
        with pytest.raises(ValueError, match="idx_np_dtype"):
            bk.evaluate(4, bad)
    for bad in [np.ones(nS - 1, dtype=np.int32), np.ones((nS, 3), dtype=np.int32), np.ones((4, 5), dtype=np.int32),
                np.ones((nS, 4, 1), dtype=np.int32), np.ones((4, nS), dtype=np.int32)]:
        with pytest.raises(ValueError, match="shape"):
            bk.evaluate(4, bad)
    with pytest.raises(ValueError, match="terminal"):
        bk.evaluate(4, np.ones(nS, dtype=np.int32), terminal=np.zeros(nS + 1))
    # well-formed arguments reach the library
    for good in [np.ones(nS, dtype=np.int32), np.ones((nS, 4), dtype=np.int32)]:
        with pytest.raises(AssertionError, match="hjb_evaluate"):
            bk.evaluate(4, good)
    u8 = hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, dtype=np.float32, index_base=1, idx_dtype="auto")
    bk.spec = u8
    with pytest.raises(ValueError, match="idx_np_dtype"):
        bk.evaluate(4, np.ones(nS, dtype=np.int32))
    bk._h = None      # (nothing for __del__ to destroy)


def test_matlab_shim_calls_only_declared_flat_entry_points():
    from test_abi import _matlab_calllibs, _prototypes
    flat = _prototypes((ROOT / "include" / "hjbdp_matlab.h").read_text())
    text = (ROOT / "optimal-control-dynamic-programming_amd" / "matlab" / "hjbdp_evaluate.m").read_text()
    calls = _matlab_calllibs(text)
    names = {c[0] for c in calls}
    assert "hjb_evaluate" in names and "hjb_create_from" in names and "hjb_destroy" in names
    for name, nargs in calls:
        assert name in flat, name
        assert nargs == len(flat[name]), (name, nargs, len(flat[name]))


CASES = [((7,), (5,)), ((6, 5), (3, 4)), ((5, 4, 3), (3, 4, 2)), ((4, 3, 4, 3), (4,))]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,m", CASES)
def test_evaluate_ref_reproduces_both_oracles_on_their_own_labels(built, n, m, dtype):
    """lerp='oracle' on the numpy oracle's labels = the numpy oracle's J; lerp='fma' on the C twin's labels = the C twin's J -
    bit for bit.  Unequal control sizes: a transposed label decode would gather another control's value."""
    from hjbdp import _abi
    from oracle import c_oracle, hjb_oracle
    from evaluate_refs import evaluate_ref, oracle_problem
    from problems import random_problem, random_terminal
    spec = random_problem(40 + len(n) + 7 * len(m), n, m, dtype=dtype, nonuniform=len(n) % 2 == 0, index_base=1)
    term = random_terminal(spec, 5)
    p = oracle_problem(spec)
    Jn, labn = hjb_oracle.backup_stage(p, term.reshape(n, order="F"))
    got = evaluate_ref(p, term, labn)
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, Jn)
    Jc, labc = c_oracle.backup_stage(_abi, spec, term)
    got = evaluate_ref(p, term, labc - spec.index_base, lerp="fma")
    assert got.dtype == np.dtype(dtype) and np.array_equal(got.reshape(-1, order="F"), Jc)
    if len(m) > 1:        # the decode matters: the row-major reading of the same labels gives other values
        sub = np.unravel_index(labn, m, order="F")
        swapped = np.ravel_multi_index(sub, m, order="C")
        assert not np.array_equal(evaluate_ref(p, term, swapped), Jn)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,m", CASES)
def test_evaluate_ref_states_is_the_whole_grid_reference_state_by_state(built, n, m, dtype):
    """evaluate_ref_states over every state = evaluate_ref(lerp='fma') bit for bit, on seeded random labels, in a shuffled state
    order and on a subset; on the C twin's own labels = the C twin's J; and with J_next behind separable_jnext = the same with the
    separable array (float32 arithmetic, float32 and binary16 storage: what fill_separable leaves on the device)."""
    from hjbdp import _abi
    from oracle import c_oracle
    from evaluate_refs import evaluate_ref, evaluate_ref_states, oracle_problem, separable_jnext
    from float64_refs import separable_ref
    from problems import random_problem, random_terminal
    spec = random_problem(40 + len(n) + 7 * len(m), n, m, dtype=dtype, nonuniform=len(n) % 2 == 0, index_base=1)
    term = random_terminal(spec, 5)
    p = oracle_problem(spec)
    rng = np.random.default_rng(12)
    lab = rng.integers(0, spec.nU, spec.nS)
    Jn = term.reshape(n, order="F")
    whole = evaluate_ref(p, term, lab, lerp="fma").reshape(-1, order="F")
    states = np.arange(spec.nS)
    got = evaluate_ref_states(p, states, lab, lambda idx: Jn[idx])
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, whole)
    sel = rng.permutation(spec.nS)[:max(3, spec.nS // 3)]
    assert np.array_equal(evaluate_ref_states(p, sel, lab[sel], lambda idx: Jn[idx]), whole[sel])
    Jc, labc = c_oracle.backup_stage(_abi, spec, term)
    assert np.array_equal(evaluate_ref_states(p, states, labc - spec.index_base, lambda idx: Jn[idx]), Jc)
    if dtype == np.float32:
        vecs = [rng.random(k).astype(np.float32) * (1.0 + a) for a, k in enumerate(n)]
        for storage in (np.float32, np.float16):
            sep = separable_ref(vecs, np.float32, storage).astype(np.float32)
            want = evaluate_ref(p, sep, lab, lerp="fma").reshape(-1, order="F")
            assert np.array_equal(evaluate_ref_states(p, states, lab, separable_jnext(vecs, np.float32, storage)), want)
            assert not np.array_equal(want, whole)


def test_fma32_repairs_a_double_rounding():
    """(1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is exactly a float32 midpoint; adding 2^-60 is lost in float64, and rounding that sum
    to float32 ties to even (1 + 2^-11), while the exact value lies above the midpoint."""
    from evaluate_refs import _fma32
    t = np.array([1.0 + 2.0 ** -12], dtype=np.float32)
    lo = np.float32(1.0 + 2.0 ** -11)
    hi = np.nextafter(lo, np.float32(2.0))
    for c, want in [(2.0 ** -60, hi), (-2.0 ** -60, lo), (0.0, lo)]:
        v0 = np.array([c], dtype=np.float32)
        s = np.float64(t[0]) * np.float64(t[0]) + np.float64(v0[0])
        assert s == 1.0 + 2.0 ** -11 + 2.0 ** -24 and np.float32(s) == lo          # what one more rounding would give
        assert _fma32(t, t, v0)[0] == want, c


def test_division_by_multiplication_is_exact(tmp_path):
    """csrc/hjbdp_walk.h magic_div / magic_quot (the evaluation kernel's 32-bit form divides by them) against `/` on the host:
    every divisor up to 5000, the neighbourhood of every power of two up to 2^31, a few large ones; numerators around the multiples
    of the divisor, the ends of the range and a seeded sample."""
    import shutil
    import subprocess
    import __graft_entry__ as g
    cxx = g._hipcc() if shutil.which(g._hipcc()) or Path(g._hipcc()).exists() else "c++"
    exe = tmp_path / "magicdiv_harness"
    r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror",
                        "-I%s/optimal-control-dynamic-programming_amd/csrc" % ROOT, "-o", str(exe), "%s/tests/magicdiv_harness.cpp" % ROOT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 wrong" in r.stdout, r.stdout[-2000:]
