"""CPU tests of the paired campaign's difference record (include/hjbdp.h "paired campaigns", csrc/hjbdp_campaign.h
campaign_pair_start; no GPU): the host reduce hjbdp.campaign_pair_reduce against the numpy restatement
(tests/campaign_pair_refs.py) bit for bit at every block shape, with exact ties, a NaN, +inf on both sides and left flags on one
side, on both and on neither; the plain C++ harness over the same header; the antisymmetry of the record under a swap of the
sides, with no tolerance; the derived statistics; the refusals of the host reduce."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import campaign_pair_refs as refs

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SIZES = (1, 2, 3, 5, 63, 64, 65, 200)
STARTS = (1, 3, 70)


@pytest.fixture(scope="module")
def hjbdp(built):
    import hjbdp
    return hjbdp


def _inputs(M, ns, seed):
    """seeded costs of two controllers with what the contract singles out: exact ties, a NaN on one side, +inf on both sides
    (inf - inf), +inf on one side, and left flags on one side only, on both sides and on neither"""
    rng = np.random.default_rng(seed)
    ca = rng.uniform(0.0, 50.0, size=(ns, M)) * 10.0 ** rng.integers(-3, 4, size=(ns, M))
    cb = ca + rng.normal(size=(ns, M)) * 10.0 ** rng.integers(-6, 2, size=(ns, M))
    tie = rng.random((ns, M)) < 0.25
    cb[tie] = ca[tie]
    la, lb = rng.random((ns, M)) < 0.3, rng.random((ns, M)) < 0.3
    la[0, 0], lb[0, 0] = True, True
    if M > 1:
        la[0, 1], lb[0, 1] = True, False
        cb[-1, 0] = np.nan                                                      # slot 0 of block 0: the earlier operand at every level
        ca[ns // 2, M - 1] = np.inf                                             # inf - inf in the last live slot
        cb[ns // 2, M - 1] = np.inf
    if M > 2:
        la[0, 2], lb[0, 2] = False, True
        cb[0, M // 2] = np.inf                                                  # +inf on B's side alone
    if M > 4:
        la[0, 3], lb[0, 3] = False, False
        ca[0, 4] = np.inf                                                       # ... and on A's side alone: the start's sum is inf - inf
    return ca.reshape(-1), cb.reshape(-1), la.reshape(-1).astype(np.uint8), lb.reshape(-1).astype(np.uint8)


@pytest.mark.parametrize("ns", STARTS)
@pytest.mark.parametrize("M", SIZES)
def test_the_host_reduce_is_the_restatement_bit_for_bit(hjbdp, M, ns):
    ca, cb, la, lb = _inputs(M, ns, 100 * M + ns)
    want = refs.pair_reduce(ca, cb, M, la, lb)
    got = hjbdp.campaign_pair_reduce(ca, cb, M, left_a=la, left_b=lb)
    assert got["stats_d"].shape == (ns, 8)
    assert refs.same_bits(got["stats_d"], want), (M, ns)
    # left flags on neither side (null arrays): every sample counts as both-in
    got0 = hjbdp.campaign_pair_reduce(ca, cb, M)
    assert refs.same_bits(got0["stats_d"], refs.pair_reduce(ca, cb, M)) and np.all(got0["n_both_in"] == M)
    # ... and on one side only
    got1 = hjbdp.campaign_pair_reduce(ca, cb, M, left_b=lb)
    assert refs.same_bits(got1["stats_d"], refs.pair_reduce(ca, cb, M, None, lb))
    # the inputs hold what they are meant to hold
    with np.errstate(invalid="ignore"):
        d = cb.reshape(ns, M) - ca.reshape(ns, M)
    assert np.array_equal(got["n_b_lower"], np.count_nonzero(d < 0, axis=1)) and np.array_equal(got["n_a_lower"], np.count_nonzero(d > 0, axis=1))
    both = (la == 0) & (lb == 0)
    assert np.array_equal(got["n_both_in"], np.count_nonzero(both.reshape(ns, M), axis=1))
    assert np.array_equal(got["n_tie"], M - got["n_b_lower"] - got["n_a_lower"])
    if M > 4:
        assert got["n_tie"].sum() > 0 and np.isnan(got["stats_d"][-1, 0]) and np.isnan(got["stats_d"][ns // 2, 0])
        assert 0 < got["n_both_in"][0] < M


@pytest.mark.parametrize("M", SIZES)
def test_swapping_the_sides_gives_the_antisymmetric_record(hjbdp, M):
    """d -> -d exactly (a rounded subtraction is odd), and every op of the reduction commutes with the negation: no tolerance"""
    ca, cb, la, lb = _inputs(M, 3, 7 * M)
    fwd = hjbdp.campaign_pair_reduce(ca, cb, M, left_a=la, left_b=lb)["stats_d"]
    rev = hjbdp.campaign_pair_reduce(cb, ca, M, left_a=lb, left_b=la)["stats_d"]
    assert refs.same_values(rev, refs.swap_of(fwd)), (M, fwd, rev)
    assert refs.same_values(refs.pair_reduce(cb, ca, M, lb, la), refs.swap_of(refs.pair_reduce(ca, cb, M, la, lb)))


def test_the_derived_statistics(hjbdp):
    rng = np.random.default_rng(3)
    M, ns = 40, 5
    ca = rng.uniform(1.0, 2.0, size=(ns, M))
    cb = ca + rng.normal(0.01, 0.05, size=(ns, M))
    cb[0] = ca[0]                                                               # a start of ties: se = 0, t = 0 / 0
    la = np.zeros((ns, M), dtype=np.uint8)
    la[1] = 1                                                                   # a start with no sample both-in
    out = hjbdp.campaign_pair_reduce(ca, cb, M, left_a=la)
    d = cb - ca
    st = out["stats_d"]
    assert np.array_equal(out["mean_diff"], st[:, 0] / M) and np.allclose(out["mean_diff"], d.mean(axis=1), rtol=1e-12, atol=1e-15)
    assert np.allclose(out["var_diff"], d.var(axis=1, ddof=1), rtol=1e-9, atol=0) and np.all(out["var_diff"] >= 0)
    assert np.array_equal(out["std_diff"], np.sqrt(out["var_diff"])) and np.array_equal(out["se_diff"], np.sqrt(out["var_diff"] / M))
    with np.errstate(invalid="ignore", divide="ignore"):
        assert refs.same_values(out["t"], out["mean_diff"] / out["se_diff"])
    assert np.isnan(out["t"][0]) and out["n_tie"][0] == M and out["min_diff"][0] == 0 and out["max_diff"][0] == 0
    assert np.isnan(out["mean_diff_both_in"][1]) and out["n_both_in"][1] == 0
    assert np.allclose(out["mean_diff_both_in"][2:], d[2:].mean(axis=1), rtol=1e-12, atol=1e-15)
    assert np.array_equal(out["min_diff"], d.min(axis=1)) and np.array_equal(out["max_diff"], d.max(axis=1))
    # a and b are campaign_reduce's dicts of the two cost arrays
    assert np.array_equal(out["a"]["stats"], hjbdp.campaign_reduce(ca, M, left=la)["stats"])
    assert np.array_equal(out["b"]["stats"], hjbdp.campaign_reduce(cb, M)["stats"]) and out["device_ms"] == 0.0
    one = hjbdp.campaign_pair_reduce([1.0, 2.0], [1.5, 1.0], 1)
    assert not one["var_diff"].any() and not one["se_diff"].any() and one["mean_diff"].tolist() == [0.5, -1.0]
    assert "NaN difference" in " ".join(hjbdp.campaign_pair_reduce.__doc__.split())


def test_plain_cpp_harness_agrees_with_the_restatement(tmp_path):
    exe = tmp_path / "campaign_pair_harness"
    r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off",
                        "-I%s/optimal-control-dynamic-programming_amd/csrc" % ROOT, "-o", str(exe), "%s/tests/campaign_pair_harness.cpp" % ROOT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert [ln for ln in lines if not ln.startswith("stats ")] == ["diff: ok", "flags: ok"], lines
    rows = [ln.split() for ln in lines if ln.startswith("stats ")]
    assert [(int(r[1]), int(r[2])) for r in rows] == [(M, s) for M in SIZES for s in range(3)]
    for row in rows:
        M, s = int(row[1]), int(row[2])
        want = refs.pair_reduce(*refs.harness_inputs(s, M)[:2], M, *refs.harness_inputs(s, M)[2:])[0]
        got = np.array([int(w, 16) for w in row[3:]], dtype=np.uint64).view(np.float64)
        assert refs.same_bits(got, want), (M, s, got, want)
    assert any(float(np.array([int(r[7], 16)], dtype=np.uint64).view(np.float64)[0]) > 0 for r in rows)      # some ties, some wins


def test_refusals(hjbdp):
    lib = hjbdp.load_library()
    f64 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ca, cb = np.array([1.0, 2.0]), np.array([2.0, 1.0])

    def call(n_starts=1, n_samples=2, a=ca, b=cb, out="own"):
        o = np.full(8, -7.25)
        return lib.hjb_rollout_campaign_pair_reduce(n_starts, n_samples, f64(a), f64(b), None, None, None if out is None else f64(o)), o

    st, o = call()
    assert st == 0 and o.tolist() == [0.0, 2.0, -1.0, 1.0, 1.0, 1.0, 2.0, 0.0]
    for kw in (dict(n_starts=-1), dict(n_samples=0), dict(n_samples=-3), dict(a=None), dict(b=None), dict(out=None),
               dict(n_starts=2 ** 40, n_samples=2 ** 40)):
        st, o = call(**kw)
        assert st != 0 and np.all(o == -7.25), kw
    st, o = call(n_starts=0)
    assert st == 0 and np.all(o == -7.25)                                       # n_starts = 0 is HJB_OK and writes nothing
    with pytest.raises(ValueError):
        hjbdp.campaign_pair_reduce([1.0, 2.0], [1.0], 1)
    with pytest.raises(ValueError):
        hjbdp.campaign_pair_reduce([1.0, 2.0, 3.0], [1.0, 2.0, 3.0], 2)
    with pytest.raises(ValueError):
        hjbdp.campaign_pair_reduce([1.0, 2.0], [1.0, 2.0], 1, left_a=[1])
