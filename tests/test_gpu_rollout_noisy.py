"""GPU tests of the noisy rollout (hjb_rollout_set_noise / hjb_rollout_run_noisy, csrc/kernels_rollout_noisy.h: K25;
hjbdp.Rollout.run_noisy, Dynamic_Solver.get_noisy_paths): bit-equality with tests/noisy_rollout_refs.py at every instantiation,
one zero node against K16, global streams, "promised equals paid" on the exactly posed lattice problem, validation and
concurrency with a device, and the built kernels' private segments."""
import ctypes as C
import re
import shutil
import subprocess
import threading

import numpy as np
import pytest

import noisy_rollout_refs as refs
from test_gpu_rollout import _diff, _random_problem, _same

pytestmark = pytest.mark.gpu


def _check_bits(out, ref):
    Xf, cost, Xp, Up, Wp = ref
    assert _same(out["X_final"], Xf), _diff(out["X_final"], Xf)
    assert _same(out["cost"], cost), _diff(out["cost"], cost)
    if out["X_path"] is not None:
        assert _same(out["X_path"], Xp), _diff(out["X_path"], Xp)
        assert _same(out["U_path"], Up), _diff(out["U_path"], Up)
        assert out["W_path"].dtype == np.int32 and np.array_equal(out["W_path"], Wp)


def _equal_runs(a, b, keys=("X_final", "cost", "X_path", "U_path", "W_path")):
    for key in keys:
        assert (a[key] is None and b[key] is None) or _same(a[key], b[key]), key


def _node_sets(rng, D):
    """(offsets [D, W], weights) for W = 1, 2 and 128.  From D = 2 on one axis of every set has all-zero offsets (stored with both
    signs of zero); at D = 1 the W = 1 set is the one whose only axis is not offset.  The W = 2 and W = 128 sets hold a
    zero-weight node, and the W = 128 offsets reach +-0.6, beyond the 0.1 the starts lie outside the grid by."""
    zero_axis = int(rng.integers(0, D))
    sets = []
    for W, amp in ((1, 0.05), (2, 0.2), (128, 0.6)):
        off = rng.uniform(-amp, amp, size=(D, W))
        if D > 1 or W == 1:
            off[zero_axis] = np.where(rng.integers(0, 2, size=W) == 0, 0.0, -0.0)
        if W == 1:
            p = None
        elif W == 2:
            p = np.array([1.0, 3.0]) if D % 2 else np.array([0.0, 2.0])
        else:
            p = rng.uniform(0.0, 1.0, size=W)
            p[[0, 77, 127]] = 0.0
        sets.append((off, p))
    return sets


# ---- 1. every instantiation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_every_instantiation_is_bit_equal_to_the_restatement(built, D, dtype):
    import hjbdp
    rng = np.random.default_rng(1000 + 100 * D + np.dtype(dtype).itemsize)
    left_grid = drew = 0
    for (off, p), nu in zip(_node_sets(rng, D), (1, 4, 2)):
        knots, labels, ut, base, A, B, c = _random_problem(rng, D, nu, dtype, 7, 3)
        lo = np.array([k[0] for k in knots])
        hi = np.array([k[-1] for k in knots])
        X0 = rng.uniform(lo[:, None] - 0.1, hi[:, None] + 0.1, size=(D, 300))      # two blocks, the second partial
        planes = rng.integers(0, 3, size=9)                                         # two Philox blocks and one word of a third
        q, r = rng.uniform(0, 1, size=D), rng.uniform(0, 1, size=nu)
        seed, first = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
        cc = c if nu == 4 else None
        with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
            ro.set_model(A, B, c=cc, q=q, r=r)
            ro.set_noise(off, p)
            for method in ("nearest", "linear"):
                ref = refs.rollout(knots, labels, ut, base, A, B, X0, planes, off, p, seed, first, method, c=cc, q=q, r=r)
                for lds in (1, 0):
                    ro.set_option("lds", lds)
                    out = ro.run_noisy(X0, planes, seed=seed, first_stream=first, method=method, keep_path=True)
                    _check_bits(out, ref)
                    lean = ro.run_noisy(X0, planes, seed=seed, first_stream=first, method=method)
                    assert lean["X_path"] is None and lean["W_path"] is None
                    _equal_runs(lean, out, ("X_final", "cost"))
                assert np.isfinite(ref[1]).mean() > 0.5     # (far outside the grid the 'linear' lookup extrapolates as a degree-D polynomial)
                Xp, Wp = ref[2], ref[4]
                left_grid += int(((Xp < lo[None, :, None]) | (Xp > hi[None, :, None])).any(axis=(1, 2)).sum())
                if p is not None:
                    assert not np.isin(Wp, np.flatnonzero(p == 0)).any()
                    drew += len(np.unique(Wp))
    assert left_grid > 0 and drew > 60              # trajectories did leave the grid, and the 128-node set was really sampled


# ---- 2. one zero node is K16 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_one_zero_node_is_k16_and_run_never_reads_the_noise(built, D):
    import hjbdp
    rng = np.random.default_rng(50 + D)
    knots, labels, ut, base, A, B, c = _random_problem(rng, D, 2, np.uint16, 9, 4)
    lo = np.array([k[0] for k in knots]) - 0.1
    hi = np.array([k[-1] for k in knots]) + 0.1
    X0 = rng.uniform(lo[:, None], hi[:, None], size=(D, 300))
    planes = rng.integers(0, 4, size=9)
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=np.ones(D), r=[0.5, 0.25])
        for method in ("linear", "nearest"):
            before = ro.run(X0, planes, method=method, keep_path=True)
            ro.set_noise(np.zeros((D, 1)))
            noisy = ro.run_noisy(X0, planes, seed=99, first_stream=5, method=method, keep_path=True)
            _equal_runs(noisy, before, ("X_final", "cost", "X_path", "U_path"))
            assert not noisy["W_path"].any()
            ro.set_noise(rng.uniform(-0.5, 0.5, size=(D, 7)), rng.uniform(0.1, 1.0, size=7))
            during = ro.run(X0, planes, method=method, keep_path=True)
            moved = ro.run_noisy(X0, planes, seed=99, first_stream=5, method=method, keep_path=True)
            ro.clear_noise()
            after = ro.run(X0, planes, method=method, keep_path=True)
            _equal_runs(during, before, ("X_final", "cost", "X_path", "U_path"))
            _equal_runs(after, before, ("X_final", "cost", "X_path", "U_path"))
            assert not _same(moved["X_final"], before["X_final"])
            with pytest.raises(hjbdp.HjbError) as ei:
                ro.run_noisy(X0, planes)
            assert "hjb_rollout_set_noise" in str(ei.value)


# ---- 3. streams are global -------------------------------------------------------------------------------------------------------
def test_streams_count_through_the_call(built):
    import hjbdp
    rng = np.random.default_rng(8)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 2, 2, np.uint8, 12, 4)
    lo = np.array([k[0] for k in knots]) - 0.1
    hi = np.array([k[-1] for k in knots]) + 0.1
    X0 = rng.uniform(lo[:, None], hi[:, None], size=(2, 600))
    planes = rng.integers(0, 4, size=9)
    off, p = rng.uniform(-0.3, 0.3, size=(2, 9)), rng.uniform(0.1, 1.0, size=9)
    kw = dict(c=c, q=[1.0, 0.5], r=[0.1, 0.2])
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, **kw)
        ro.set_noise(off, p)
        whole = ro.run_noisy(X0, planes, seed=12, keep_path=True)
        _check_bits(whole, refs.rollout(knots, labels, ut, base, A, B, X0, planes, off, p, 12, 0, "linear", **kw))
        # chunks of 97 (six full ones and a rest of 18) against the one launch
        ro.set_option("chunk", 97)
        _equal_runs(ro.run_noisy(X0, planes, seed=12, keep_path=True), whole)
        ro.set_option("chunk", 1 << 20)
        # 600 at stream 0 = 300 at stream 0, then 300 at stream 300
        halves = [ro.run_noisy(X0[:, i:i + 300], planes, seed=12, first_stream=i, keep_path=True) for i in (0, 300)]
        for key in ("cost", "X_path", "U_path", "W_path"):
            assert _same(np.concatenate([h[key] for h in halves], axis=0), whole[key]), key
        assert _same(np.concatenate([h["X_final"] for h in halves], axis=1), whole["X_final"])
        # the stream's second counter word changes inside the call, in one launch and across chunks
        first = 2 ** 32 - 100
        ref = refs.rollout(knots, labels, ut, base, A, B, X0[:, :300], planes, off, p, 12, first, "linear", **kw)
        far = ro.run_noisy(X0[:, :300], planes, seed=12, first_stream=first, keep_path=True)
        _check_bits(far, ref)
        ro.set_option("chunk", 97)
        _check_bits(ro.run_noisy(X0[:, :300], planes, seed=12, first_stream=first, keep_path=True), ref)
        ro.set_option("chunk", 1 << 20)
        assert not np.array_equal(far["W_path"], whole["W_path"][:300])
        other = ro.run_noisy(X0, planes, seed=13, keep_path=True)
        assert not np.array_equal(other["W_path"], whole["W_path"])
        big_seed = ro.run_noisy(X0[:, :40], planes, seed=2 ** 64 - 1, keep_path=True)
        _check_bits(big_seed, refs.rollout(knots, labels, ut, base, A, B, X0[:, :40], planes, off, p, 2 ** 64 - 1, 0, "linear", **kw))


def test_node_block_that_pushes_the_tables_past_the_lds_limit(built):
    """[knots | 1/dx | u_table] of 4008 doubles fit 32 KiB alone; the 128-node block (127 + 128 doubles) does not fit behind them:
    the library runs the global-memory form - the bits of the forced one (option "lds" = 0) and of the restatement.  With 9 nodes
    (8 + 9 doubles: 4025 in all) the same object stays in LDS."""
    import hjbdp
    rng = np.random.default_rng(31)
    knots = [np.linspace(-1.0, 1.0, 4)]
    labels = rng.integers(0, 4000, size=(4, 2)).astype(np.int32)
    ut = rng.uniform(-1, 1, size=(4000, 1))
    X0 = rng.uniform(-1.1, 1.1, size=(1, 300))
    planes = [0, 1, 1, 0, 1]
    with hjbdp.Rollout(knots, labels, ut, index_base=0) as ro:
        ro.set_model([[0.5]], [[0.05]], q=[1.0], r=[1.0])
        for W in (128, 9):
            off, p = rng.uniform(-0.3, 0.3, size=(1, W)), rng.uniform(0.1, 1.0, size=W)
            ro.set_noise(off, p)
            ref = refs.rollout(knots, labels, ut, 0, [[0.5]], [[0.05]], X0, planes, off, p, 3, 0, "linear", q=[1.0], r=[1.0])
            out = ro.run_noisy(X0, planes, seed=3, keep_path=True)
            _check_bits(out, ref)
            ro.set_option("lds", 0)
            _equal_runs(ro.run_noisy(X0, planes, seed=3, keep_path=True), out)
            ro.set_option("lds", 1)


# ---- 4. promised equals paid -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice(built):
    """the lattice problem solved on the GPU under both modes: {mode: (J at stage 1 [33], labels [33, 6])}"""
    import hjbdp
    out = {}
    for mode in ("expect", "worst"):
        with hjbdp.Backup(refs.lattice_spec(mode)) as bk:
            sol = bk.solve(refs.LATTICE_STAGES, keep_J=True, keep_idx=True)
        out[mode] = (sol["J_stages"].reshape(33, refs.LATTICE_STAGES, order="F")[:, 0],
                     sol["idx_stages"].reshape(33, refs.LATTICE_STAGES, order="F"))
    return out


def _fly_lattice(labels, weights, n_samples, seed):
    import hjbdp
    X0 = np.repeat(refs.LATTICE_STARTS, n_samples).reshape(1, -1)               # sample j of start i on stream i * n_samples + j
    with hjbdp.Rollout([refs.LATTICE_KNOTS], labels, refs.LATTICE_U, index_base=0) as ro:
        ro.set_model([[1.0]], [[1.0]], q=[1.0], r=[0.5])
        ro.set_noise(refs.LATTICE_NODES, weights)
        out = ro.run_noisy(X0, np.arange(refs.LATTICE_STAGES), seed=seed)
    return out["cost"].reshape(refs.LATTICE_STARTS.size, n_samples)


def test_expected_cost_promised_is_the_cost_paid(lattice):
    J1, labels = lattice["expect"]
    starts = (refs.LATTICE_STARTS + 16).astype(np.int64)
    costs, prob = refs.lattice_enumeration(labels)
    mean = costs @ prob
    assert np.array_equal(mean, J1[starts])                                     # the promise is the exact expectation
    sigma = np.sqrt(((costs - mean[:, None]) ** 2) @ prob)                      # exact, from the 3^6 sequences: never from samples
    assert np.all(sigma > 0)
    n = 1 << 16
    paid = _fly_lattice(labels, refs.LATTICE_P, n, seed=2025)
    assert np.isin(paid, costs).all()
    err = np.abs(paid.mean(axis=1) - J1[starts])
    print("promised", J1[starts], "paid", paid.mean(axis=1), "err / (sigma / 2^8)", err / (sigma / 256.0))
    assert np.all(err <= 6.0 * sigma / 256.0), (err, sigma)


def test_worst_case_promised_is_the_worst_cost_paid(lattice):
    J1, labels = lattice["worst"]
    starts = (refs.LATTICE_STARTS + 16).astype(np.int64)
    costs, _ = refs.lattice_enumeration(labels)
    assert np.array_equal(costs.max(axis=1), J1[starts])
    paid = _fly_lattice(labels, None, 1 << 16, seed=2026)                       # uniform over the three nodes
    assert np.all(paid <= J1[starts][:, None])
    assert np.array_equal(paid.max(axis=1), J1[starts])


# ---- 5. validation with a device ---------------------------------------------------------------------------------------------------
def test_validation_with_a_device_and_two_threads(built):
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(77)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 3, 2, np.int32, 9, 5)
    X0 = rng.uniform(-1.0, 1.0, size=(3, 2000))
    planes = rng.integers(0, 5, size=9)
    off, p = rng.uniform(-0.2, 0.2, size=(3, 5)), rng.uniform(0.1, 1.0, size=5)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        lib, h = ro.lib, ro._ro
        err = lambda: lib.hjb_rollout_last_error(h).decode()
        with pytest.raises(hjbdp.HjbError) as ei:                               # no model yet (check_run)
            ro.run_noisy(X0, planes)
        assert ei.value.status == _abi.HJB_E_INVALID and "hjb_rollout_set_model" in str(ei.value)
        ro.set_model(A, B, c=c, q=[1, 1, 1])
        with pytest.raises(hjbdp.HjbError) as ei:                               # a model, no noise
            ro.run_noisy(X0, planes)
        assert ei.value.status == _abi.HJB_E_INVALID and "before hjb_rollout_set_noise" in str(ei.value)
        ro.set_noise(off, p)
        good = ro.run_noisy(X0, planes, seed=4, keep_path=True)
        offF = np.ascontiguousarray(off.reshape(-1, order="F"))
        bad_off = offF.copy()
        bad_off[3 * 2 + 1] = np.nan
        for args, text in (((-1, dp(offF), None), "n_nodes=-1"), ((129, dp(offF), None), "n_nodes=129"), ((5, None, None), "null offsets"),
                           ((5, dp(bad_off), None), "offset of axis 1, node 2 is not finite"),
                           ((5, dp(offF), dp([1, 1, np.inf, 1, 1])), "weight 2 is not finite or is negative"),
                           ((5, dp(offF), dp([1, -1, 1, 1, 1])), "weight 1 is not finite or is negative"),
                           ((5, dp(offF), dp([0, 0, 0, 0, 0])), "weights sum to 0")):
            assert lib.hjb_rollout_set_noise(h, *args) == _abi.HJB_E_INVALID and text in err(), (err(), text)
            # the node set is the one it was
            _equal_runs(ro.run_noisy(X0, planes, seed=4, keep_path=True), good)
        # run_noisy's refusals leave every output untouched
        Xc = np.ascontiguousarray(X0.T)
        ps = np.ascontiguousarray(planes, dtype=np.int32)
        pp = ps.ctypes.data_as(C.POINTER(C.c_int32))
        nt, K = X0.shape[1], len(ps)
        Xn = Xc.copy()
        Xn[17, 2] = np.inf
        far = np.array([0, 5] + [0] * (K - 2), dtype=np.int32)
        for call, text in ((dict(first=-1), "first_stream=-1 < 0"), (dict(first=2 ** 63 - 1000), "overflows"), (dict(method=7), "method 7"),
                           (dict(K=-1), "n_steps=-1"), (dict(pl=far.ctypes.data_as(C.POINTER(C.c_int32))), "plane_of_step[1] = 5"),
                           (dict(pl=None), "null plane_of_step"), (dict(X=dp(Xn)), "not finite"), (dict(X=None), "null X0")):
            outs = [np.full(m, 7.25) for m in (nt * 3, nt, nt * 3 * (K + 1), nt * 2 * K, nt * K)]
            ms = C.c_double(7.25)
            st = lib.hjb_rollout_run_noisy(h, call.get("method", 1), call.get("K", K), call.get("pl", pp), nt, call.get("X", dp(Xc)), 4,
                                           call.get("first", 0), *[dp(o) for o in outs], C.byref(ms))
            assert st == _abi.HJB_E_INVALID and text in err(), (call, err())
            assert all(np.all(o == 7.25) for o in outs) and ms.value == 7.25, call
        _equal_runs(ro.run_noisy(X0, planes, seed=4, keep_path=True), good)
        # two threads on the one object: the calls take turns
        par = [None, None]

        def work(t):
            for _ in range(3):
                par[t] = ro.run_noisy(X0, planes, seed=4 + t, first_stream=1000 * t, keep_path=True)
        ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        _equal_runs(par[0], good)
        _check_bits(par[1], refs.rollout(knots, labels, ut, base, A, B, X0, planes, off, p, 5, 1000, "linear", c=c, q=[1, 1, 1]))
    # a model other than the affine one
    k6, l6, u6, b6, _, _, _ = _random_problem(rng, 6, 3, np.uint8, 5, 2)
    with hjbdp.Rollout(k6, l6, u6, index_base=b6) as ro:
        ro.set_attitude_model([1.0, 2.0, 3.0], 0.01)
        ro.set_noise(np.full((6, 2), 0.01))
        with pytest.raises(hjbdp.HjbError) as ei:
            ro.run_noisy(np.zeros((6, 4)), [0, 1])
        assert ei.value.status == _abi.HJB_E_INVALID and "attitude model" in str(ei.value)


def test_dynamic_solver_get_noisy_paths(built):
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N, ds.dx, ds.du = 20, 35, 100
    off, w = hjbdp.gaussian_nodes([0.02, 0.05], order=3)
    ds.disturbance = (off, w, "expect")
    ds.run()
    X0s = np.array([[2.0, 0.5, -1.0], [1.0, -0.5, 0.25]])
    cost = ds.get_noisy_paths(X0s, 50, seed=6)
    assert cost.shape == (3, 50)
    assert ds.noisy_cost_mean.shape == ds.noisy_cost_std.shape == ds.noisy_cost_max.shape == (3,)
    assert np.array_equal(ds.noisy_cost_mean, cost.mean(axis=1)) and np.array_equal(ds.noisy_cost_max, cost.max(axis=1))
    assert np.all(ds.noisy_cost_std > 0)
    s_r = np.asarray(ds.s_r, dtype=np.float64)
    ut = np.asarray(ds._U_mesh, dtype=np.float64)
    with hjbdp.Rollout([s_r, s_r], ds.u_star_idxs, ut, index_base=1) as ro:
        ro.set_model(ds.A, ds.B, q=np.diag(ds.Q), r=[ds.R])
        ro.set_noise(off, w)
        for i in range(3):                                                      # sample j of start i on stream i * n_samples + j
            by_hand = ro.run_noisy(np.repeat(X0s[:, i:i + 1], 50, axis=1), np.arange(19), seed=6, first_stream=50 * i)
            assert _same(by_hand["cost"], cost[i])
    frozen = ds.get_noisy_paths(X0s, 50, seed=6, mode="ssu", ssu_num=3)
    assert frozen.shape == (3, 50) and not np.array_equal(frozen, cost)
    ds.disturbance = (off, None, "worst")                                       # a 'worst' set is sampled uniformly
    uniform = ds.get_noisy_paths(X0s, 50, seed=6)
    assert uniform.shape == (3, 50) and not np.array_equal(uniform, cost)
    ds.disturbance = None
    with pytest.raises(RuntimeError):
        ds.get_noisy_paths(X0s, 5)


# ---- 6. no scratch -----------------------------------------------------------------------------------------------------------------
def test_no_scratch_in_the_built_kernels(built, tmp_path):
    """Read from the code objects inside the built library (llvm-objdump --offloading, llvm-readelf --notes): the 72
    k_rollout_noisy instantiations (label type x method x LDS x D) exist and none has a private segment."""
    tools = "/opt/rocm/lib/llvm/bin"
    objdump = shutil.which("llvm-objdump", path=tools) or shutil.which("llvm-objdump")
    readelf = shutil.which("llvm-readelf", path=tools) or shutil.which("llvm-readelf")
    assert objdump and readelf, "llvm-objdump / llvm-readelf of the ROCm toolchain not found"
    lib = tmp_path / "libhjbdp.so"
    shutil.copy(built.LIB, lib)
    r = subprocess.run([objdump, "--offloading", lib.name], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    for co in sorted(tmp_path.glob("libhjbdp.so.*gfx950*")):
        notes = subprocess.run([readelf, "--notes", co.name], cwd=tmp_path, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:                           # one block per kernel of the code object
            m = re.search(r"\.name:\s+(_ZN3hjb15k_rollout_noisyI\S*)", blk)
            if m:
                found[m.group(1)] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                                     int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)))
    forms = {re.match(r"_ZN3hjb15k_rollout_noisyILi(\d)E(\w)Li([01])ELb([01])E", n).groups() for n in found}
    assert len(found) == 72 and forms == {(str(d), t, m, l) for d in range(1, 7) for t in "hti" for m in "01" for l in "01"}, len(found)
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
