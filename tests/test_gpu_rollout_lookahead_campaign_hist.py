"""GPU tests of the lookahead campaign's histogram (hjb_rollout_run_lookahead_campaign_hist,
csrc/kernels_rollout_lookahead_campaign_hist.h: K30; hjbdp.Rollout.run_lookahead_campaign_hist,
Dynamic_Solver.get_lookahead_cost_quantiles).  The anchor is code older than the histogram: run_lookahead(noisy=True) (K27) for the
costs, hjbdp.campaign_hist_reduce (the host twin of the bin rule, checked without a device) for the counts, and
run_lookahead_campaign (K29) for the statistics, compared as bits: at the 24 instantiations under both "lds" settings, under
chunking, on the exactly posed lattice against the label campaign's histogram, and through Dynamic_Solver."""
import numpy as np
import pytest

import campaign_hist_refs as hrefs
import lookahead_campaign_refs as lc
import noisy_rollout_refs as nrefs
from lookahead_campaign_refs import bits
from test_gpu_rollout_lookahead_campaign import DS_NODES, DS_U_RANGE, DS_WEIGHTS, _open

pytestmark = pytest.mark.gpu

PLANES = [1, -1, 0, 2]                       # few steps: -1 inside


def _costs(ro, X0, M, planes, seed, first):
    return ro.run_lookahead(np.repeat(X0, M, axis=1), planes, noisy=True, seed=seed, first_stream=first)["cost"]


def _check(ro, X0, M, planes, seed, first, lo, hi, n_bins, cost):
    import hjbdp
    plain = ro.run_lookahead_campaign(X0, planes, M, seed=seed, first_stream=first, cost_threshold=0.5, settle_tol=0.3)
    got = ro.run_lookahead_campaign_hist(X0, planes, M, (lo, hi, n_bins), seed=seed, first_stream=first, cost_threshold=0.5, settle_tol=0.3)
    want = hjbdp.campaign_hist_reduce(cost, M, lo, hi, n_bins)
    assert got["hist"].shape == (X0.shape[1], n_bins + 2) and np.array_equal(got["hist"], want), (got["hist"], want)
    assert np.all(got["hist"].sum(axis=1) == M)
    assert np.array_equal(bits(got["stats"]), bits(plain["stats"]))
    return got


# ---- 1. every instantiation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_every_instantiation_counts_what_the_host_reduce_counts(built, D, dtype):
    pb = lc.problem(D, dtype, n_starts=2)
    M, n_bins = 3, 4
    X0, seed, first = pb["X0"], pb["seed"], pb["first"]
    with _open(pb) as ro:
        cost = _costs(ro, X0, M, PLANES, seed, first)
        lo, hi = hrefs.exact_range(cost, M)
        hi = np.where(cost.reshape(2, M).min(axis=1) < cost.reshape(2, M).max(axis=1), hi, lo + 1.0)
        for lds in (1, 0):
            ro.set_option("lds", lds)
            got = _check(ro, X0, M, PLANES, seed, first, lo, hi, n_bins, cost)
            assert not got["hist"][:, 0].any() and not got["hist"][:, -1].any()
            mid = float(np.median(cost))                                        # one scalar range: samples under, inside and over
            _check(ro, X0, M, PLANES, seed, first, mid - 1e-3, mid + 1e-3, n_bins, cost)


# ---- 2. chunking and the wave form --------------------------------------------------------------------------------------------------
def test_chunks_change_no_count(built):
    """3 starts x 200 samples: 12 blocks of 64 lanes, the histogram per wave in LDS; launches of one block, of three (a start's four
    blocks across launches) and of all"""
    pb = lc.problem(2, np.float32, n_starts=3)
    M, first, n_bins = 200, 300, 16
    X0 = pb["X0"]
    with _open(pb) as ro:
        cost = _costs(ro, X0, M, lc.PLANES, 12, first)
        lo, hi = hrefs.exact_range(cost, M)
        whole = _check(ro, X0, M, lc.PLANES, 12, first, lo, hi, n_bins, cost)
        for chunk in (1, 64, 192, 1 << 20):
            ro.set_option("chunk", chunk)
            for lds in (1, 0):
                ro.set_option("lds", lds)
                got = _check(ro, X0, M, lc.PLANES, 12, first, lo, hi, n_bins, cost)
                assert np.array_equal(got["hist"], whole["hist"]) and np.array_equal(bits(got["stats"]), bits(whole["stats"])), (chunk, lds)


# ---- 3. common random numbers: the lookahead campaign's histogram is the label campaign's -------------------------------------------
@pytest.mark.parametrize("mode", ["expect", "worst"])
def test_lattice_histograms_of_the_two_controllers_are_identical(built, mode):
    """on the exactly posed lattice the flights of the two controllers coincide under one seed (the plain K29 suite shows it for
    the statistics): so do their histograms, count for count"""
    import hjbdp
    K = nrefs.LATTICE_STAGES
    with hjbdp.Backup(nrefs.lattice_spec(mode)) as bk:
        sol = bk.solve(K, keep_J=True, keep_idx=True)
    J = sol["J_stages"].reshape(33, K, order="F")
    idx = sol["idx_stages"].reshape(33, K, order="F")
    weights = nrefs.LATTICE_P if mode == "expect" else None
    X0 = nrefs.LATTICE_STARTS.reshape(1, -1)                                    # 9 starts
    M, seed, n_bins = 1 << 10, 2030, 32
    with hjbdp.Rollout([nrefs.LATTICE_KNOTS], idx, nrefs.LATTICE_U, index_base=0) as ro:
        ro.set_model([[1.0]], [[1.0]], q=[1.0], r=[0.5])
        ro.set_noise(nrefs.LATTICE_NODES, weights)
        ro.set_values(J)
        ro.set_lookahead(nrefs.LATTICE_NODES, weights, mode)
        first = ro.run_campaign(X0, np.arange(K), M, seed=seed, method="nearest")
        rng_ = (first["min"], np.nextafter(first["max"], np.inf), n_bins)
        labels = ro.run_campaign(X0, np.arange(K), M, seed=seed, method="nearest", hist=rng_)
        look = ro.run_lookahead_campaign_hist(X0, list(range(1, K)) + [-1], M, rng_, seed=seed)
    assert np.array_equal(look["hist"], labels["hist"]) and np.array_equal(bits(look["stats"]), bits(labels["stats"]))
    assert np.all(look["hist"].sum(axis=1) == M) and not look["hist"][:, 0].any() and not look["hist"][:, -1].any()
    assert np.all((look["hist"][:, 1:-1] > 0).sum(axis=1) > 1)                  # a distribution, not one bin


# ---- 4. the mirror -------------------------------------------------------------------------------------------------------------------
def test_dynamic_solver_lookahead_cost_quantiles(built):
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.dx, ds.du, ds.N = 13, 17, 6
    ds.u_min, ds.u_max = DS_U_RANGE
    ds.disturbance = (DS_NODES, DS_WEIGHTS, "expect")
    ds.run()
    M, n_bins = 64, 16
    qs = (0.0, 0.5, 0.95, 1.0)
    X0s = np.array([[0.3, -0.5, 0.1], [0.2, 0.4, -0.6]])
    out = ds.get_lookahead_cost_quantiles(X0s, M, q=qs, n_bins=n_bins, seed=6)
    cost = ds.get_lookahead_paths(X0s, n_samples=M, seed=6)                     # [3, 64], the same streams
    srt = np.sort(cost, axis=1)
    assert np.array_equal(out["hist"], hjbdp.campaign_hist_reduce(cost, M, out["hist_lo"], out["hist_hi"], n_bins))
    assert np.array_equal(bits(out["stats"]), bits(ds.get_lookahead_cost_statistics(X0s, M, seed=6)["stats"]))
    for s in range(3):
        lo, hi = out["hist_lo"][s], out["hist_hi"][s]
        for i, q in enumerate(qs):
            j = hrefs.quantile_column(out["hist"][s], q)
            x = srt[s, hrefs.rank_of(q, M) - 1]
            q_hat, below = min(hrefs.edge(j, lo, hi, n_bins), srt[s, -1]), hrefs.edge(j - 1, lo, hi, n_bins)
            assert out["quantiles"][s, i] == q_hat and below <= x <= q_hat, (s, q, below, x, q_hat)
    assert np.array_equal(out["quantiles"][:, -1], srt[:, -1])
    qmap = ds.lookahead_cost_quantile_map(8, q=(0.5, 1.0), n_bins=4, seed=6, lookahead="nominal")
    assert qmap["quantiles"].shape == (13, 13, 2) and qmap["hist"].shape == (13, 13, 6)
    assert np.array_equal(qmap["quantiles"][:, :, 1], qmap["max"]) and np.all(qmap["hist"].sum(axis=2) == 8)
    with pytest.raises(ValueError):
        ds.get_lookahead_cost_quantiles(X0s, M, lookahead="other")
