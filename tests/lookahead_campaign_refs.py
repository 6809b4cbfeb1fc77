"""What the tests of the lookahead campaign (hjb_rollout_run_lookahead_campaign, K29) share: the seeded problem of every
instantiation - K27's test's problem (tests/test_gpu_rollout_lookahead.py: greedy_rollout_refs.random_problem, a lookahead set of 3
nodes on a proper subset of the axes, a flight set of 4 nodes on another subset, the modes alternated) - and the chain of entry
points older than the campaign that its statistics must equal as bits, with no device:
    noise_thresholds -> noise_draw -> lookahead_host(nodes=..., flight_offsets=..., keep_path=True) -> campaign_refs.left_flags
    -> campaign_reduce
on the starts repeated M times: trajectory s * M + m is sample m of start s, on stream first_stream + s * M + m."""
from __future__ import annotations

import numpy as np

import campaign_refs as crefs
import greedy_rollout_refs as grefs
import lookahead_rollout_refs as lrefs

PLANES = [2, 0, -1, 1, 2, 1]               # 6 steps: -1 inside, the Philox block of k = 4 begins inside
N_STARTS = 37                              # with M = 5: G = 8 with three padding slots, 37 blocks - the last wave part-filled


# the generator's seed per (D, 8-byte values): 2900 + 10 D + wide where test_lookahead_campaign_host.py's three conditions on the
# statistics hold at M = 5 (some flight left the grid; n_exceed and n_settled neither empty nor full), else the next + 100 that does:
# at D = 4 with float32 planes no flight of 2940 settled
RNG_SEEDS = {(D, w): 2900 + 10 * D + w for D in range(1, 7) for w in (0, 1)}
RNG_SEEDS[(4, 0)] = 3040


def axes(D):
    """(lookahead axes, flight axes) as K27's test takes them: a proper subset of the axes from D = 2 on, and another one"""
    look = [0, D - 1] if D >= 3 else [D - 1]
    fly = sorted({D // 2, 1 % D}) if D != 2 else [0]
    return look, fly


def flight_set(rng, D, fly_axes, W=4):
    F = np.zeros((D, W))
    for a in fly_axes:
        F[a] = rng.uniform(-0.15, 0.15, size=W)
    F[fly_axes[0], 1] = 0.0
    return F, rng.uniform(0.2, 1.0, size=W)


def problem(D, dtype, n_starts=N_STARTS):
    """the seeded problem of instantiation (D, dtype): a dict of lookahead_host's arguments (`model`), the two node sets, the
    starts, the seed and the first stream"""
    wide = np.dtype(dtype).itemsize == 8
    rng = np.random.default_rng(RNG_SEEDS[(D, int(wide))])
    nu = (D - 1 + wide) % 4 + 1                                 # n_u cycles over 1..4
    mode = "expect" if (D + wide) % 2 else "worst"              # the modes alternate
    knots, ut, A, B, c, q, r, V = grefs.random_problem(rng, D, nu, 5, 3, dtype)
    look_axes, fly_axes = axes(D)
    E, P = lrefs.node_sets(rng, D, 3, look_axes, with_weights=(mode == "expect"))
    F, Pf = flight_set(rng, D, fly_axes)
    return dict(D=D, knots=knots, ut=ut, A=A, B=B, V=V, model=dict(c=c, q=q, r=r), E=E, P=P, mode=mode, F=F, Pf=Pf,
                X0=grefs.starts(rng, knots, n_starts), seed=91 + D, first=4000 + 7 * D)


def fly_chain(pb, X0, M, planes=PLANES, seed=None, first=None):
    """the per-trajectory flights of the chain: lookahead_host's dict (keep_path) on np.repeat(X0, M, axis=1), plus "left" """
    import hjbdp
    seed = pb["seed"] if seed is None else seed
    first = pb["first"] if first is None else first
    Xr = np.repeat(X0, M, axis=1)
    nodes = hjbdp.noise_draw(hjbdp.noise_thresholds(pb["Pf"], pb["F"].shape[1]), Xr.shape[1], len(planes), seed=seed, first_stream=first)
    flown = hjbdp.lookahead_host(pb["knots"], pb["ut"], pb["A"], pb["B"], pb["V"], Xr, planes, pb["E"], pb["P"], pb["mode"], nodes=nodes,
                                 flight_offsets=pb["F"], keep_path=True, **pb["model"])
    flown["left"] = crefs.left_flags(flown["X_path"], pb["knots"])
    return flown


def reduce_flown(flown, M, thr=None, tol=None):
    """campaign_reduce of a per-trajectory dict (fly_chain's, or run_lookahead's with "left" added)"""
    import hjbdp
    return hjbdp.campaign_reduce(flown["cost"], M, X_final=flown["X_final"], left=flown["left"], cost_threshold=thr, settle_tol=tol)


def bounds_of(flown):
    """a threshold and a tolerance taken from the flight itself: the median cost, the mean |x_final| per axis"""
    return float(np.median(flown["cost"])), np.abs(flown["X_final"]).mean(axis=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
