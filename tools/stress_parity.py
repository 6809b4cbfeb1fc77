"""Randomised GPU-vs-oracle parity stress: random shapes (D, C, grid sizes, dtype, knot spacing, displacement
spread, J storage, argmin label width, float64-built query tables, float64 cost terms, the monitor in float32 or float64), every applicable
stage-kernel variant plus hjb_solve's multi-stage paths, whole grids and slabs; every handle that takes option "grid" sweeps a second
time under a launch drawn from [1, 2 x its automatic grid] (a walk of several passes, or idle workgroups).
Every result must equal the C oracle's bit for bit.  usage: python tools/stress_parity.py [seconds=120] [seed=0]"""
import os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "optimal-control-dynamic-programming_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hjbdp
from hjbdp import _abi
from oracle import c_oracle
from problems import colsweep_problem, nested_problem, random_problem, random_terminal

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
t_end = time.time() + budget
n_prob = n_runs = 0
seen = {}
while time.time() < t_end:
    D = int(rng.integers(1, 7))
    C = int(rng.integers(1, 4))
    cap = {1: 400, 2: 70, 3: 18, 4: 9, 5: 6, 6: 5}[D]
    n = tuple(int(rng.integers(2, cap + 1)) for _ in range(D))
    m = tuple(int(rng.integers(1, 8)) for _ in range(C))
    if np.prod(n) * np.prod(m) > 3e6:
        continue
    dtype = np.float32 if rng.random() < 0.6 else np.float64
    nonuniform = bool(rng.random() < 0.4)
    spread = float(rng.choice([0.02, 0.1, 0.3, 0.8]))
    seed = int(rng.integers(1 << 30))
    grid_rng = np.random.default_rng([seed, 0x67726964])      # the forced launch sizes: a sequence of its own per problem
    kind = rng.choice(["nested", "nested_mixed", "random", "rowwise", "local2d", "colsweep", "colsweep"]) if C <= D else "random"
    try:
        if kind == "local2d":         # every query within one cell of its state: hjb_solve's several-stages-per-launch path
            from hjbdp import Term
            D, C = 2, 1
            n = (int(rng.integers(3, 90)), int(rng.integers(3, 90)))
            kx, kv = np.linspace(-0.5, 0.5, n[0]), np.linspace(-0.4, 0.6, n[1])
            hx, hv = kx[1] - kx[0], kv[1] - kv[0]
            U = np.linspace(-0.26, 0.26, int(rng.integers(1, 6)))
            m = (len(U),)
            nxt = [[Term((0,), kx), Term((1,), 0.9 * hx * np.sin(3 * kv))],
                   [Term((1,), kv), Term((0,), 0.4 * hv * np.cos(5 * kx)), Term((2,), 0.55 * hv * U / 0.26)]]
            cost = [Term((0,), 6 * kx ** 2), Term((1,), 3 * kv ** 2), Term((2,), 0.1 * U ** 2), Term((0, 1), 0.05 * rng.random(n))]
            spec = hjbdp.ProblemSpec([kx, kv], m, nxt, cost, dtype=dtype, index_base=1)
        elif kind == "colsweep":      # the pos-att shape: variant 7 in its forms (one load per row / two, cooperative)
            D, C = 4, 1
            n = (int(rng.choice([int(rng.integers(3, 150)), 64, 120, 128, 60, 61, 121])), int(rng.integers(2, 14)),
                 int(rng.integers(3, 13)), int(rng.integers(3, 13)))
            if np.prod(n) > 4e5:
                n = (n[0], min(n[1], 6), min(n[2], 7), min(n[3], 7))
            nU = int(rng.integers(1, 17))
            m = (nU,)
            dtype = np.float32
            gax = int(rng.choice([2, 3]))
            spec = colsweep_problem(seed, n, nU=nU, nonuniform=nonuniform, gax=gax, big=float(rng.choice([0.4, 1.3, 2.7, 3.8])),
                                    small=float(rng.choice([0.2, 0.6, 0.95])), cost=str(rng.choice(["fast", "step01", "multi", "ctrl_only"])),
                                    a1_amp=float(rng.choice([0.3, 0.6, 1.8])), levels=int(rng.integers(1, 7)),
                                    a1_axis=(None if rng.random() < 0.5 else int(rng.choice([2, 3]))))
        elif kind == "rowwise":       # no axis but axis 0 depends on state dim 0: variant 6 (lean form when it applies)
            if D < 2:
                continue
            sp0 = nested_problem(seed, n, m, dtype=dtype, nonuniform=nonuniform, spread=spread)
            nxt = [sp0.next_terms[0]] + [[t for t in sp0.next_terms[a] if 0 not in t.dims] for a in range(1, D)]
            spec = hjbdp.ProblemSpec(sp0.knots, sp0.m, nxt, sp0.cost_terms, dtype=dtype, index_base=1)
        elif kind == "random":
            spec = random_problem(seed, n, m, dtype=dtype, nonuniform=nonuniform)
        else:
            spec = nested_problem(seed, n, m, dtype=dtype, nonuniform=nonuniform, spread=spread,
                                  mixed_inner=(kind == "nested_mixed"))
    except Exception as e:       # generator constraints (e.g. too many terms)
        continue
    if dtype == np.float32 and rng.random() < 0.25:
        spec = hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, dtype=np.float32, index_base=1,
                                 j_storage=np.float16)
    # the typing options of round 3: label width, float64-built tables (float32 problems; the float64 copy of the terms
    # is what the generators produced before the spec rounded them), the monitor's summation type
    idx_dtype = [None, None, "auto", np.uint8, np.uint16][int(rng.integers(0, 5))]
    if idx_dtype is np.uint8 and spec.nU - 1 + spec.index_base > 255:
        idx_dtype = "auto"
    tab64 = bool(spec.dtype == np.float32 and rng.random() < 0.3)
    cost64 = bool(spec.dtype == np.float32 and rng.random() < 0.25)      # round 4: float64 cost terms, one rounding per backup
    if idx_dtype is not None or tab64 or cost64:
        spec = hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, dtype=spec.dtype, index_base=spec.index_base,
                                 j_storage=None if spec.j_dtype == spec.dtype else spec.j_dtype, idx_dtype=idx_dtype,
                                 table_dtype=np.float64 if tab64 else None, cost_dtype=np.float64 if cost64 else None)
    mon = {}
    if rng.random() < 0.3:
        mon = dict(monitor_period=int(rng.integers(1, 4)), monitor_tol=float(rng.choice([0.0, 1e-3, 1e30])),
                   monitor_single=bool(rng.random() < 0.5))
    term = random_terminal(spec, seed + 1).astype(spec.j_dtype)
    stages = int(rng.choice([1, 2, 5, 17, 40, 70]))
    if kind == "local2d":
        stages = int(rng.choice([16, 23, 40, 70, 129]))
    if spec.nS * spec.nU * stages > 4e7:
        stages = 2
    ref = c_oracle.sweep(_abi, spec, stages, terminal=term, nthreads=16, **mon)
    jabs = np.abs(ref["J"].astype(np.float64))
    if not np.all(np.isfinite(jabs)) or jabs.max() > (1e30 if spec.j_dtype.itemsize <= 4 else 1e290):
        continue      # random dynamics with strong extrapolation can blow J up to inf/NaN: outside the contract
                      # (SURVEY 8a note 3: "NaNs ... none arise"; min/argmin of NaNs is not defined alike everywhere).
                      # A finite final J of magnitude 1e36 has passed through -inf / NaN states on the way (found by
                      # seed 11: variant 3's cross-lane reduction and the sequential `tot < best` treat NaN totals differently)
    n_prob += 1
    for v in (None, 0, 1, 2, 3, 4, 5, 6, 7, "7 two loads", "7 coop"):
        try:
            bk = hjbdp.Backup(spec, variant=7 if isinstance(v, str) else v)
        except hjbdp.HjbError as e:
            assert e.status == _abi.HJB_E_UNSUPPORTED, (v, str(e))
            continue
        if mon and kind == "local2d":
            pass
        with bk:
            if v == "7 two loads":
                bk.set_option("cs_dpp", 0)
            if v == "7 coop":
                bk.set_option("cs_coop", 1)
                if not bk.get_option("cs_coop"):
                    continue
            kv = bk.info()["kernel_variant"]
            out = bk.solve(stages, terminal=term, **mon)
            assert out["idx"].dtype == spec.idx_np_dtype
            runs = [(None, out)]
            # ... and once more under a launch of another size (the kernels that walk their work in grid-sized passes: fewer workgroups
            # than the work, or idle ones), drawn from a generator of its own: the sequence of problems does not depend on it
            auto_grid = bk.get_option("grid")
            grid = int(grid_rng.integers(1, min(2 * auto_grid, 1 << 20) + 1))
            try:
                bk.set_option("grid", grid)
            except hjbdp.HjbError as e:       # the launch is part of the kernel's plan (variants 7 and 1, K15)
                assert e.status == _abi.HJB_E_UNSUPPORTED, (v, str(e))
            else:
                runs.append((grid, bk.solve(stages, terminal=term, **mon)))
        for grid, out in runs:
            ok = np.array_equal(out["J"], ref["J"], equal_nan=True) and np.array_equal(out["idx"], ref["idx"])
            if mon:
                # float32 sums: the library's stated order, bit for bit; float64 sums: order-free to rounding
                exact = mon["monitor_single"] and spec.dtype == np.float32
                close = (out["last_e"] == ref["last_e"]) if exact else (abs(out["last_e"] - ref["last_e"]) <= 1e-9 * max(abs(ref["last_e"]), 1e-300) + 1e-9)
                ok = ok and out["stages_done"] == ref["stages_done"] and (close or not np.isfinite(ref["last_e"])) and out["last_e2"] == ref["last_e2"]   # (f16 J may overflow to inf/NaN over many stages - on both sides alike)
            seen[(v, kv)] = seen.get((v, kv), 0) + 1
            n_runs += 1
            if not ok:
                dj = np.flatnonzero(~((out["J"] == ref["J"]) | (np.isnan(out["J"].astype(np.float64)) & np.isnan(ref["J"].astype(np.float64)))))
                di = np.flatnonzero(out["idx"] != ref["idx"])
                print("  J differs at %d of %d states (first %s), idx at %d (first %s)" % (dj.size, spec.nS, dj[:6], di.size, di[:6]), flush=True)
                if dj.size:
                    print("  J gpu", out["J"][dj[:4]], "oracle", ref["J"][dj[:4]], flush=True)
                if di.size:
                    print("  idx gpu", out["idx"][di[:4]], "oracle", ref["idx"][di[:4]], "J there", out["J"][di[:4]], ref["J"][di[:4]], flush=True)
                print("  stages_done", out.get("stages_done"), ref.get("stages_done"), "info", bk.info() if False else kv, flush=True)
                try:
                    import pickle
                    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
                    with open(os.path.join(ROOT, "gpurun_out", "stress_fail.pkl"), "wb") as fh:
                        pickle.dump(dict(knots=[np.asarray(k) for k in spec.knots], m=list(spec.m),
                                         next_terms=[[(t.dims, np.asarray(t.data)) for t in ts] for ts in spec.next_terms],
                                         cost_terms=[(t.dims, np.asarray(t.data)) for t in spec.cost_terms], dtype=str(spec.dtype),
                                         j_dtype=str(spec.j_dtype), idx_dtype=str(idx_dtype), tab64=tab64, cost64=cost64, term=term, stages=stages,
                                         mon=mon, forced=v, grid=grid), fh)
                except Exception as e:
                    print("  (dump failed: %s)" % e)
                print("MISMATCH", dict(D=D, C=C, n=n, m=m, dtype=str(np.dtype(dtype)), j=str(spec.j_dtype), nonuniform=nonuniform,
                                       spread=spread, seed=seed, kind=str(kind), stages=stages, forced=v, ran=kv, grid=grid, idx=str(idx_dtype), tab64=tab64, cost64=cost64, mon=mon), flush=True)
                sys.exit(1)
    # a random slab of the last axis with the halos the library asks for, one stage
    nl = spec.n[-1]
    if nl >= 4:
        with hjbdp.Backup(spec) as bk:
            need = bk.info()
        b = int(rng.integers(0, nl - 1)); e = int(rng.integers(b + 1, nl + 1))
        lo, hi = min(need["halo_needed_lo"], b), min(need["halo_needed_hi"], nl - e)
        if (e + hi) - (b - lo) >= 2:
            inner = spec.nS // nl
            sub = np.asfortranarray(term.reshape(inner, nl, order="F")[:, b - lo:e + hi]).reshape(-1, order="F")
            Jr, ir = c_oracle.backup_stage(_abi, spec, sub, slab=(b, e, lo, hi), nthreads=16)
            with hjbdp.Backup(spec, slab=(b, e, lo, hi)) as bk:
                Jg, ig = bk.backup_stage(sub)
            n_runs += 1
            own = slice(lo * inner, (lo + e - b) * inner)
            if not (np.array_equal(Jg[own], Jr[own], equal_nan=True) and np.array_equal(ig, ir)):
                print("SLAB MISMATCH", dict(D=D, C=C, n=n, m=m, seed=seed, kind=str(kind), slab=(b, e, lo, hi)), flush=True)
                sys.exit(1)
print("stress ok: %d problems, %d GPU runs, all bit-exact; (forced, ran) counts: %s" % (n_prob, n_runs, dict(sorted(seen.items(), key=str))))
