"""Device time of the disturbed stage (kernel variant 8, csrc/kernels_disturb.h) beside the generic stage kernel (variant 0) of the
SAME handle in the SAME process.

Per case, on one handle, on the null stream, after warm-up: a few backup stages from a separable terminal cost make a realistic J;
then the median of REPS HIP-event timings each of hjb_backup_stage_device with
  t0        variant 0 forced, no disturbance (the generic kernel: one gather set per (state, control));
  w1        variant 8, one zero node (its J is then checked equal to variant 0's at sampled states);
  w9_two    variant 8, 9 nodes on two axes (the 3 x 3 Gauss-Hermite product, hjbdp.gaussian_nodes), expected value;
  w9_all    variant 8, 9 seeded nodes that offset EVERY axis, equal weights.
Cases: c4 (tests/problems.py pos_att_channel_spec("terms", n=120) with float32 queries - table_dtype None: the float32 terms typing
the generic kernel serves; 120^4 states, 9 controls, uint8 labels) and kirk (Dynamic_Solver's default problem: 100^2 states, 1000
controls; two axes are all it has, so w9_two offsets ONE axis and w9_all both).
gathers = states x controls x nodes x 2^D corner reads; gathers_per_s = that / time, recorded beside t0's.
Pass condition (recorded as "pass" per case and overall; the tool exits non-zero when it fails): t(W) <= 1.05 * W * t0 for each of
the three - the disturbed stage does W times variant 0's gathers while sharing its term sums and cost; the 5 % is for the
run-to-run spread within one process.

    python tools/time_disturbance.py [--cases c4,kirk] [--reps 20] [--n 120] [--out profiles/disturbance_time.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "optimal-control-dynamic-programming_amd"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))


def time_case(hjbdp, spec, reps, two_axes, warm_stages=2):
    from time_evaluate import Events
    ev = Events()
    esz = np.dtype(spec.j_dtype).itemsize
    isz = np.dtype(spec.idx_np_dtype).itemsize
    nS, D = spec.nS, spec.D
    rng = np.random.default_rng(11)
    vecs = [rng.random(n).astype(spec.dtype) for n in spec.n]
    med = lambda xs: float(np.median(xs))
    cell = np.array([(k[-1] - k[0]) / (len(k) - 1) for k in spec.knots])
    sigma = np.zeros(D)
    sigma[list(two_axes)] = 0.5 * cell[list(two_axes)]
    off_two, w_two = hjbdp.gaussian_nodes(sigma, order=3)
    off_all = 0.5 * cell[:, None] * rng.uniform(-1.0, 1.0, (D, 9))
    configs = [("w1", 1, np.zeros((D, 1)), None), ("w9_two", 9, off_two, w_two), ("w9_all", 9, off_all, None)]
    out = {"grid": "x".join(str(n) for n in spec.n), "n_states": int(nS), "n_controls": int(spec.nU), "reps": int(reps)}
    with hjbdp.Backup(spec) as bk, hjbdp.DeviceBuffer(nS * esz) as dA, hjbdp.DeviceBuffer(nS * esz) as dB, \
            hjbdp.DeviceBuffer(nS * esz) as dC, hjbdp.DeviceBuffer(nS * isz) as dL:
        out["automatic_variant"] = int(bk.info()["kernel_variant"])
        bk.fill_separable(vecs, dA)
        for _ in range(warm_stages):                    # a J a few stages deep, ending in dA (the handle's automatic kernel)
            bk.backup_stage_device(dA, dB, dL)
            bk.backup_stage_device(dB, dA, dL)
        bk.set_option("variant", 0)
        bk.backup_stage_device(dA, dB, dL)              # warm-up
        bk.check_device_status()
        t0 = [ev.time(lambda: bk.backup_stage_device(dA, dB, dL)) for _ in range(reps)]
        g0 = nS * spec.nU * (1 << D)
        out["t0"] = {"variant": 0, "ms": round(med(t0), 4), "ms_min": round(min(t0), 4), "gathers_per_s": float("%.4g" % (g0 / (med(t0) * 1e-3)))}
        sel = rng.integers(0, nS, min(nS, 1 << 20))
        ok = True
        for name, W, off, w in configs:
            bk.set_disturbance(off, w, "expect")
            assert bk.info()["kernel_variant"] == 8
            bk.backup_stage_device(dA, dC, dL)          # warm-up
            bk.check_device_status()
            t = [ev.time(lambda: bk.backup_stage_device(dA, dC, dL)) for _ in range(reps)]
            rec = {"variant": 8, "nodes": W, "offset_axes_mask": bk.get_option("dist_axes"), "index_form": "32-bit" if bk.get_option("dist_form") else "64-bit",
                   "ms": round(med(t), 4), "ms_min": round(min(t), 4), "gathers_per_s": float("%.4g" % (g0 * W / (med(t) * 1e-3))),
                   "over_W_t0": round(med(t) / (W * med(t0)), 4)}
            rec["pass"] = bool(med(t) <= 1.05 * W * med(t0))
            if name == "w1":
                rec["equals_variant_0_at_samples"] = bool(np.array_equal(dB.gather(spec.j_dtype, sel), dC.gather(spec.j_dtype, sel)))
                ok = ok and rec["equals_variant_0_at_samples"]
            ok = ok and rec["pass"]
            out[name] = rec
        bk.clear_disturbance()
    ev.close()
    out["pass"] = bool(ok)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c4,kirk")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=120, help="points per axis of the c4 case")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "disturbance_time.json"))
    a = ap.parse_args()
    import hjbdp
    if hjbdp.device_count() < 1:
        raise SystemExit("time_disturbance needs a HIP device")
    res = {"tool": "time_disturbance", "timing": "median of HIP-event pairs on the null stream, one handle, one process, after warm-up",
           "condition": "t(W) <= 1.05 * W * t0 for w1, w9_two, w9_all"}
    for c in a.cases.split(","):
        if c == "c4":
            from problems import pos_att_channel_spec
            s = pos_att_channel_spec("terms", n=a.n)
            spec = hjbdp.ProblemSpec(s.knots, s.m, s.next_terms, s.cost_terms, dtype=np.float32, index_base=1, idx_dtype=s.idx_dtype)
            two = (2, 3)
        elif c == "kirk":
            spec = hjbdp.Dynamic_Solver().build_spec()
            two = (1,)
        else:
            raise SystemExit("unknown case %r" % c)
        res[c] = time_case(hjbdp, spec, a.reps, two)
    res["pass"] = all(res[c]["pass"] for c in a.cases.split(","))
    print(json.dumps(res))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    if not res["pass"]:
        raise SystemExit("the disturbed stage missed t(W) <= 1.05 W t0 (or differs from variant 0 at one zero node): %s"
                         % {c: {k: v.get("over_W_t0") for k, v in res[c].items() if isinstance(v, dict) and "over_W_t0" in v} for c in a.cases.split(",")})


if __name__ == "__main__":
    main()
