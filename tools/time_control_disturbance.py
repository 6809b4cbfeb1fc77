"""Device time of the per-control disturbed stage (kernel variant 8 in its per-control form, csrc/kernels_ctrldist.h) beside the
additive disturbed stage (csrc/kernels_disturb.h) of the SAME handle in the SAME process.

Per case, on one handle, on the null stream, after warm-up: a few backup stages from a separable terminal cost make a realistic J;
then the median of REPS HIP-event timings each of hjb_backup_stage_device with
  a_additive   hjb_set_disturbance with a 9-node set (the 3 x 3 Gauss-Hermite product on two axes, hjbdp.gaussian_nodes);
  b_repeated   hjb_set_control_disturbance with that set repeated for every control - the same problem read from the table
               (its J is then checked equal to (a)'s at sampled states);
  c_actuator   hjb_set_control_disturbance with an hjbdp.actuator_nodes table: 9 relative actuator errors eps_w, the offsets of
               control l are eps_w times the control's own part of the next state.
Cases: c4 (tests/problems.py pos_att_channel_spec("terms", n=120) with float32 queries: 120^4 states, 9 controls, uint8 labels;
nodes on axes 2 and 3) and kirk (Dynamic_Solver's default problem: 100^2 states, 1000 controls; nodes on both axes).
Pass condition (recorded as "pass" per case and overall; the tool exits non-zero when it fails): t(b) <= 1.05 * t(a) - the table
costs nothing beside the block; the 5 % is for the run-to-run spread within one process.  (c) is recorded, not judged: it is
another problem (other offset axes, other cells).

    python tools/time_control_disturbance.py [--cases c4,kirk] [--reps 20] [--n 120] [--out profiles/control_disturbance_time.json]
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


def control_part(spec):
    """[D, nU]: per state axis the sum of the next-state terms that depend on the controls alone - B u_l of a linear plant."""
    out = np.zeros((spec.D, spec.nU))
    for a in range(spec.D):
        for t in spec.next_terms[a]:
            if all(d >= spec.D for d in t.dims):
                shape = [1] * spec.C
                for ax, d in enumerate(t.dims):
                    shape[d - spec.D] = spec.m[d - spec.D]
                full = np.broadcast_to(np.asarray(t.data, dtype=np.float64).reshape(shape, order="F"), spec.m)
                out[a] += full.reshape(-1, order="F")
    return out


def time_case(hjbdp, spec, reps, two_axes, warm_stages=2):
    from time_evaluate import Events
    ev = Events()
    esz = np.dtype(spec.j_dtype).itemsize
    isz = np.dtype(spec.idx_np_dtype).itemsize
    nS, D, nU = spec.nS, spec.D, spec.nU
    rng = np.random.default_rng(11)
    vecs = [rng.random(n).astype(spec.dtype) for n in spec.n]
    med = lambda xs: float(np.median(xs))
    cell = np.array([(k[-1] - k[0]) / (len(k) - 1) for k in spec.knots])
    sigma = np.zeros(D)
    sigma[list(two_axes)] = 0.5 * cell[list(two_axes)]
    off, w = hjbdp.gaussian_nodes(sigma, order=3)
    W = off.shape[1]
    eps = np.linspace(-0.2, 0.2, W)
    act, _ = hjbdp.actuator_nodes(np.eye(D), control_part(spec).T, eps)
    configs = [("a_additive", lambda bk: bk.set_disturbance(off, w, "expect")),
               ("b_repeated", lambda bk: bk.set_control_disturbance(np.repeat(off[:, :, None], nU, axis=2), w, "expect")),
               ("c_actuator", lambda bk: bk.set_control_disturbance(act, w, "expect"))]
    out = {"grid": "x".join(str(n) for n in spec.n), "n_states": int(nS), "n_controls": int(nU), "nodes": int(W), "reps": int(reps)}
    with hjbdp.Backup(spec) as bk, hjbdp.DeviceBuffer(nS * esz) as dA, hjbdp.DeviceBuffer(nS * esz) as dB, \
            hjbdp.DeviceBuffer(nS * esz) as dC, hjbdp.DeviceBuffer(nS * isz) as dL:
        bk.fill_separable(vecs, dA)
        for _ in range(warm_stages):                    # a J a few stages deep, ending in dA (the handle's automatic kernel)
            bk.backup_stage_device(dA, dB, dL)
            bk.backup_stage_device(dB, dA, dL)
        sel = rng.integers(0, nS, min(nS, 1 << 20))
        for name, setit in configs:
            setit(bk)
            assert bk.info()["kernel_variant"] == 8
            dOut = dB if name == "a_additive" else dC
            bk.backup_stage_device(dA, dOut, dL)        # warm-up
            bk.check_device_status()
            t = [ev.time(lambda: bk.backup_stage_device(dA, dOut, dL)) for _ in range(reps)]
            out[name] = {"per_control": bool(bk.get_option("dist_ctrl")), "offset_axes_mask": bk.get_option("dist_axes"),
                         "index_form": "32-bit" if bk.get_option("dist_form") else "64-bit", "ms": round(med(t), 4), "ms_min": round(min(t), 4)}
            if name == "b_repeated":
                out[name]["equals_additive_at_samples"] = bool(np.array_equal(dB.gather(spec.j_dtype, sel), dC.gather(spec.j_dtype, sel)))
        bk.clear_disturbance()
    ev.close()
    out["b_over_a"] = round(out["b_repeated"]["ms"] / out["a_additive"]["ms"], 4)
    out["c_over_a"] = round(out["c_actuator"]["ms"] / out["a_additive"]["ms"], 4)
    out["pass"] = bool(out["b_repeated"]["ms"] <= 1.05 * out["a_additive"]["ms"] and out["b_repeated"]["equals_additive_at_samples"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c4,kirk")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=120, help="points per axis of the c4 case")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "control_disturbance_time.json"))
    a = ap.parse_args()
    import hjbdp
    if hjbdp.device_count() < 1:
        raise SystemExit("time_control_disturbance needs a HIP device")
    res = {"tool": "time_control_disturbance", "timing": "median of HIP-event pairs on the null stream, one handle, one process, after warm-up",
           "condition": "t(b_repeated) <= 1.05 * t(a_additive), and equal J at the sampled states"}
    for c in a.cases.split(","):
        if c == "c4":
            from problems import pos_att_channel_spec
            s = pos_att_channel_spec("terms", n=a.n)
            spec = hjbdp.ProblemSpec(s.knots, s.m, s.next_terms, s.cost_terms, dtype=np.float32, index_base=1, idx_dtype=s.idx_dtype)
            two = (2, 3)
        elif c == "kirk":
            spec = hjbdp.Dynamic_Solver().build_spec()
            two = (0, 1)
        else:
            raise SystemExit("unknown case %r" % c)
        res[c] = time_case(hjbdp, spec, a.reps, two)
    res["pass"] = all(res[c]["pass"] for c in a.cases.split(","))
    print(json.dumps(res))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    if not res["pass"]:
        raise SystemExit("the per-control stage missed t(b) <= 1.05 t(a) (or differs from the additive stage on a repeated set): %s"
                         % {c: res[c]["b_over_a"] for c in a.cases.split(",")})


if __name__ == "__main__":
    main()
