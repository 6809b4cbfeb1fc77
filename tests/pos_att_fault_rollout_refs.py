"""Plain numpy restatement of hjb_rollout_run_pos_att_faults (include/hjbdp.h, csrc/kernels_rollout_pos_att_faults.h), the checker of
tests/test_gpu_rollout_pos_att_faults.py, vectorised over trajectories, one IEEE float64 operation at a time.  It is
pos_att_rollout_refs.rollout (whose pieces it imports) with, per trajectory i at stage k:
  channel x looked up in the fault controller when switch_stage[i] <= k, else in the nominal one (both through the oracle's C
  twin, oracle.c_oracle.lookup, then a select per trajectory: the twin need not branch);
  the applied forces fa_j = +0.0 where fault_stage[i] <= k and bit j of fault_mask[i] is set, else the commanded f_j;
  U_M, a and the RK4 sub-steps on fa; impulse = (sum over k, in order, of ((|fa0| + |fa1|) + ...) + |fa11|) * h;
  settle_stage = 1 + the last m whose state X_m has (x0^2 + x1^2) + x2^2 > pos_tol^2 or (q1^2 + q2^2) + q3^2 > att_tol^2 or a NaN in
  either sum (0 when none has).
None (mask, stages): no fault / stage 0 / never.  Nothing here comes from the package's kernel path.
"""
from __future__ import annotations

import numpy as np

from attitude_rollout_refs import asinc
from pos_att_rollout_refs import AXIS, SLOTS, eci2body, inv3, moments_and_acceleration, mul3, prepare_channels, rk4_stage


def rollout(channels, fault_channel, inertia, mass, t_dist, h, substeps, rsw2eci, coef, X0, plane_of_step, fault_mask=None,
            fault_stage=None, switch_stage=None, pos_tol=np.inf, att_tol=np.inf):
    """channels: for x, y, z (knots [4 grid vectors], labels nS x n_planes (column-major, any shape), u_table [n_labels, 4],
    index_base); fault_channel: the same for the fault controller of channel x, or None; inertia, rsw2eci [3, 3]; coef
    [n_nodes, 5]; X0 [13, n]; fault_mask, fault_stage, switch_stage [n] or None.
    Returns a dict: X_final [13, n], X_path [n, 13, K+1], F_path [n, 12, K] (applied), FM_path [n, 6, K], impulse [n],
    settle_stage [n] (int32), and for the tests' own conditions F_cmd [n, 12, K] (commanded) and Fx_nominal [n, 4, K] (what the
    nominal controller of channel x gives at the same state)."""
    from hjbdp import _abi
    from oracle import c_oracle
    chans = prepare_channels(list(channels) + ([fault_channel] if fault_channel is not None else []))
    J = [float(v) for v in np.asarray(inertia, dtype=np.float64).reshape(9)]
    Ji = [float(v) for v in inv3(np.array(J))]
    RSW = [float(v) for v in np.asarray(rsw2eci, dtype=np.float64).reshape(9)]
    RSWi = [float(v) for v in inv3(np.array(RSW))]
    S = int(substeps)
    hs = float(h) / S
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 5)
    x = np.array(np.asarray(X0, dtype=np.float64).reshape(13, -1))
    n = x.shape[1]
    planes = np.asarray(plane_of_step, dtype=np.int64).reshape(-1)
    K = planes.size
    mask = np.zeros(n, np.int64) if fault_mask is None else np.asarray(fault_mask, dtype=np.int64).reshape(n)
    f_at = np.zeros(n, np.int64) if fault_stage is None else np.asarray(fault_stage, dtype=np.int64).reshape(n)
    s_at = np.full(n, K, np.int64) if switch_stage is None else np.asarray(switch_stage, dtype=np.int64).reshape(n)
    if fault_channel is None and (s_at < K).any():
        raise ValueError("a hand-over needs the fault controller")
    p2, a2 = np.float64(pos_tol) * np.float64(pos_tol), np.float64(att_tol) * np.float64(att_tol)

    def lookup(ch, p, pts):
        ks, lab, ut, base, dense = chans[ch]
        if p not in dense:
            dense[p] = lab[:, p].astype(np.float64)
        L = c_oracle.lookup(_abi, ks, dense[p], pts, "nearest").astype(np.int64) - base
        return ut[L].T                                              # [4, n]

    def outside(y):
        return ~((((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]) <= p2) & (((y[6] * y[6] + y[7] * y[7]) + y[8] * y[8]) <= a2))

    X_path = np.zeros((n, 13, K + 1))
    F_path = np.zeros((n, 12, K))
    F_cmd = np.zeros((n, 12, K))
    Fx_nominal = np.zeros((n, 4, K))
    FM_path = np.zeros((n, 6, K))
    X_path[:, :, 0] = x.T
    imp = np.zeros(n)
    with np.errstate(all="ignore"):
        last_outside = np.where(outside(x), 0, -1)
        for k, p in enumerate(planes):
            s = x[6:9]
            s = np.where(s > 1.0, 1.0, np.where(s < -1.0, -1.0, s))
            th = 2.0 * asinc(s)
            E = eci2body(x[6], x[7], x[8], x[9])
            M = [(E[3 * r] * RSW[c] + E[3 * r + 1] * RSW[3 + c]) + E[3 * r + 2] * RSW[6 + c] for r in range(3) for c in range(3)]
            xb, vb = mul3(M, x[0], x[1], x[2]), mul3(M, x[3], x[4], x[5])
            f = np.zeros((12, n))
            for ch in range(3):
                pts = np.ascontiguousarray(np.stack([xb[ch], vb[ch], th[AXIS[ch]], x[10 + AXIS[ch]]], axis=1))
                u = lookup(ch, p, pts)
                if ch == 0:
                    Fx_nominal[:, :, k] = u.T
                    if (s_at <= k).any():
                        u = np.where(s_at <= k, lookup(3, p, pts), u)
                for j, slot in enumerate(SLOTS[ch]):
                    f[slot] = u[j]
            F_cmd[:, :, k] = f.T
            dead = np.where(f_at <= k, mask, 0)
            for j in range(12):
                f[j] = np.where((dead >> j) & 1 == 1, 0.0, f[j])
            sk = np.abs(f[0]) + np.abs(f[1])
            for j in range(2, 12):
                sk = sk + np.abs(f[j])
            imp = imp + sk
            um, a = moments_and_acceleration(f, E, RSWi, mass, t_dist)
            F_path[:, :, k] = f.T
            FM_path[:, :, k] = np.stack(a + um, axis=1)
            x = rk4_stage(J, Ji, coef, k, S, hs, a, um, x)
            X_path[:, :, k + 1] = x.T
            last_outside = np.where(outside(x), k + 1, last_outside)
        impulse = imp * np.float64(h)
    return {"X_final": x, "X_path": X_path, "F_path": F_path, "FM_path": FM_path, "impulse": impulse,
            "settle_stage": (last_outside + 1).astype(np.int32), "F_cmd": F_cmd, "Fx_nominal": Fx_nominal}
