"""Reference for the backup under a control-dependent disturbance (hjb_set_control_disturbance, kernel variant 8 in its per-control
form): disturbance_refs.DisturbedRef with the ONE change the contract of include/hjbdp.h makes - in step 1 the offset of node w is
read from the candidate's own column, off[a, w, label] (label: 0-based, column-major).  Steps 2 - 5, the first-minimum scan and the
sweep are inherited unchanged.
"""
from __future__ import annotations

import numpy as np

from disturbance_refs import DisturbedRef
from oracle import hjb_oracle


class ControlDisturbedRef(DisturbedRef):
    """spec: hjbdp.ProblemSpec (no state model); offsets [D, W, nU] float64 (or [D, W, *m], flattened column-major), weights [W]
    or None, mode - what Backup.set_control_disturbance takes."""

    def __init__(self, spec, offsets, weights=None, mode="expect"):
        off = np.array(offsets, dtype=np.float64)
        if off.ndim == 2 + spec.C and off.shape[2:] == spec.m:
            off = off.reshape(off.shape[:2] + (spec.nU,), order="F")
        assert off.ndim == 3 and off.shape[0] == spec.D and off.shape[2] == spec.nU
        super().__init__(spec, off[:, :, 0], weights, mode)
        self.axes = [bool(np.any(off[a] != 0.0)) for a in range(spec.D)]        # some (w, l) entry of row a is not zero
        self.off = off.astype(self.TQ)                                           # rounded once to TQ

    def _node_query(self, q, a, w, labels0):
        return (q[a] + self.off[a, w, labels0]).astype(self.TQ, copy=False) if self.axes[a] else q[a]

    def locate(self, states, labels0):
        sp = self.spec
        labels0 = np.asarray(labels0, dtype=np.int64)
        at = tuple(np.unravel_index(np.asarray(states, dtype=np.int64), sp.n, order="F")) + \
            tuple(np.unravel_index(labels0, sp.m, order="F"))
        q = [self._osum(sp.next_terms[a], at, self.TQ) for a in range(sp.D)]                       # step 1
        cells, ts = [], []
        for w in range(self.W):
            cw, tw = [], []
            for a in range(sp.D):
                i, t = hjb_oracle.cell_and_weight(self.knots[a], self._node_query(q, a, w, labels0))   # step 2
                cw.append(i)
                tw.append(t.astype(self.T))
            cells.append(cw)
            ts.append(tw)
        return at, q, cells, ts

    def coverage(self):
        sp = self.spec
        states = np.repeat(np.arange(sp.nS), sp.nU)
        labels0 = np.tile(np.arange(sp.nU), sp.nS)
        _, q, cells, _ = self.locate(states, labels0)
        out = {}
        for a in range(sp.D):
            if not self.axes[a]:
                continue
            qw = np.stack([self._node_query(q, a, w, labels0) for w in range(self.W)])
            cw = np.stack([cells[w][a] for w in range(self.W)])
            out[a] = (bool((qw < self.knots[a][0]).any()), bool((qw > self.knots[a][-1]).any()),
                      bool((cw.max(axis=0) != cw.min(axis=0)).any()))
        return out
