"""Reference for the disturbed backup (hjb_set_disturbance, kernel variant 8): a numpy restatement of the contract in include/hjbdp.h
for a LIST of (state, control) pairs, bit for bit under every typing a ProblemSpec can carry.

Built on the numpy oracle's own pieces - oracle.hjb_oracle.cell_and_weight and the ordered left-to-right sums - and on
evaluate_refs' exact float32 fma; what those lack is here:
  - float64 queries with the weight rounded to float32 once (table_dtype float64: knots as given, 1 / dx in double);
  - float64 cost sums rounded once (cost_dtype float64);
  - float16 J storage: read widened (exact), stored rounded to nearest even (numpy's astype);
  - the two node combinations: acc = (T)(p_0 v_0), acc = fma(p_w, v_w, acc) / acc = v_0, acc = v_w > acc ? v_w : acc;
  - the first-minimum scan in the kernels' visiting order (control dim 0 slowest), labels column-major (dim 0 fastest);
  - an exact float64 fma on arrays (fma64: error-free transformations and one rounding to odd; evaluate_refs._fma64 is the same
    function one Fraction at a time - tests/test_disturbance_refs.py holds the two equal).
It imports the oracle and changes nothing under oracle/.
"""
from __future__ import annotations

import numpy as np

from evaluate_refs import _fma32
from oracle import hjb_oracle


# ---- exact float64 fma on arrays -----------------------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker's product on Veltkamp's splitting; no overflow / underflow in the ranges tested here)."""
    p = a * b
    c = 134217729.0                                       # 2^27 + 1
    ta, tb = c * a, c * b
    ah = ta - (ta - a)
    bh = tb - (tb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_round_odd(a, b):
    """a + b rounded to odd: the exact sum where it is a double, else the neighbour whose last mantissa bit is 1."""
    s, e = _two_sum(a, b)
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    toward = np.where(e > 0, np.inf, -np.inf)             # the side of s the exact sum lies on
    return np.where(fix, np.nextafter(s, toward), s)


def fma64(a, b, c):
    """float64 fma(a, b, c) with ONE rounding (Boldo & Melquiond, "Emulation of a FMA and correctly rounded sums", 2008):
    (uh, ul) = a * b exactly, (th, tl) = c + ul exactly, (vh, vl) = uh + th exactly, result = RN(vh + RO(vl + tl))."""
    a, b, c = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), np.broadcast(a, b, c).shape)) for x in (a, b, c))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    return vh + _add_round_odd(vl, tl)


# ---- the contract --------------------------------------------------------------------------------------------------------------
class DisturbedRef:
    """spec: hjbdp.ProblemSpec (no state model); offsets [D, W] float64, weights [W] or None, mode "expect" / "worst" - what
    Backup.set_disturbance takes.  Everything below follows include/hjbdp.h's steps 1 - 5 by number."""

    def __init__(self, spec, offsets, weights=None, mode="expect"):
        assert spec.model is None and mode in ("expect", "worst")
        self.spec = spec
        self.T = np.dtype(spec.dtype)
        self.TQ = np.dtype(np.float64) if spec.table_dtype is not None else self.T
        off = np.array(offsets, dtype=np.float64, ndmin=2)
        assert off.shape[0] == spec.D
        self.W = off.shape[1]
        self.axes = [bool(np.any(off[a] != 0.0)) for a in range(spec.D)]        # the host's mask: option "dist_axes"
        self.off = off.astype(self.TQ)                                           # rounded once to TQ
        self.p = (np.full(self.W, 1.0 / self.W) if weights is None else np.asarray(weights, dtype=np.float64)).astype(self.T)
        self.mode = mode
        # knots: rounded to T by the library; the float64 shadow (table_dtype float64) takes them as given
        self.knots = [np.asarray(k, dtype=np.float64).astype(self.TQ) for k in spec.knots]
        self.fma = _fma32 if self.T == np.float32 else fma64

    @property
    def axes_mask(self):
        return sum(1 << a for a in range(self.spec.D) if self.axes[a])

    def _osum(self, terms, at, dt):
        acc = None
        for t in terms:
            x = np.broadcast_to(np.asarray(t.data, dtype=dt)[tuple(at[d] for d in t.dims)], at[0].shape)
            acc = x if acc is None else (acc + x).astype(dt, copy=False)
        return acc

    def locate(self, states, labels0):
        """(cells [W][D], weights [W][D] in T) of every node's query for the listed (state, 0-based column-major label) pairs."""
        sp = self.spec
        at = tuple(np.unravel_index(np.asarray(states, dtype=np.int64), sp.n, order="F")) + \
            tuple(np.unravel_index(np.asarray(labels0, dtype=np.int64), sp.m, order="F"))
        q = [self._osum(sp.next_terms[a], at, self.TQ) for a in range(sp.D)]                       # step 1
        cells, ts = [], []
        for w in range(self.W):
            cw, tw = [], []
            for a in range(sp.D):
                qa = (q[a] + self.off[a, w]).astype(self.TQ, copy=False) if self.axes[a] else q[a]
                i, t = hjb_oracle.cell_and_weight(self.knots[a], qa)                               # step 2 (formed in TQ ...
                cw.append(i)
                tw.append(t.astype(self.T))                                                        # ... rounded to T once)
            cells.append(cw)
            ts.append(tw)
        return at, q, cells, ts

    def coverage(self):
        """What the node queries of EVERY (state, control) reach, per offset axis: {axis: (some query below the first knot,
        some query above the last knot, the nodes of some pair in two different cells)} - a test on interior-only inputs
        would not see a wrong extrapolation or a cell that is not found again per node."""
        sp = self.spec
        states = np.repeat(np.arange(sp.nS), sp.nU)
        labels0 = np.tile(np.arange(sp.nU), sp.nS)
        _, q, cells, _ = self.locate(states, labels0)
        out = {}
        for a in range(sp.D):
            if not self.axes[a]:
                continue
            qw = np.stack([(q[a] + self.off[a, w]).astype(self.TQ) for w in range(self.W)])
            cw = np.stack([cells[w][a] for w in range(self.W)])
            out[a] = (bool((qw < self.knots[a][0]).any()), bool((qw > self.knots[a][-1]).any()),
                      bool((cw.max(axis=0) != cw.min(axis=0)).any()))
        return out

    def candidates(self, J_next, states, labels0):
        """The candidate value, in T, of each listed (state, label) pair.  J_next: the stored cost-to-go (spec.j_dtype), flat
        column-major or shaped spec.n."""
        sp, T = self.spec, self.T
        Jn = np.asarray(J_next)
        Jn = (Jn.reshape(sp.n, order="F") if Jn.ndim == 1 else Jn.reshape(sp.n)).astype(T)         # widening a float16 is exact
        at, _, cells, ts = self.locate(states, labels0)
        acc = None
        for w in range(self.W):
            vals = [Jn[tuple(cells[w][a] + ((corner >> a) & 1) for a in range(sp.D))] for corner in range(1 << sp.D)]
            for a in range(sp.D):                                                                  # step 3: axis 0 first
                vals = [self.fma(ts[w][a], (vals[j + 1] - vals[j]).astype(T, copy=False), vals[j]) for j in range(0, len(vals), 2)]
            v = vals[0]
            if self.mode == "expect":                                                              # step 4
                acc = (self.p[0] * v).astype(T, copy=False) if w == 0 else self.fma(np.broadcast_to(self.p[w], v.shape), v, acc)
            else:
                acc = v if w == 0 else np.where(v > acc, v, acc)
        if sp.cost_dtype is not None:                                                              # step 5
            g = self._osum(sp.cost_terms, at, np.float64).astype(T)
        else:
            g = self._osum(sp.cost_terms, at, T)
        return (g + acc).astype(T, copy=False)

    def evaluate(self, J_next, labels, states=None):
        """hjb_evaluate_stage on `labels` (as the library writes them: index_base included) at `states` (None: every state)
        -> J as STORED (spec.j_dtype)."""
        sp = self.spec
        states = np.arange(sp.nS) if states is None else np.asarray(states, dtype=np.int64)
        lab0 = np.asarray(labels).astype(np.int64) - sp.index_base
        return self.candidates(J_next, states, lab0).astype(sp.j_dtype)

    def backup(self, J_next, states=None):
        """hjb_backup_stage at `states` (None: every state) -> (J as stored, labels in spec.idx_np_dtype with index_base)."""
        sp = self.spec
        states = np.arange(sp.nS) if states is None else np.asarray(states, dtype=np.int64)
        nU = sp.nU
        # visiting order: control dim 0 slowest (C-order over m); the label is the column-major flat index
        sub = np.unravel_index(np.arange(nU), sp.m, order="C")
        label_of_visit = np.ravel_multi_index(sub, sp.m, order="F")
        tot = self.candidates(J_next, np.repeat(states, nU), np.tile(label_of_visit, states.size)).reshape(states.size, nU)
        best = tot[:, 0].copy()
        best_u = np.zeros(states.size, dtype=np.int64)
        for u in range(1, nU):                              # first minimum: a later control replaces only when strictly smaller
            take = tot[:, u] < best
            best = np.where(take, tot[:, u], best)
            best_u = np.where(take, u, best_u)
        return best.astype(sp.j_dtype), (label_of_visit[best_u] + sp.index_base).astype(sp.idx_np_dtype)

    def sweep(self, n_stages, states=None):
        """n_stages backups from a zero terminal cost over the whole grid -> list of (J, labels) as computed (first = the
        stage with the reference's index n_stages), each restricted to `states` if given."""
        sp = self.spec
        J = np.zeros(sp.nS, dtype=sp.j_dtype)
        out = []
        for _ in range(n_stages):
            J, lab = self.backup(J)
            out.append((J, lab) if states is None else (J[states], lab[states]))
        return out
