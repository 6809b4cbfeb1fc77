"""Plain float64 restatements of the lookup, probe and fill kernels' operations, for the tests (no oracle import):
what each kernel computes, written the obvious way, with the tolerance each comparison allows."""
from __future__ import annotations

import numpy as np


def nearest_ref(knots, V, pts):
    """griddedInterpolant 'nearest' in float64: per axis the nearer knot of the enclosing cell (clamped to the edge
    cells outside the grid), the upper one at an exact midpoint.  Also returns a mask of the points that lie within
    two units in the last place of `dtype(pts)` of a midpoint on some axis: there a rounded distance may tip either way."""
    pts = np.asarray(pts)
    ulp = np.spacing(np.abs(pts).astype(pts.dtype)).astype(np.float64)
    q = pts.astype(np.float64)
    idx, near_mid = [], np.zeros(len(q), dtype=bool)
    for a, k in enumerate(knots):
        k = np.asarray(k, dtype=np.float64)
        i = np.clip(np.searchsorted(k, q[:, a], side="right") - 1, 0, len(k) - 2)
        lo, hi = q[:, a] - k[i], k[i + 1] - q[:, a]
        idx.append(np.where(lo >= hi, i + 1, i))
        near_mid |= np.abs(lo - hi) <= 4 * ulp[:, a]
    return np.asarray(V)[tuple(idx)], near_mid


def linear_ref(knots, V, pts):
    """N-linear interpolation with linear extrapolation in float64 (scipy's RegularGridInterpolator), and per point
    the sum of the absolute corner weights prod_a (|1 - t_a| + |t_a|): the factor by which rounding in the values
    and weights can grow (1 inside the grid, about 2 |t| when extrapolating by t cells)."""
    from scipy.interpolate import RegularGridInterpolator
    kn = [np.asarray(k, dtype=np.float64) for k in knots]
    q = np.asarray(pts, dtype=np.float64).reshape(-1, len(kn))
    ref = RegularGridInterpolator(kn, np.asarray(V, dtype=np.float64), method="linear", bounds_error=False, fill_value=None)(q)
    w = np.ones(len(q))
    for a, k in enumerate(kn):
        i = np.clip(np.searchsorted(k, q[:, a], side="right") - 1, 0, len(k) - 2)
        t = (q[:, a] - k[i]) / (k[i + 1] - k[i])
        w *= np.abs(1.0 - t) + np.abs(t)
    return ref, w


def linear_tol(dtype, D, vmax, w):
    """What N-linear interpolation in `dtype` may differ from float64 by: about (D + 1) roundings per axis of the
    weight, the difference and the fused lerp, each relative to the value scale max|V| times the weight sum w.
    float64: 1e-12 relative; float32: 8 (D + 1) units of float32 rounding."""
    if np.dtype(dtype) == np.float64:
        return 1e-12 * vmax * w
    return 8 * (D + 1) * np.finfo(np.float32).eps * vmax * w


def ordered_sum(arrays, dtype):
    """((a0 + a1) + a2) + ... with every add rounded to `dtype`, left to right."""
    acc = None
    for x in arrays:
        x = np.asarray(x).astype(dtype)
        acc = x if acc is None else (acc + x).astype(dtype)
    return acc


def term_block(term, D, lo, hi, control, dtype):
    """One term's values over the state block [lo, hi) (axis 0 fastest) at one control, shape = the block's extents."""
    ext = tuple(h - l for l, h in zip(lo, hi))
    index = []
    for d in term.dims:
        if d < D:
            shape = [1] * D
            shape[d] = ext[d]
            index.append(np.arange(lo[d], hi[d]).reshape(shape))
        else:
            index.append(np.full([1] * D, control[d - D]))
    data = np.asarray(term.data).astype(dtype)
    return np.broadcast_to(data[tuple(index)], ext) if index else np.broadcast_to(data, ext)


def separable_ref(vecs, dtype, storage):
    """J[i0, i1, ...] = ((v0[i0] + v1[i1]) + ...) in `dtype`, rounded once to `storage`; flattened column-major."""
    D = len(vecs)
    parts = []
    for a, v in enumerate(vecs):
        shape = [1] * D
        shape[a] = len(v)
        parts.append(np.asarray(v, dtype=dtype).reshape(shape))
    full = ordered_sum([np.broadcast_to(p, tuple(len(v) for v in vecs)) for p in parts], dtype)
    return full.astype(storage).reshape(-1, order="F")
