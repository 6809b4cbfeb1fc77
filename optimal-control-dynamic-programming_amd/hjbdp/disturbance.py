"""Node sets for the disturbed backup (ProblemSpec.disturbance, Backup.set_disturbance; hjbdp.h hjb_set_disturbance), and
actuator_nodes: the per-control table of ProblemSpec.control_disturbance / Backup.set_control_disturbance.

The first two helpers return (offsets [D, W], weights [W] or None) with D = len of their argument: row a is the offset of state
axis a, an axis given 0 gets a row of zeros and is not offset at all."""
from __future__ import annotations

import itertools

import numpy as np

from . import _abi


def _product_guard(k, per_axis, extra=0):
    W = per_axis ** k + extra
    if W > _abi.HJB_DIST_MAX_NODES:
        raise ValueError("%d axes x %d nodes per axis = %d nodes: more than the %d one disturbance holds"
                         % (k, per_axis, W, _abi.HJB_DIST_MAX_NODES))
    return W


def gaussian_nodes(sigma, order=3):
    """Independent zero-mean Gaussian noise of standard deviation sigma[a] on every axis with sigma[a] > 0: the tensor
    product of `order`-point Gauss-Hermite rules (exact for polynomials up to degree 2 * order - 1 per axis), weights
    normalised in float64.  For mode "expect"."""
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(sigma)) or np.any(sigma < 0):
        raise ValueError("sigma must be finite and non-negative")
    order = int(order)
    if order < 1:
        raise ValueError("order must be at least 1")
    active = [a for a in range(sigma.size) if sigma[a] > 0]
    W = _product_guard(len(active), order)
    x, w = np.polynomial.hermite_e.hermegauss(order)      # weight exp(-x^2 / 2): the nodes are in units of sigma
    off = np.zeros((sigma.size, W))
    wts = np.ones(W)
    for i, combo in enumerate(itertools.product(range(order), repeat=len(active))):
        for a, j in zip(active, combo):
            off[a, i] = sigma[a] * x[j]
            wts[i] *= w[j]
    return off, wts / wts.sum()


def box_nodes(delta, centre=True):
    """The 2^k corners of the box |d_a| <= delta[a] over the k axes with delta[a] > 0, and its centre: an N-linear
    interpolant takes its extrema over a box inside one cell at the corners.  For mode "worst" (weights None)."""
    delta = np.asarray(delta, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(delta)) or np.any(delta < 0):
        raise ValueError("delta must be finite and non-negative")
    active = [a for a in range(delta.size) if delta[a] > 0]
    W = _product_guard(len(active), 2, 1 if centre else 0)
    off = np.zeros((delta.size, W))
    first = 1 if centre else 0                            # the centre first: the nominal next state is node 0
    for i, signs in enumerate(itertools.product((-1.0, 1.0), repeat=len(active))):
        for a, s in zip(active, signs):
            off[a, first + i] = s * delta[a]
    return off, None


def actuator_nodes(B, u_table, eps, weights=None, base=None):
    """The per-control node table of an actuator that delivers u * (1 + eps_w) instead of u:
        x+ = ... + B (u o (1 + eps_w))   =>   d_w(l) = B @ (u_table[l] * eps[w])
    B [D, n_u]; u_table [nU, n_u] (or [nU] with one input), row l = the control with 0-based column-major label l; eps [W], one
    relative error for every input, or [W, n_u]; base: an optional additive node set [D, W] (as gaussian_nodes / box_nodes give it)
    added to every control's nodes.  Computed in float64.  Returns (offsets [D, W, nU], weights as given) - what
    ProblemSpec(control_disturbance=...) and Backup.set_control_disturbance take.  The zero control's nodes are all zero: it is
    noise-free, and a larger control is more uncertain."""
    B = np.array(B, dtype=np.float64, ndmin=2)
    u = np.array(u_table, dtype=np.float64)
    if u.ndim == 1:
        u = u[:, None]
    if B.ndim != 2 or u.ndim != 2 or B.shape[1] != u.shape[1]:
        raise ValueError("B must be [D, n_u] and u_table [nU, n_u], got %r and %r" % (B.shape, u.shape))
    e = np.array(eps, dtype=np.float64)
    if e.ndim == 1:
        e = np.repeat(e[:, None], u.shape[1], axis=1)
    if e.ndim != 2 or e.shape[1] != u.shape[1] or e.shape[0] < 1:
        raise ValueError("eps must be [W] or [W, n_u=%d], got %r" % (u.shape[1], e.shape))
    W = e.shape[0]
    if W > _abi.HJB_DIST_MAX_NODES:
        raise ValueError("%d nodes: more than the %d one disturbance holds" % (W, _abi.HJB_DIST_MAX_NODES))
    if not (np.all(np.isfinite(B)) and np.all(np.isfinite(u)) and np.all(np.isfinite(e))):
        raise ValueError("B, u_table and eps must be finite")
    off = np.einsum("dk,wlk->dwl", B, u[None, :, :] * e[:, None, :])
    if base is not None:
        b = np.array(base, dtype=np.float64, ndmin=2)
        if b.shape != (B.shape[0], W):
            raise ValueError("base must be [D=%d, W=%d], got %r" % (B.shape[0], W, b.shape))
        off = off + b[:, :, None]
    return off, weights
