"""Node sets for the disturbed backup (ProblemSpec.disturbance, Backup.set_disturbance; hjbdp.h hjb_set_disturbance).

Both helpers return (offsets [D, W], weights [W] or None) with D = len of their argument: row a is the offset of state
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
