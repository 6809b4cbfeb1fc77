"""Thin host binding of libhjbdp (include/hjbdp.h) - the only way the host
classes reach the GPU.  There is NO CPU fallback: if the shared library is
missing, or no HIP device is visible, every compute call raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import _abi
from .problem import ProblemSpec, check_control_disturbance, check_disturbance

_LIB = None
LIB_PATH = Path(__file__).resolve().parent / "libhjbdp.so"


class HjbError(RuntimeError):
    def __init__(self, status, text):
        super().__init__("libhjbdp: %s (status %d)" % (text, status))
        self.status = status


def _share_torch_hip_runtime():
    """If PyTorch-ROCm is installed, map ITS bundled libamdhip64 (same soname,
    libamdhip64.so.7) before libhjbdp so the process has one HIP runtime: torch
    tensors, torch streams and RCCL then share a context with our kernels.  With
    ROCm's copy loaded first, a later `import torch` finds no GPU.  No torch
    installed -> the system ROCm runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
        if cand.exists():
            C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
    except OSError:
        pass


def load_library(path=None):
    """Load libhjbdp.so (built in-tree by __graft_entry__.build()).  Loading needs
    no GPU; raises if the file is missing - the product never falls back."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = Path(path) if path else Path(os.environ.get("HJBDP_LIB", LIB_PATH))
    if not p.exists():
        raise FileNotFoundError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). libhjbdp has no CPU fallback." % p)
    _share_torch_hip_runtime()
    lib = _abi.bind(C.CDLL(str(p)))
    if path is None:
        _LIB = lib
    return lib


def device_count():
    return int(load_library().hjb_device_count())


def _check(lib, handle, st):
    if st != _abi.HJB_OK:
        msg = lib.hjb_last_error(handle)
        raise HjbError(st, (msg or b"").decode() or lib.hjb_status_string(st).decode())


def policy_lookup(knots, values, points, method="nearest", device=0):
    """Batched griddedInterpolant(knots, values, method) at `points` [nq, D] on the GPU
    (hjb_policy_lookup).  values.dtype (float32/float64) is the arithmetic type: with float32 the knots and the
    points are rounded to float32 and 'nearest' compares the distances in float32 (NearestPolicy.lookup_many does
    not: it follows the host's float64 rule)."""
    lib = load_library()
    values = np.asarray(values)
    dt = values.dtype if values.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    D = len(knots)
    V = np.ascontiguousarray(np.asarray(values, dtype=dt).reshape(-1, order="F"))
    Q = np.ascontiguousarray(np.asarray(points, dtype=dt).reshape(-1, D))
    nq = Q.shape[0]
    ks = [np.ascontiguousarray(k, dtype=np.float64) for k in knots]
    n = (C.c_int32 * D)(*[len(k) for k in ks])
    kp = (C.POINTER(C.c_double) * D)(*[k.ctypes.data_as(C.POINTER(C.c_double)) for k in ks])
    out = np.empty(nq, dtype=dt)
    meth = {"nearest": _abi.HJB_LOOKUP_NEAREST, "linear": _abi.HJB_LOOKUP_LINEAR}[method]
    st = lib.hjb_policy_lookup(int(device), _abi.HJB_F32 if dt == np.float32 else _abi.HJB_F64, D, n, kp,
                               V.ctypes.data, nq, Q.ctypes.data, meth, out.ctypes.data)
    _check(lib, None, st)
    return out


_IDX_OF_DTYPE = {np.dtype(np.uint8): _abi.HJB_IDX_U8, np.dtype(np.uint16): _abi.HJB_IDX_U16, np.dtype(np.int32): _abi.HJB_IDX_I32}


def _f64p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _i32p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _ptr(x):
    """A device pointer as the library takes it: of a torch tensor, a DeviceBuffer or an integer; None stays None (a null pointer)."""
    if x is None:
        return None
    return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x)


def _stream(s):
    """A HIP stream handle as the library takes it: 0 is the null pointer."""
    return int(s) or None


def _j_vector(J, dtype, size, what):
    """J_next or a terminal cost as the library reads it: a flat Fortran-order vector of `dtype`, refused when it does not have
    `size` elements (None: any size).  what: "J_next" or "terminal", which of the two refusals."""
    v = np.ascontiguousarray(np.asarray(J, dtype=dtype).reshape(-1, order="F"))
    if size is not None and v.size != size:
        raise ValueError("terminal cost must have nS elements" if what == "terminal"
                         else "J_next has %d elements, the handle's J layout has %d" % (v.size, size))
    return v


class _Handle:
    """The lifetime and the errors of an object that owns one library handle (Rollout, Backup, MultiBackup, RankSlab).  A
    subclass states three facts: the attribute that holds its handle, and the library's destroy and last-error functions."""
    _handle = _destroy = _last_error = None

    def _raise(self, st):
        h = getattr(self, self._handle)
        msg = getattr(self.lib, self._last_error)(h if h.value else None)
        raise HjbError(st, (msg or b"").decode() or self.lib.hjb_status_string(st).decode())

    def _check(self, st):
        if st != _abi.HJB_OK:
            self._raise(st)

    def _created(self, st):
        """The status of the create call: a failure leaves a null handle and raises the error the library keeps for no object."""
        if st != _abi.HJB_OK:
            setattr(self, self._handle, C.c_void_p())
            self._raise(st)

    def close(self):
        h = getattr(self, self._handle, None)
        if h and h.value:
            getattr(self.lib, self._destroy)(h)
            setattr(self, self._handle, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---- the marshalling of the rollout entry points (pure numpy): each run* is the starts, the planes, the outputs, one library
# call, the dict -------------------------------------------------------------------------------------------------------------
def _f64_vec(v, m):
    """v as m contiguous doubles; None stays None (the library's "not given")."""
    return None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(m))


def _f64_colmajor(v, r, c):
    """v as an [r, c] matrix of doubles laid out column-major, flat; None stays None."""
    return None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(r, c).reshape(-1, order="F"))


def _starts(X0, rows):
    """The initial states as the library reads them: [n_traj, rows] C-contiguous float64 = [rows, n_traj] column-major.  A 1-D
    X0 is one start."""
    X = np.asarray(X0, dtype=np.float64)
    return np.ascontiguousarray((X.reshape(rows, 1) if X.ndim == 1 else X).reshape(rows, -1).T)


def _int32_vector(values, name, n_traj=None):
    """values as a contiguous int32 vector, refused when an element does not fit.  n_traj None: flattened as it comes (a list of
    planes).  n_traj given: one value per trajectory - None stays None, integer types only, a scalar or one element broadcasts."""
    if values is None and n_traj is not None:
        return None
    a = np.asarray(values)
    if n_traj is None:
        a = a.reshape(-1)
    else:
        if a.dtype.kind not in "iu":
            raise TypeError("%s must be integers, got %s" % (name, a.dtype))
        a = np.broadcast_to(a.reshape(-1) if a.ndim else a, (n_traj,))
    if a.size and (a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max):
        raise ValueError("%s does not fit int32" % name)
    return np.ascontiguousarray(a, dtype=np.int32)


def _path_buffers(nt, keep_path, *specs):
    """The optional per-step outputs of a run, specs = (name, rows, cols) each.  Returns (flat, views): flat the buffers to hand
    to the library in the order given (every one None without keep_path), views {name: the same memory as [nt, rows, cols] in
    Fortran order, or None}, valid once the call has filled them."""
    flat = [np.empty(nt * rows * cols) if keep_path else None for _, rows, cols in specs]
    return flat, {name: None if a is None else a.reshape((nt, rows, cols), order="F") for (name, rows, cols), a in zip(specs, flat)}


def _value_planes(J, nS):
    """Value planes as the library reads them: (flat float32 or float64 vector in Fortran order, its HJB_F32 / HJB_F64).  Any
    other floating type is refused (float16: convert first), as is a size that is not a whole number of nS-state planes."""
    v = np.asarray(J)
    if v.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("value planes must be float32 or float64, got %s" % v.dtype)
    v = np.ascontiguousarray(v.reshape(-1, order="F"))
    if nS < 1 or v.size == 0 or v.size % nS:
        raise ValueError("values: %d elements are not a whole number of %d-state planes" % (v.size, nS))
    return v, (_abi.HJB_F32 if v.dtype == np.float32 else _abi.HJB_F64)


_LOOKUP = {"nearest": _abi.HJB_LOOKUP_NEAREST, "linear": _abi.HJB_LOOKUP_LINEAR}
_DIST_MODE = {"expect": _abi.HJB_DIST_EXPECT, "worst": _abi.HJB_DIST_WORST}
_ATT_INTEGRATOR = {"taylor": _abi.HJB_ATT_TAYLOR, "RK4": _abi.HJB_ATT_RK4, "rk4": _abi.HJB_ATT_RK4}
# the per-step outputs of the 7-state and the 13-state loops: (name, rows, stages - n_steps), as Rollout._run reads them
_ATT_PATHS = (("X_path", 7, 1), ("U_path", 3, 0), ("A_path", 3, 0))
_PA_PATHS = (("X_path", 13, 1), ("F_path", 12, 0), ("FM_path", 6, 0))


class Rollout(_Handle):
    """A stored per-stage policy resident on one GPU, for batched fixed-step closed-loop rollouts (hjb_rollout_*):

        with Rollout(knots, labels, u_table, index_base=1) as ro:
            ro.set_model(A, B, c=None, q=None, r=None)
            out = ro.run(X0, plane_of_step, method="linear", keep_path=False)

    knots: D grid vectors.  labels: the argmin labels of n_planes stages, nS states each, column-major (hjb_solve's
    idx_stages, e.g. [n_1, .., n_D, n_planes] or [nS, n_planes]) in uint8, uint16 or int32.  u_table: [n_labels, n_u] (n_u <= 4)
    controls per label.  Step k of a trajectory looks plane plane_of_step[k] up at x ('nearest' / 'linear', bit-identical to
    policy_lookup in float64 on the dense values u_table[labels[:, p] - index_base]), adds the stage cost
    x'diag(q)x + u'diag(r)u and steps x <- A x + B u + c.  X0: [D, n_traj].  run returns X_final [D, n_traj], cost [n_traj],
    X_path [n_traj, D, n_steps+1] and U_path [n_traj, n_u, n_steps] (None unless keep_path) and device_ms.

    The loops that take one policy per channel (pos-att, position, simplified attitude) are a model set on the first of several
    Rollout objects: Rollout.open_channels opens and closes such a set."""

    _handle, _destroy, _last_error = "_ro", "hjb_rollout_destroy", "hjb_rollout_last_error"

    def __init__(self, knots, labels, u_table, index_base=1, device=0):
        self.lib = load_library()
        self._ro = C.c_void_p()
        self._pa_steps = self._pos_steps = 0              # the stages the pos-att / position model set last covers
        ks = [np.ascontiguousarray(k, dtype=np.float64).reshape(-1) for k in knots]
        self.D = len(ks)
        self.n = [len(k) for k in ks]
        nS = int(np.prod(self.n, dtype=np.int64)) if ks else 1
        lab = np.asarray(labels)
        if lab.dtype not in _IDX_OF_DTYPE:
            if lab.dtype.kind not in "iu":
                raise TypeError("labels must be integers (uint8, uint16 or int32), got %s" % lab.dtype)
            if lab.size and (lab.min() < np.iinfo(np.int32).min or lab.max() > np.iinfo(np.int32).max):
                raise ValueError("labels do not fit int32")
            lab = lab.astype(np.int32)
        lab = np.ascontiguousarray(lab.reshape(-1, order="F"))
        if nS < 1 or lab.size % nS or lab.size == 0:
            raise ValueError("labels: %d elements are not a whole number of %d-state planes" % (lab.size, nS))
        self.n_planes = lab.size // nS
        self.labels_dtype = lab.dtype
        ut = np.asarray(u_table, dtype=np.float64)
        ut = ut.reshape(-1, 1) if ut.ndim == 1 else ut
        self.n_labels, self.n_u = ut.shape
        ut = np.ascontiguousarray(ut.reshape(-1, order="F"))
        kcat = np.ascontiguousarray(np.concatenate(ks) if ks else np.zeros(0))
        n = (C.c_int32 * max(self.D, 1))(*self.n)
        self._keep = (kcat, lab, ut)
        st = self.lib.hjb_rollout_create(int(device), self.D, n, _f64p(kcat), _IDX_OF_DTYPE[lab.dtype], int(index_base),
                                         int(self.n_planes), lab.ctypes.data, int(self.n_labels), int(self.n_u), _f64p(ut),
                                         C.byref(self._ro))
        self._keep = None
        self._created(st)
        self.device = int(device)

    @classmethod
    @contextlib.contextmanager
    def open_channels(cls, channels, device=0, index_base=1, label_dtype=None):
        """with Rollout.open_channels(channels) as ros: one Rollout per (knots, labels, table) of `channels`, in order, on one
        device (label_dtype: the labels cast to it first).  All that were created are closed on the way out, also when a later
        one cannot be created.  The model goes on ros[0]: ros[0].set_pos_att_model(ros[1], ros[2], ...)."""
        ros = []
        try:
            for knots, labels, table in channels:
                if label_dtype is not None:
                    labels = np.asarray(labels).astype(label_dtype, copy=False)
                ros.append(cls(knots, labels, table, index_base=index_base, device=device))
            yield ros
        finally:
            for ro in ros:
                ro.close()

    def set_option(self, key, value):
        """hjb_rollout_set_option.  "chunk" (default 2^20): trajectories per launch, which bounds the device memory of a run.
        "lds" (default 1): 1 stages knots, 1/dx and u_table in LDS when they fit 32 KiB; 0 never stages, so every run_* of this
        object reads them from global memory (same bits).  Any other key or value raises HjbError (HJB_E_INVALID)."""
        self._check(self.lib.hjb_rollout_set_option(self._ro, key.encode(), int(value)))

    def set_model(self, A, B, c=None, q=None, r=None):
        D, nu = self.D, self.n_u
        self._check(self.lib.hjb_rollout_set_model(self._ro, _f64p(_f64_colmajor(A, D, D)), _f64p(_f64_colmajor(B, D, nu)),
                                                   _f64p(_f64_vec(c, D)), _f64p(_f64_vec(q, D)), _f64p(_f64_vec(r, nu))))

    def run(self, X0, plane_of_step, method="linear", keep_path=False):
        return self._run(self.lib.hjb_rollout_run, (_LOOKUP[method],), X0, self.D, plane_of_step, "plane_of_step", keep_path,
                         (("X_path", self.D, 1), ("U_path", self.n_u, 0)))

    def set_noise(self, offsets, weights=None):
        """A node set for run_noisy (hjb_rollout_set_noise): offsets [D, W] (row a: the additive offsets of state axis a), weights
        [W] non-negative with a positive sum, or None = equal - what Backup.set_disturbance takes, so one node set serves the
        solve, the policy's price and the flight.  A property of the object, independent of the model; run and every other run_*
        do not read it."""
        off, w, _ = check_disturbance(self.D, offsets, weights, "expect")
        offc = np.ascontiguousarray(off.reshape(-1, order="F"))
        self._check(self.lib.hjb_rollout_set_noise(self._ro, off.shape[1], _f64p(offc), _f64p(w)))

    def clear_noise(self):
        """Detach the node set (hjb_rollout_set_noise with n_nodes = 0)."""
        self._check(self.lib.hjb_rollout_set_noise(self._ro, 0, None, None))

    def run_noisy(self, X0, plane_of_step, seed=0, first_stream=0, method="linear", keep_path=False):
        """run under the node set of set_noise (hjb_rollout_run_noisy): after every step's affine update a node w is drawn and
        offsets[:, w] added on the axes that have an offset.  Trajectory i of the call reads the Philox4x32-10 stream
        first_stream + i under `seed` (both unsigned 64-bit; chunking does not change a bit).  Returns run's dict plus W_path
        [n_traj, n_steps] int32, the drawn nodes (None unless keep_path)."""
        return self._run(self.lib.hjb_rollout_run_noisy, (_LOOKUP[method],), X0, self.D, plane_of_step, "plane_of_step", keep_path,
                         (("X_path", self.D, 1), ("U_path", self.n_u, 0), ("W_path", 1, 0)),
                         mid=(int(seed) & (2 ** 64 - 1), int(first_stream)))

    def run_campaign(self, X0, plane_of_step, n_samples, seed=0, first_stream=0, method="linear", cost_threshold=None,
                     settle_tol=None, hist=None):
        """Every start of X0 [D, n_starts] flown n_samples times under the node set of set_noise, the costs reduced per start on
        the GPU (hjb_rollout_run_campaign): sample m of start s is run_noisy's trajectory on stream first_stream + s * n_samples
        + m of `seed`, and nothing of length n_starts * n_samples exists on either side.  cost_threshold: a scalar or one value
        per start (n_exceed counts the samples with cost > threshold); settle_tol: a scalar or one value per axis (a sample
        settled when |x_final| <= tol on every axis).  Returns the dict of campaign_reduce plus device_ms.
        hist = (lo, hi, n_bins), lo and hi scalars or one value per start: the same flights with a histogram of every start's
        costs beside the statistics (hjb_rollout_run_campaign_hist; the bin rule: campaign_hist_reduce); the dict gains hist
        [n_starts, n_bins + 2] int64 (underflow, the bins, overflow), hist_lo and hist_hi, and its stats are the plain call's
        bits.  hist=None is the plain call."""
        ps = _int32_vector(plane_of_step, "plane_of_step")
        fn = self.lib.hjb_rollout_run_campaign if hist is None else self.lib.hjb_rollout_run_campaign_hist
        return self._campaign(fn, (_LOOKUP[method], int(ps.size), _i32p(ps)), X0, n_samples, seed, first_stream, cost_threshold,
                              settle_tol, hist=hist)

    def _run(self, fn, lead, X0, width, planes, plane_name, keep_path, paths, inputs=(), mid=(), cost="cost", flag=None, flag_last=False,
             null=(), ms=True):
        """The one path of the run calls: fn(handle, *lead, n_steps, planes, n_traj, X0, *inputs, *mid, X_final, [cost,] [flag,]
        *paths, [flag,] [device_ms]) and the dict of its outputs.  lead: what the entry point has in front of n_steps - its method
        or fly_noise; inputs: (values, name) int32 per trajectory; mid: the scalars in front of X_final; paths: (name, rows,
        stages - n_steps) each, the ones in `null` never asked for; cost, flag: the keys of the [n_traj] double and int32
        outputs (None: the entry point has none), the flag behind the paths with flag_last."""
        X = _starts(X0, width)
        nt = X.shape[0]
        ps = _int32_vector(planes, plane_name)
        K = int(ps.size)
        ins = [_int32_vector(v, name, nt) for v, name in inputs]
        Xf = np.empty((nt, width))
        vecs = {key: a for key, a in ((cost, np.empty(nt)), (flag, np.full(nt, -1, np.int32))) if key is not None}
        flat, views = _path_buffers(nt, keep_path, *((name, rows, K + more) for name, rows, more in paths))
        for name in null:
            flat[[p[0] for p in paths].index(name)], views[name] = None, None
        f = [_i32p(vecs[flag])] if flag else []
        ms = [C.c_double(0.0)] if ms else []
        self._check(fn(self._ro, *lead, K, _i32p(ps), nt, _f64p(X), *map(_i32p, ins), *mid, _f64p(Xf), *([_f64p(vecs[cost])] if cost else []),
                       *([] if flag_last else f), *map(_f64p, flat), *(f if flag_last else []), *map(C.byref, ms)))
        for name, dtype in (("L_path", np.int32), ("V_path", None), ("W_path", np.int32)):     # the one-row paths: [n_traj, n_steps]
            if views.get(name) is not None:
                views[name] = views[name][:, 0, :] if dtype is None else views[name][:, 0, :].astype(dtype)
        return {"X_final": Xf.T, **vecs, **views, **{"device_ms": m.value for m in ms}}

    def _campaign(self, fn, lead, X0, n_samples, seed, first_stream, cost_threshold, settle_tol, hist=None, pair=False):
        """The one path of the campaign calls: fn(handle, *lead, n_starts, n_samples, X0, seed, first_stream, threshold, tol,
        [lo, hi, n_bins,] stats [x 3 for a pair], [hist,] device_ms) and the dict of its records.  lead: what the entry point
        has in front of n_starts - its method, its planes and their count, or the pair's two sides."""
        X = _starts(X0, self.D)
        ns, M = X.shape[0], int(n_samples)
        thr, tol = _campaign_bounds(ns, self.D, cost_threshold, settle_tol)
        stats = [np.empty((ns, _abi.HJB_CAMPAIGN_NSTAT)) for _ in range(3 if pair else 1)]
        bins, counts, extra = (), (), {}
        if hist is not None:
            lo, hi, nb, cnt = _campaign_hist_args(ns, hist)
            bins, counts, extra = (_f64p(lo), _f64p(hi), nb), (_i64p(cnt),), {"hist": cnt, "hist_lo": lo, "hist_hi": hi}
        ms = C.c_double(0.0)
        self._check(fn(self._ro, *lead, ns, M, _f64p(X), int(seed) & (2 ** 64 - 1), int(first_stream), _f64p(thr), _f64p(tol), *bins,
                       *map(_f64p, stats), *counts, C.byref(ms)))
        if pair:
            return {"a": _campaign_dict(stats[0], M), "b": _campaign_dict(stats[1], M), **_campaign_pair_dict(stats[2], M),
                    "device_ms": ms.value}
        return {**_campaign_dict(stats[0], M), **extra, "device_ms": ms.value}

    def set_values(self, J):
        """Value planes for run_greedy (hjb_rollout_set_values): J float32 or float64, [nS, n_planes] or grid-shaped with a
        trailing plane axis, Fortran order (hjb_solve's J_stages; Dynamic_Solver's J_star).  A property of the object,
        independent of the model and of the labels; run and every other run_* do not read it."""
        nS = int(np.prod(self.n, dtype=np.int64))
        v, dtype = _value_planes(J, nS)
        self._check(self.lib.hjb_rollout_set_values(self._ro, dtype, v.size // nS, v.ctypes.data))
        self.n_value_planes = v.size // nS

    def clear_values(self):
        """Detach the value planes (hjb_rollout_set_values with n_planes = 0)."""
        self._check(self.lib.hjb_rollout_set_values(self._ro, _abi.HJB_F64, 0, None))
        self.n_value_planes = 0

    def run_greedy(self, X0, value_plane_of_step, keep_path=False):
        """The affine model flown by one-step lookahead on the planes of set_values (hjb_rollout_run_greedy): at every step the
        row of u_table that minimises g(x, u) + J(A x + B u + c), J the plane value_plane_of_step[k] blended N-linearly at the
        next state (-1: the zero function), first minimum.  The labels of the object are not read.  Returns run's dict plus
        L_path [n_traj, n_steps] int32, the chosen labels (index_base added), and V_path [n_traj, n_steps], the minima - the
        cost-to-go the controller believed (both None unless keep_path)."""
        return self._run(self.lib.hjb_rollout_run_greedy, (), X0, self.D, value_plane_of_step, "value_plane_of_step", keep_path,
                         (("X_path", self.D, 1), ("U_path", self.n_u, 0), ("L_path", 1, 0), ("V_path", 1, 0)))

    def set_lookahead(self, offsets, weights=None, mode="expect"):
        """A lookahead node set for run_lookahead (hjb_rollout_set_lookahead): what Backup.set_disturbance takes - offsets [D, W],
        weights [W] (mode "expect" only; None = 1 / W each; used as given, not normalised), mode "expect" or "worst".  It is
        what the controller believes; set_noise's set is the plant, and the two may differ.  run_lookahead alone reads it."""
        off, w, mode = check_disturbance(self.D, offsets, weights, mode)
        offc = np.ascontiguousarray(off.reshape(-1, order="F"))
        self._check(self.lib.hjb_rollout_set_lookahead(self._ro, _DIST_MODE[mode], off.shape[1], _f64p(offc), _f64p(w)))

    def clear_lookahead(self):
        """Detach the lookahead node set (hjb_rollout_set_lookahead with n_nodes = 0)."""
        self._check(self.lib.hjb_rollout_set_lookahead(self._ro, _abi.HJB_DIST_EXPECT, 0, None, None))

    def run_lookahead(self, X0, value_plane_of_step, noisy=False, seed=0, first_stream=0, keep_path=False):
        """run_greedy with the disturbed backup inside every candidate (hjb_rollout_run_lookahead): at every step the row of
        u_table that minimises g(x, u) + E_w J(A x + B u + c + e_w) (or max_w) over set_lookahead's nodes, J the plane
        value_plane_of_step[k] of set_values (-1: the zero function).  noisy=False flies the nominal plant (seed and first_stream
        are not read); noisy=True flies run_noisy's plant under set_noise's nodes, trajectory i on the stream first_stream + i
        of `seed`.  Returns run_greedy's dict plus W_path [n_traj, n_steps] int32, the drawn nodes (None unless noisy and
        keep_path)."""
        return self._run(self.lib.hjb_rollout_run_lookahead, (1 if noisy else 0,), X0, self.D, value_plane_of_step, "value_plane_of_step",
                         keep_path, (("X_path", self.D, 1), ("U_path", self.n_u, 0), ("L_path", 1, 0), ("V_path", 1, 0), ("W_path", 1, 0)),
                         mid=(int(seed) & (2 ** 64 - 1), int(first_stream)), null=() if noisy else ("W_path",))

    def run_lookahead_campaign(self, X0, value_plane_of_step, n_samples, seed=0, first_stream=0, cost_threshold=None, settle_tol=None):
        """run_campaign for run_lookahead's controller (hjb_rollout_run_lookahead_campaign): every start of X0 [D, n_starts] flown
        n_samples times by the lookahead on set_values' planes under set_lookahead's nodes, on the plant of set_noise, the costs
        reduced per start on the GPU.  Sample m of start s is run_lookahead(noisy=True)'s trajectory on stream first_stream +
        s * n_samples + m of `seed` - the stream run_campaign gives that sample, so the two campaigns of one seed, first_stream
        and n_samples fly common random numbers and their per-start means can be differenced with the sampling noise largely
        cancelled.  cost_threshold, settle_tol and the returned dict: run_campaign's.  With a histogram of every start's costs
        beside the statistics: run_lookahead_campaign_hist."""
        ps = _int32_vector(value_plane_of_step, "value_plane_of_step")
        return self._campaign(self.lib.hjb_rollout_run_lookahead_campaign, (int(ps.size), _i32p(ps)), X0, n_samples, seed, first_stream,
                              cost_threshold, settle_tol)

    def run_lookahead_campaign_hist(self, X0, value_plane_of_step, n_samples, hist, seed=0, first_stream=0, cost_threshold=None,
                                    settle_tol=None):
        """run_lookahead_campaign with a histogram of every start's costs beside the statistics
        (hjb_rollout_run_lookahead_campaign_hist): hist = (lo, hi, n_bins) and the returned dict as run_campaign(hist=...) has
        them, the flights, the streams (common random numbers with run_campaign) and the stats run_lookahead_campaign's."""
        ps = _int32_vector(value_plane_of_step, "value_plane_of_step")
        return self._campaign(self.lib.hjb_rollout_run_lookahead_campaign_hist, (int(ps.size), _i32p(ps)), X0, n_samples, seed,
                              first_stream, cost_threshold, settle_tol, hist=hist)

    def run_campaign_pair(self, X0, a, b, n_samples, seed=0, first_stream=0, cost_threshold=None, settle_tol=None):
        """Two controllers a and b on this object's plant (the affine model under set_noise's nodes), every start of X0
        [D, n_starts] flown n_samples times by each on the plain campaigns' streams - sample m of start s on stream first_stream +
        s * n_samples + m under both - and the per-sample cost difference d = cost_b - cost_a reduced per start on the GPU
        (hjb_rollout_run_campaign_pair): the variance of d holds the pairing that two separately reduced records do not.  A
        controller is ("labels", plane_of_step, method) - run_campaign's - or ("lookahead", value_plane_of_step) -
        run_lookahead_campaign's, under set_lookahead's nodes - or ("greedy", value_plane_of_step): the lookahead under one
        zero node of weight 1, whatever set_lookahead holds.  Returns campaign_pair_reduce's dict with a and b the plain
        campaigns' dicts (their bits) and device_ms; a negative difference means b paid less."""
        (ka, ma, pa), (kb, mb, pb) = _pair_side(a, "a"), _pair_side(b, "b")
        if pa.size != pb.size:
            raise ValueError("a and b: %d and %d steps" % (pa.size, pb.size))
        return self._campaign(self.lib.hjb_rollout_run_campaign_pair, (ka, ma, _i32p(pa), kb, mb, _i32p(pb), int(pa.size)), X0, n_samples,
                              seed, first_stream, cost_threshold, settle_tol, pair=True)

    def set_attitude_model(self, inertia, h, integrator="taylor", q=None, r=None):
        """The 6-D attitude loop instead of the affine one (hjb_rollout_set_attitude_model; the last model set wins):
        inertia = (J1, J2, J3), step h, integrator 'taylor' or 'RK4', stage-cost weights q [7] and r [3] (None: zeros).
        Needs D = 6 axes in the order (w1, w2, w3, yaw, pitch, roll) and n_u = 3."""
        self._check(self.lib.hjb_rollout_set_attitude_model(self._ro, _f64p(_f64_vec(inertia, 3)), float(h), _ATT_INTEGRATOR[integrator],
                                                            _f64p(_f64_vec(q, 7)), _f64p(_f64_vec(r, 3))))

    def run_attitude(self, X0, plane_of_step, method="nearest", keep_path=False):
        """hjb_rollout_run_attitude: X0 [7, n_traj] (X = [w1 w2 w3 q1 q2 q3 q4], q4 scalar).  Returns X_final [7, n_traj],
        cost [n_traj], X_path [n_traj, 7, n_steps+1], U_path [n_traj, 3, n_steps], A_path [n_traj, 3, n_steps] (the yaw, pitch,
        roll in radians each step looked up at; the paths None unless keep_path) and device_ms."""
        return self._run(self.lib.hjb_rollout_run_attitude, (_LOOKUP[method],), X0, 7, plane_of_step, "plane_of_step", keep_path,
                         _ATT_PATHS)

    def set_pos_att_model(self, rollout_y, rollout_z, inertia, mass, t_dist, h, rsw2eci, orbit_coef, substeps=1):
        """The 13-state pos-att loop (hjb_rollout_set_pos_att_model; the last model set wins) with this object as channel x and
        two more Rollout objects as channels y and z (each D = 4 over (position, velocity, angle, rate), n_u = 4, one device, one
        label type).  inertia [3, 3], rsw2eci [3, 3] and orbit_coef [n_nodes, 5] as hjbdp.rollout.pos_att_orbit_table builds them
        (n_nodes = 2 * substeps * k + 1).  The model keeps what it reads of the other two alive: they may be closed afterwards."""
        J, rsw = _f64_colmajor(inertia, 3, 3), _f64_colmajor(rsw2eci, 3, 3)
        coef = np.ascontiguousarray(np.asarray(orbit_coef, dtype=np.float64).reshape(-1, 5))
        self._check(self.lib.hjb_rollout_set_pos_att_model(self._ro, rollout_y._ro, rollout_z._ro, _f64p(J), float(mass), float(t_dist),
                                                           float(h), int(substeps), _f64p(rsw), int(coef.shape[0]), _f64p(coef)))
        self._pa_steps = (coef.shape[0] - 1) // (2 * int(substeps))

    def run_pos_att(self, X0, plane_of_step=None, keep_path=False):
        """hjb_rollout_run_pos_att: X0 [13, n_traj] (X = [x(3) v(3) q(4) w(3)], q4 scalar).  plane_of_step None: every stage the
        orbit table covers, on plane 0 (stationary policies).  Returns X_final [13, n_traj] and X_path [n_traj, 13, n_steps+1], F_path [n_traj, 12, n_steps]
        (f0..f11), FM_path [n_traj, 6, n_steps] (a_x a_y a_z U_M); the paths None unless keep_path."""
        planes = np.zeros(self._pa_steps, np.int32) if plane_of_step is None else plane_of_step
        return self._run(self.lib.hjb_rollout_run_pos_att, (), X0, 13, planes, "plane_of_step", keep_path, _PA_PATHS, cost=None,
                         ms=False)

    def set_pos_att_fault_controller(self, other):
        """hjb_rollout_set_pos_att_fault_controller: attach `other` (a Rollout with D = 4, n_u = 4 = [f0 f1 f6 f7], this object's
        device and label type, a grid of its own) as the fault controller of channel x to the pos-att model this object holds;
        None detaches.  The model keeps what it reads of `other` alive: it may be closed afterwards.  Setting a model again drops
        the attachment; run_pos_att ignores it."""
        self._check(self.lib.hjb_rollout_set_pos_att_fault_controller(self._ro, None if other is None else other._ro))

    def run_pos_att_faults(self, X0, plane_of_step=None, fault_mask=None, fault_stage=None, switch_stage=None, pos_tol=np.inf,
                           att_tol=np.inf, keep_path=False):
        """hjb_rollout_run_pos_att_faults (K23): run_pos_att with, per trajectory, the thrusters of fault_mask (bit j = thruster j)
        dead in the plant from stage fault_stage on and channel x handed over to the attached fault controller from stage
        switch_stage on.  fault_mask / fault_stage / switch_stage: None (no fault / stage 0 / never), a scalar or [n_traj]; a stage
        >= n_steps never comes.  Returns a dict: X_final [13, n_traj]; impulse [n_traj] = h * sum over stages and thrusters of
        |applied force|; settle_stage [n_traj] (int32): the first state index from which the path stays within pos_tol of the
        origin and |q(1:3)| within att_tol to the end, n_steps + 1 if the last state is outside; X_path, F_path (the APPLIED
        forces), FM_path as run_pos_att's, None unless keep_path; device_ms."""
        planes = np.zeros(self._pa_steps, np.int32) if plane_of_step is None else plane_of_step
        return self._run(self.lib.hjb_rollout_run_pos_att_faults, (), X0, 13, planes, "plane_of_step", keep_path, _PA_PATHS,
                         inputs=((fault_mask, "fault_mask"), (fault_stage, "fault_stage"), (switch_stage, "switch_stage")),
                         mid=(float(pos_tol), float(att_tol)), cost="impulse", flag="settle_stage")

    def set_position_model(self, rollout_y, rollout_z, n_sub, table, tol=1e-8):
        """Solver_position's RKF45 loop (hjb_rollout_set_position_model; the last model set wins) with this object as channel x and
        two more Rollout objects as channels y and z (each D = 2 over (position, velocity), n_u = 1, one device, one label type).
        n_sub [n_steps] and table [n_steps, max_sub, 32] as hjbdp.rollout.position_rkf45_table builds them; tol is rkf45's.  The
        model keeps what it reads of the other two alive: they may be closed afterwards."""
        ns = np.ascontiguousarray(np.asarray(n_sub).reshape(-1).astype(np.int32))
        tab = np.ascontiguousarray(np.asarray(table, dtype=np.float64))
        if tab.ndim != 3 or tab.shape[0] != ns.size or tab.shape[2] != 32:
            raise ValueError("table must be [n_steps, max_sub, 32] with one n_sub per stage, got %r for %d stages" % (tab.shape, ns.size))
        self._check(self.lib.hjb_rollout_set_position_model(self._ro, rollout_y._ro, rollout_z._ro, float(tol), int(ns.size),
                                                            int(tab.shape[1]), _i32p(ns), _f64p(tab)))
        self._pos_steps = int(ns.size)

    def run_position(self, X0, plane_of_step=None, keep_path=False):
        """hjb_rollout_run_position: X0 [6, n_traj] (y = [x(3) v(3)]).  plane_of_step None: every stage the table covers, on plane 0
        (stationary policies).  Returns X_final [6, n_traj], off_schedule [n_traj] (int32: the first stage that left rkf45's
        schedule, -1 if none) and X_path [n_traj, 6, n_steps+1], A_path [n_traj, 3, n_steps]; the paths None unless keep_path."""
        planes = np.zeros(self._pos_steps, np.int32) if plane_of_step is None else plane_of_step
        return self._run(self.lib.hjb_rollout_run_position, (), X0, 6, planes, "plane_of_step", keep_path,
                         (("X_path", 6, 1), ("A_path", 3, 0)), cost=None, ms=False, flag="off_schedule", flag_last=True)

    def set_attitude_simplified_model(self, rollout_2, rollout_3, inertia, h, substeps=1, dynamics="full", qw=None, qt=None, r=None):
        """The simplified attitude loop (hjb_rollout_set_attitude_simplified_model; the last model set wins) with this object as
        channel 1 and two more Rollout objects as channels 2 and 3 (each D = 2 over (w_i, theta_i), n_u = 1, one device, one label
        type).  inertia [3, 3]; dynamics 'full' (full inertia matrix, `substeps` RK4 steps of h / substeps per stage in place of
        the reference's ode45, quaternion not renormalised: max |dX| against a Dormand-Prince stage integrator 4.9e-13 over 5,999
        stages at substeps 1, 1.4e-14 at 2) or 'diagonal' (diag(inertia), one RK4 step, q / |q|: the reference's own arithmetic,
        substeps must be 1).  qw, qt, r [3]: the stage-cost weights on w_i^2, theta_i^2, u_i^2 (None: zeros).  The model keeps what
        it reads of the other two alive: they may be closed afterwards."""
        dyn = {"full": _abi.HJB_ATTS_FULL, "diagonal": _abi.HJB_ATTS_DIAGONAL}[dynamics]
        self._check(self.lib.hjb_rollout_set_attitude_simplified_model(self._ro, rollout_2._ro, rollout_3._ro, _f64p(_f64_colmajor(inertia, 3, 3)),
                                                                       float(h), int(substeps), dyn, _f64p(_f64_vec(qw, 3)),
                                                                       _f64p(_f64_vec(qt, 3)), _f64p(_f64_vec(r, 3))))

    def run_attitude_simplified(self, X0, plane_of_step, keep_path=False):
        """hjb_rollout_run_attitude_simplified: X0 [7, n_traj] (X = [w1 w2 w3 q1 q2 q3 q4], q4 scalar).  Returns X_final [7, n_traj],
        cost [n_traj], X_path [n_traj, 7, n_steps+1], U_path [n_traj, 3, n_steps], A_path [n_traj, 3, n_steps] (the three
        theta_i = 2 asin(q_i) in radians each stage looked up at); the paths None unless keep_path."""
        return self._run(self.lib.hjb_rollout_run_attitude_simplified, (), X0, 7, plane_of_step, "plane_of_step", keep_path, _ATT_PATHS,
                         ms=False)


class ActuatorRollout(Rollout):
    """A Rollout that can also be flown under ACTUATOR noise (hjb_rollout_set_actuator_noise, hjb_rollout_run_actuator,
    hjb_rollout_run_actuator_campaign): the plant delivers u * (1 + eps_w) instead of the commanded u.  Everything Rollout has
    is here unchanged - set_noise, run, run_noisy, run_campaign of an object that holds an actuator set give the bits they gave -
    and the same C object is behind both.  A class of its own because Rollout's set of run methods is a pinned interface
    (tests/test_rollout_run_marshalling.py holds it to its nine); this one's marshalling is tests/test_actuator_rollout_refs.py's."""

    def set_actuator_noise(self, eps, weights=None, base=None):
        """An actuator node set for run_actuator (hjb_rollout_set_actuator_noise): the plant delivers u * (1 + eps_w) instead of
        the commanded u.  eps [W] (one relative error for every input) or [W, n_u] - the shapes actuator_nodes takes; weights [W]
        as set_noise's; base: an optional additive node set [D, W] on the same nodes.  So the set a policy was designed under
        (ProblemSpec(control_disturbance=actuator_nodes(B, u_table, eps, weights, base))) is the set it is flown under.  A property
        of the object, independent of set_noise's set and of the model; run_actuator and run_actuator_campaign alone read it."""
        e = np.array(eps, dtype=np.float64)
        if e.ndim == 1:
            e = np.repeat(e[:, None], self.n_u, axis=1)
        if e.ndim != 2 or e.shape[1] != self.n_u or not (1 <= e.shape[0] <= _abi.HJB_DIST_MAX_NODES):
            raise ValueError("eps must be [W] or [W, n_u=%d] with 1 <= W <= %d, got %r" % (self.n_u, _abi.HJB_DIST_MAX_NODES, e.shape))
        W = e.shape[0]
        b = None
        if base is not None:
            b = np.array(base, dtype=np.float64, ndmin=2)
            if b.shape != (self.D, W):
                raise ValueError("base must be [D=%d, W=%d], got %r" % (self.D, W, b.shape))
            b = np.ascontiguousarray(b.reshape(-1, order="F"))
        w = None
        if weights is not None:
            w = np.array(weights, dtype=np.float64).reshape(-1)
            if w.shape != (W,):
                raise ValueError("weights must be [W=%d], got %r" % (W, w.shape))
        ec = np.ascontiguousarray(e.reshape(-1))              # [W, n_u] row-major is [n_u, W] column-major
        self._check(self.lib.hjb_rollout_set_actuator_noise(self._ro, W, _f64p(ec), _f64p(b), _f64p(w)))

    def clear_actuator_noise(self):
        """Detach the actuator node set (hjb_rollout_set_actuator_noise with n_nodes = 0)."""
        self._check(self.lib.hjb_rollout_set_actuator_noise(self._ro, 0, None, None, None))

    def run_actuator(self, X0, plane_of_step, seed=0, first_stream=0, method="linear", keep_path=False):
        """run under the actuator node set of set_actuator_noise (hjb_rollout_run_actuator): run_noisy's loop, stream numbering
        and sampler, with x+ = A x + B (u (1 + eps_w)) + c + base_w at the drawn node w; the cost is charged on the commanded u.
        Returns run_noisy's dict: U_path holds the commanded controls, W_path the drawn nodes."""
        return self._run(self.lib.hjb_rollout_run_actuator, (_LOOKUP[method],), X0, self.D, plane_of_step, "plane_of_step", keep_path,
                         (("X_path", self.D, 1), ("U_path", self.n_u, 0), ("W_path", 1, 0)),
                         mid=(int(seed) & (2 ** 64 - 1), int(first_stream)))

    def run_actuator_campaign(self, X0, plane_of_step, n_samples, seed=0, first_stream=0, method="linear", cost_threshold=None,
                              settle_tol=None):
        """run_campaign on the plant of set_actuator_noise (hjb_rollout_run_actuator_campaign): sample m of start s is
        run_actuator's trajectory on stream first_stream + s * n_samples + m of `seed`, reduced per start on the GPU; nothing of
        length n_starts * n_samples exists on either side.  Returns the dict of campaign_reduce plus device_ms."""
        ps = _int32_vector(plane_of_step, "plane_of_step")
        return self._campaign(self.lib.hjb_rollout_run_actuator_campaign, (_LOOKUP[method], int(ps.size), _i32p(ps)), X0, n_samples, seed,
                              first_stream, cost_threshold, settle_tol)


class ControlLookaheadRollout(ActuatorRollout):
    """An ActuatorRollout that can also fly the value function of a control-dependent backup directly
    (hjb_rollout_set_control_lookahead, hjb_rollout_run_control_lookahead, hjb_rollout_run_control_lookahead_campaign): one-step
    lookahead with a node set PER CANDIDATE, on the nominal plant or on set_actuator_noise's.  Everything ActuatorRollout has is
    here unchanged, and the same C object is behind all three classes.  A class of its own because the method sets of Rollout and
    ActuatorRollout are pinned interfaces (tests/test_rollout_run_marshalling.py, tests/test_actuator_rollout_refs.py); this one's
    marshalling is tests/test_control_lookahead_refs.py's."""

    def set_control_lookahead(self, offsets, weights=None, mode="expect"):
        """A per-control lookahead node set for run_control_lookahead (hjb_rollout_set_control_lookahead): what
        Backup.set_control_disturbance takes - offsets [D, W, n_labels] (actuator_nodes' table: offsets[:, w, l] is node w of the
        candidate with 0-based label l), weights [W] (mode "expect" only; None = 1 / W each; used as given), mode "expect" or
        "worst".  It is what the controller believes; set_actuator_noise's set is the plant, and the two may differ.  A property of
        its own: set_lookahead's set is neither read nor changed, and run_control_lookahead and its campaign alone read this one."""
        off, w, mode = check_control_disturbance(self.D, (self.n_labels,), offsets, weights, mode)
        offc = np.ascontiguousarray(off.reshape(-1, order="F"))
        self._check(self.lib.hjb_rollout_set_control_lookahead(self._ro, _DIST_MODE[mode], off.shape[1], off.shape[2], _f64p(offc), _f64p(w)))

    def clear_control_lookahead(self):
        """Detach the per-control lookahead node set (hjb_rollout_set_control_lookahead with n_nodes = 0)."""
        self._check(self.lib.hjb_rollout_set_control_lookahead(self._ro, _abi.HJB_DIST_EXPECT, 0, 0, None, None))

    def run_control_lookahead(self, X0, value_plane_of_step, actuator=False, seed=0, first_stream=0, keep_path=False):
        """run_lookahead with a node set per candidate (hjb_rollout_run_control_lookahead): at every step the row l of u_table that
        minimises g(x, u_l) + E_w J(A x + B u_l + c + e_w(l)) (or max_w) over set_control_lookahead's nodes, J the plane
        value_plane_of_step[k] of set_values (-1: the zero function).  actuator=False flies the nominal plant (seed and first_stream
        are not read); actuator=True flies run_actuator's plant under set_actuator_noise's nodes, trajectory i on the stream
        first_stream + i of `seed`, the cost charged on the commanded u.  Returns run_lookahead's dict: U_path the commanded
        controls, W_path [n_traj, n_steps] int32 the drawn nodes (None unless actuator and keep_path)."""
        return self._run(self.lib.hjb_rollout_run_control_lookahead, (1 if actuator else 0,), X0, self.D, value_plane_of_step,
                         "value_plane_of_step", keep_path,
                         (("X_path", self.D, 1), ("U_path", self.n_u, 0), ("L_path", 1, 0), ("V_path", 1, 0), ("W_path", 1, 0)),
                         mid=(int(seed) & (2 ** 64 - 1), int(first_stream)), null=() if actuator else ("W_path",))

    def run_control_lookahead_campaign(self, X0, value_plane_of_step, n_samples, seed=0, first_stream=0, cost_threshold=None,
                                       settle_tol=None):
        """run_lookahead_campaign for run_control_lookahead's controller on the plant of set_actuator_noise
        (hjb_rollout_run_control_lookahead_campaign): sample m of start s is run_control_lookahead(actuator=True)'s trajectory on
        stream first_stream + s * n_samples + m of `seed` - the stream run_actuator_campaign gives that sample, so the stored
        labels and the value function fly common random numbers.  cost_threshold, settle_tol and the returned dict: run_campaign's."""
        ps = _int32_vector(value_plane_of_step, "value_plane_of_step")
        return self._campaign(self.lib.hjb_rollout_run_control_lookahead_campaign, (int(ps.size), _i32p(ps)), X0, n_samples, seed,
                              first_stream, cost_threshold, settle_tol)


def noise_thresholds(weights, n_nodes=None):
    """The sampler's W - 1 thresholds of a weight vector (hjb_rollout_noise_table; no device): weights [W], or None with
    n_nodes = W for equal weights.  Node w is drawn when T[w-1] <= word < T[w] (T[-1] = 0, T[W-1] = 2^32)."""
    lib = load_library()
    w = None if weights is None else np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    W = int(n_nodes) if n_nodes is not None else (0 if w is None else w.size)
    if w is not None and w.size != W:
        raise ValueError("weights: %d values for n_nodes = %d" % (w.size, W))
    T = np.empty(max(W - 1, 0))
    _check(lib, None, lib.hjb_rollout_noise_table(W, _f64p(w), _f64p(T)))
    return T


def noise_draw(thresholds, n_traj, n_steps, seed=0, first_stream=0):
    """The nodes run_noisy draws (hjb_rollout_noise_draw; no device): [n_traj, n_steps] int32, row i from the stream
    first_stream + i under `seed`, for the node set whose thresholds (noise_thresholds) are given (W = len + 1)."""
    lib = load_library()
    T = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    nodes = np.empty((int(n_steps), int(n_traj)), dtype=np.int32)
    _check(lib, None, lib.hjb_rollout_noise_draw(int(seed) & (2 ** 64 - 1), int(first_stream), int(n_traj), int(n_steps), T.size + 1,
                                                 _f64p(T), _i32p(nodes)))
    return np.ascontiguousarray(nodes.T)


def _campaign_bounds(n_starts, D, cost_threshold, settle_tol):
    """cost_threshold (None, a scalar or [n_starts]) and settle_tol (None, a scalar or [D]) as the library reads them"""
    thr = None if cost_threshold is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cost_threshold, dtype=np.float64).reshape(-1),
                                                                                  (n_starts,)))
    tol = None if settle_tol is None else np.ascontiguousarray(np.broadcast_to(np.asarray(settle_tol, dtype=np.float64).reshape(-1), (D,)))
    return thr, tol


def _campaign_dict(stats, M):
    """stats [n_starts, 8] as the library wrote it -> the dict run_campaign and campaign_reduce return"""
    total, sumsq = stats[:, 0], stats[:, 1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        var = np.maximum((sumsq - total * total / M) / (M - 1), 0.0) if M > 1 else np.zeros(stats.shape[0])
        n_settled = stats[:, 6].astype(np.int64)
        mean_settled = np.where(n_settled > 0, stats[:, 7] / np.maximum(n_settled, 1), np.nan)
    return {"stats": stats, "mean": total / M, "var": var, "std": np.sqrt(var), "min": stats[:, 2], "max": stats[:, 3],
            "n_exceed": stats[:, 4].astype(np.int64), "n_left": stats[:, 5].astype(np.int64), "n_settled": n_settled,
            "mean_settled": mean_settled}


def _i64p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))


def _campaign_hist_args(n_starts, hist):
    """hist = (lo, hi, n_bins), lo and hi scalars or [n_starts] -> lo, hi as the library reads them, n_bins and the zeroed output
    [n_starts, n_bins + 2] int64 (the library's [n_bins + 2, n_starts] column-major)"""
    lo, hi, n_bins = hist
    nb = int(n_bins)
    if not 1 <= nb <= _abi.HJB_CAMPAIGN_MAX_BINS:
        raise ValueError("n_bins must lie in 1..%d" % _abi.HJB_CAMPAIGN_MAX_BINS)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64).reshape(-1), (n_starts,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64).reshape(-1), (n_starts,)))
    return lo, hi, nb, np.zeros((n_starts, nb + 2), dtype=np.int64)


def campaign_hist_reduce(cost, n_samples, lo, hi, n_bins):
    """The binning of Rollout.run_campaign(hist=...) on the CPU (hjb_rollout_campaign_hist_reduce; no device): cost
    [n_starts * n_samples] (trajectory s * n_samples + m is sample m of start s), lo and hi scalars or one value per start
    (finite, lo < hi), n_bins in 1..256.  A cost c < lo counts in column 0, one with not c < hi (a NaN too) in column n_bins + 1,
    any other in column 1 + min(n_bins - 1, int((c - lo) * (n_bins / (hi - lo)))).  Returns hist [n_starts, n_bins + 2] int64:
    the counts run_campaign(hist=...) returns for the same samples; every row sums to n_samples."""
    lib = load_library()
    c = np.ascontiguousarray(np.asarray(cost, dtype=np.float64).reshape(-1))
    M = int(n_samples)
    if M < 1 or c.size % M:
        raise ValueError("cost: %d values are not a whole number of %d samples" % (c.size, M))
    ns = c.size // M
    lo, hi, nb, counts = _campaign_hist_args(ns, (lo, hi, n_bins))
    _check(lib, None, lib.hjb_rollout_campaign_hist_reduce(ns, M, _f64p(c), _f64p(lo), _f64p(hi), nb, _i64p(counts)))
    return counts


def _hist_edges(hist, lo, hi):
    h = np.asarray(hist, dtype=np.int64)
    h = h.reshape(1, -1) if h.ndim == 1 else h
    nb = h.shape[1] - 2
    if nb < 1:
        raise ValueError("hist: %d columns are not underflow, at least one bin and overflow" % h.shape[1])
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64).reshape(-1), (h.shape[0],))
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64).reshape(-1), (h.shape[0],))
    return h, nb, lo, hi


def campaign_quantiles(hist, lo, hi, q, cmin=None, cmax=None):
    """Upper bounds of order statistics from campaign histograms (pure numpy).  hist [n_starts, n_bins + 2] as
    run_campaign(hist=...) returns it, lo and hi the ranges it was binned with, q a scalar or a sequence in [0, 1].  With M a
    row's sum and the rank k = max(1, ceil(q * M)), the result [n_starts, len(q)] is the upper edge lo + j * (hi - lo) / n_bins of
    the first bin j whose cumulative count - the underflow column counted first - reaches k: the k-th smallest cost lies in
    that bin, so it is at most the result and more than the result minus one bin width.  cmin / cmax (per start, e.g. the
    campaign's min and max) clip the result.  NaN where the rank falls in the underflow and no cmin is given, or in the
    overflow and no cmax is given (with cmin / cmax those give cmin / cmax)."""
    h, nb, lo, hi = _hist_edges(hist, lo, hi)
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if np.any(~((qs >= 0) & (qs <= 1))):
        raise ValueError("q must lie in [0, 1]")
    ns = h.shape[0]
    M = h.sum(axis=1)
    cum = np.cumsum(h, axis=1)
    out = np.full((ns, qs.size), np.nan)
    for i, qq in enumerate(qs):
        k = np.maximum(1, np.ceil(qq * M)).astype(np.int64)
        col = np.argmax(cum >= k[:, None], axis=1)                              # the first column whose cumulative count reaches k
        inside = (col >= 1) & (col <= nb) & (M > 0)
        edge = lo + col * (hi - lo) / nb
        edge = np.where(col == nb, hi, edge)                                    # the last edge is hi itself, not its rounding
        val = np.where(inside, edge, np.nan)
        if cmin is not None:
            val = np.where((col == 0) & (M > 0), np.broadcast_to(np.asarray(cmin, dtype=np.float64).reshape(-1), (ns,)), val)
        if cmax is not None:
            val = np.where((col == nb + 1) & (M > 0), np.broadcast_to(np.asarray(cmax, dtype=np.float64).reshape(-1), (ns,)), val)
        if cmin is not None or cmax is not None:
            val = np.clip(val, None if cmin is None else np.asarray(cmin, dtype=np.float64).reshape(-1),
                          None if cmax is None else np.asarray(cmax, dtype=np.float64).reshape(-1))
        out[:, i] = val
    return out


def campaign_tail_mean(hist, lo, hi, q):
    """The mean of the samples at or above the q-quantile, estimated from campaign histograms (pure numpy): the samples of rank
    k = max(1, ceil(q * M)) and above, each taken at its bin's midpoint - an ESTIMATE within one bin width of the exact tail
    mean, not a bound, and exact in no digit.  hist, lo, hi, q as in campaign_quantiles; returns [n_starts, len(q)].  NaN where
    a sample of the tail lies in the underflow or the overflow column (it has no midpoint) or the row is empty."""
    h, nb, lo, hi = _hist_edges(hist, lo, hi)
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if np.any(~((qs >= 0) & (qs <= 1))):
        raise ValueError("q must lie in [0, 1]")
    ns = h.shape[0]
    M = h.sum(axis=1)
    cum = np.cumsum(h, axis=1)
    before = cum - h                                                            # samples of lower columns
    mid = lo[:, None] + (np.arange(nb)[None, :] + 0.5) * ((hi - lo) / nb)[:, None]
    out = np.full((ns, qs.size), np.nan)
    for i, qq in enumerate(qs):
        k = np.maximum(1, np.ceil(qq * M)).astype(np.int64)
        take = np.clip(cum - np.maximum(before, (k - 1)[:, None]), 0, None)     # of every column, the samples of rank >= k
        n_tail = M - (k - 1)
        ok = (M > 0) & (take[:, 0] == 0) & (take[:, nb + 1] == 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, i] = np.where(ok, (take[:, 1:nb + 1] * mid).sum(axis=1) / np.maximum(n_tail, 1), np.nan)
    return out


def campaign_reduce(cost, n_samples, X_final=None, left=None, cost_threshold=None, settle_tol=None):
    """Rollout.run_campaign's reduction on the CPU (hjb_rollout_campaign_reduce; no device), over per-trajectory results such as
    run_noisy returns for starts repeated n_samples times: cost [n_starts * n_samples] (trajectory s * n_samples + m is sample m
    of start s), X_final [D, n_starts * n_samples] (needed with settle_tol), left [n_starts * n_samples] (non-zero: the
    trajectory left the grid; None counts none).  Returns stats [n_starts, 8] (sum, sum of squares, min, max, n_exceed, n_left,
    n_settled, sum over settled: the bits run_campaign returns for the same samples), mean, var = (sumsq - sum^2 / M) / (M - 1)
    clipped at 0 (0 for M = 1), std, min, max, n_exceed / n_left / n_settled (int64) and mean_settled (NaN where none settled)."""
    lib = load_library()
    c = np.ascontiguousarray(np.asarray(cost, dtype=np.float64).reshape(-1))
    M = int(n_samples)
    if M < 1 or c.size % M:
        raise ValueError("cost: %d values are not a whole number of %d samples" % (c.size, M))
    ns = c.size // M
    D, Xf = 1, None
    if X_final is not None:
        Xf2 = np.asarray(X_final, dtype=np.float64)
        Xf2 = Xf2.reshape(1, -1) if Xf2.ndim == 1 else Xf2
        if Xf2.shape[1] != c.size:
            raise ValueError("X_final: %d columns for %d costs" % (Xf2.shape[1], c.size))
        D, Xf = Xf2.shape[0], np.ascontiguousarray(Xf2.T)
    lf = None
    if left is not None:
        lf = np.ascontiguousarray((np.asarray(left).reshape(-1) != 0).astype(np.uint8))
        if lf.size != c.size:
            raise ValueError("left: %d flags for %d costs" % (lf.size, c.size))
    if settle_tol is not None and Xf is None:
        raise ValueError("settle_tol needs X_final")
    thr, tol = _campaign_bounds(ns, D, cost_threshold, settle_tol)
    stats = np.empty((ns, _abi.HJB_CAMPAIGN_NSTAT))
    _check(lib, None, lib.hjb_rollout_campaign_reduce(ns, M, D, _f64p(c), _f64p(Xf), None if lf is None else lf.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                      _f64p(thr), _f64p(tol), _f64p(stats)))
    return _campaign_dict(stats, M)


_PAIR_KIND = {"labels": _abi.HJB_PAIR_LABELS, "lookahead": _abi.HJB_PAIR_LOOKAHEAD, "greedy": _abi.HJB_PAIR_GREEDY}


def _pair_side(side, name):
    """("labels", planes, method) / ("lookahead", value_planes) / ("greedy", value_planes) -> kind, method and the planes"""
    if not isinstance(side, (tuple, list)) or len(side) < 2 or side[0] not in _PAIR_KIND:
        raise ValueError('%s must be ("labels", planes, method), ("lookahead", value_planes) or ("greedy", value_planes)' % name)
    if side[0] == "labels":
        method = side[2] if len(side) > 2 else "linear"
        if method not in _LOOKUP:
            raise ValueError("%s: method must be one of %s" % (name, sorted(_LOOKUP)))
        return _PAIR_KIND["labels"], _LOOKUP[method], _int32_vector(side[1], "plane_of_step")
    if len(side) != 2:
        raise ValueError("%s: a %s controller is (%r, value_planes)" % (name, side[0], side[0]))
    return _PAIR_KIND[side[0]], 0, _int32_vector(side[1], "value_plane_of_step")


def _campaign_pair_dict(stats_d, M):
    """stats_d [n_starts, 8] as the library wrote it -> the difference entries run_campaign_pair and campaign_pair_reduce return"""
    total, sumsq = stats_d[:, 0], stats_d[:, 1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        var = np.maximum((sumsq - total * total / M) / (M - 1), 0.0) if M > 1 else np.zeros(stats_d.shape[0])
        mean = total / M
        se = np.sqrt(var / M)
        t = mean / se
        n_both = stats_d[:, 6].astype(np.int64)
        mean_both = np.where(n_both > 0, stats_d[:, 7] / np.maximum(n_both, 1), np.nan)
    n_b, n_a = stats_d[:, 4].astype(np.int64), stats_d[:, 5].astype(np.int64)
    return {"stats_d": stats_d, "mean_diff": mean, "var_diff": var, "std_diff": np.sqrt(var), "se_diff": se, "t": t,
            "min_diff": stats_d[:, 2], "max_diff": stats_d[:, 3], "n_b_lower": n_b, "n_a_lower": n_a, "n_tie": M - n_b - n_a,
            "n_both_in": n_both, "mean_diff_both_in": mean_both}


def campaign_pair_reduce(cost_a, cost_b, n_samples, left_a=None, left_b=None):
    """Rollout.run_campaign_pair's difference record on the CPU (hjb_rollout_campaign_pair_reduce; no device), over per-trajectory
    costs of two controllers flown on the same streams, such as run_noisy and run_lookahead(noisy=True) return for starts repeated
    n_samples times: cost_a, cost_b [n_starts * n_samples] (trajectory s * n_samples + m is sample m of start s), left_a, left_b
    [n_starts * n_samples] (non-zero: that flight left the grid; None: none left).  d = cost_b - cost_a per sample, one rounded
    subtraction; a negative d means b paid less.  Returns stats_d [n_starts, 8] (sum d, sum d * d, min d, max d, n(b lower),
    n(a lower), n(both stayed in the grid), sum d over those: the bits run_campaign_pair returns for the same samples),
    mean_diff, var_diff = (sumsq - sum^2 / M) / (M - 1) clipped at 0 (0 for M = 1), std_diff, se_diff = sqrt(var_diff / M),
    t = mean_diff / se_diff under numpy's rules (inf or NaN where se_diff is 0), min_diff, max_diff, n_b_lower, n_a_lower,
    n_tie = M - n_b_lower - n_a_lower - a NaN difference is neither lower and is counted here, as a tie -, n_both_in and
    mean_diff_both_in (NaN where no sample of the start kept both flights in the grid); a and b, campaign_reduce's dicts of the two
    cost arrays, and device_ms = 0.0."""
    lib = load_library()
    ca = np.ascontiguousarray(np.asarray(cost_a, dtype=np.float64).reshape(-1))
    cb = np.ascontiguousarray(np.asarray(cost_b, dtype=np.float64).reshape(-1))
    M = int(n_samples)
    if ca.size != cb.size:
        raise ValueError("cost_a and cost_b: %d and %d values" % (ca.size, cb.size))
    if M < 1 or ca.size % M:
        raise ValueError("cost: %d values are not a whole number of %d samples" % (ca.size, M))
    ns = ca.size // M
    flags = []
    for name, left in (("left_a", left_a), ("left_b", left_b)):
        lf = None
        if left is not None:
            lf = np.ascontiguousarray((np.asarray(left).reshape(-1) != 0).astype(np.uint8))
            if lf.size != ca.size:
                raise ValueError("%s: %d flags for %d costs" % (name, lf.size, ca.size))
        flags.append(lf)
    u8p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))
    stats_d = np.empty((ns, _abi.HJB_CAMPAIGN_PAIR_NSTAT))
    _check(lib, None, lib.hjb_rollout_campaign_pair_reduce(ns, M, _f64p(ca), _f64p(cb), u8p(flags[0]), u8p(flags[1]), _f64p(stats_d)))
    # a and b: the plain records of the two cost arrays (campaign_reduce, no threshold and no tolerance); no device ran
    return {"a": campaign_reduce(ca, M, left=flags[0]), "b": campaign_reduce(cb, M, left=flags[1]), **_campaign_pair_dict(stats_d, M),
            "device_ms": 0.0}


def greedy_host(knots, u_table, A, B, J, X0, value_plane_of_step, c=None, q=None, r=None, index_base=0, keep_path=False):
    """Rollout.run_greedy on the CPU (hjb_rollout_greedy_host; no device, no object): the functions the kernel calls, in a
    plain loop over the trajectories.  knots, u_table: as Rollout takes them; A, B, c, q, r: as set_model; J: as set_values, or
    None when every plane index is -1.  Returns run_greedy's dict without device_ms; L_path holds label + index_base."""
    lib = load_library()
    ks = [np.ascontiguousarray(k, dtype=np.float64).reshape(-1) for k in knots]
    D = len(ks)
    n = [len(k) for k in ks]
    nS = int(np.prod(n, dtype=np.int64)) if ks else 1
    ut = np.asarray(u_table, dtype=np.float64)
    ut = ut.reshape(-1, 1) if ut.ndim == 1 else ut
    n_labels, nu = ut.shape
    ut = np.ascontiguousarray(ut.reshape(-1, order="F"))
    kcat = np.ascontiguousarray(np.concatenate(ks) if ks else np.zeros(0))
    v, dtype = (None, _abi.HJB_F64) if J is None else _value_planes(J, nS)
    X = _starts(X0, D)
    nt = X.shape[0]
    ps = _int32_vector(value_plane_of_step, "value_plane_of_step")
    K = int(ps.size)
    Xf = np.empty((nt, D))
    cost = np.empty(nt)
    flat, paths = _path_buffers(nt, keep_path, ("X_path", D, K + 1), ("U_path", nu, K), ("L_path", 1, K), ("V_path", 1, K))
    _check(lib, None, lib.hjb_rollout_greedy_host(D, (C.c_int32 * max(D, 1))(*n), _f64p(kcat), int(n_labels), int(nu), _f64p(ut),
                                                  _f64p(_f64_colmajor(A, D, D)), _f64p(_f64_colmajor(B, D, nu)), _f64p(_f64_vec(c, D)),
                                                  _f64p(_f64_vec(q, D)), _f64p(_f64_vec(r, nu)), dtype, 0 if v is None else v.size // nS,
                                                  None if v is None else v.ctypes.data, K, _i32p(ps), nt, _f64p(X), _f64p(Xf), _f64p(cost),
                                                  *map(_f64p, flat)))
    if keep_path:
        paths["L_path"] = paths["L_path"][:, 0, :].astype(np.int32) + np.int32(index_base)
        paths["V_path"] = paths["V_path"][:, 0, :]
    return {"X_final": Xf.T, "cost": cost, **paths}


def lookahead_host(knots, u_table, A, B, J, X0, value_plane_of_step, offsets, weights=None, mode="expect", c=None, q=None, r=None,
                   index_base=0, nodes=None, flight_offsets=None, keep_path=False):
    """Rollout.run_lookahead on the CPU (hjb_rollout_lookahead_host; no device, no object): greedy_host's arguments, the
    lookahead set as set_lookahead takes it, and optionally the plant's noise as GIVEN nodes - nodes [n_traj, n_steps] int32
    (noise_draw's output) into flight_offsets [D, W_f] (set_noise's offsets); None flies the nominal plant.  Returns
    run_greedy's dict without device_ms; L_path holds label + index_base."""
    lib = load_library()
    ks = [np.ascontiguousarray(k, dtype=np.float64).reshape(-1) for k in knots]
    D = len(ks)
    n = [len(k) for k in ks]
    nS = int(np.prod(n, dtype=np.int64)) if ks else 1
    ut = np.asarray(u_table, dtype=np.float64)
    ut = ut.reshape(-1, 1) if ut.ndim == 1 else ut
    n_labels, nu = ut.shape
    ut = np.ascontiguousarray(ut.reshape(-1, order="F"))
    kcat = np.ascontiguousarray(np.concatenate(ks) if ks else np.zeros(0))
    v, dtype = (None, _abi.HJB_F64) if J is None else _value_planes(J, nS)
    X = _starts(X0, D)
    nt = X.shape[0]
    ps = _int32_vector(value_plane_of_step, "value_plane_of_step")
    K = int(ps.size)
    off, w, mode = check_disturbance(D, offsets, weights, mode)
    offc = np.ascontiguousarray(off.reshape(-1, order="F"))
    nd = fo = None
    Wf = 0
    if nodes is not None:
        if flight_offsets is None:
            raise ValueError("nodes need flight_offsets [D, W_f]")
        fo2 = np.array(flight_offsets, dtype=np.float64, ndmin=2).reshape(D, -1)
        Wf = fo2.shape[1]
        fo = np.ascontiguousarray(fo2.reshape(-1, order="F"))
        nd = np.asarray(nodes)
        if nd.shape != (nt, K) or nd.dtype.kind not in "iu":
            raise ValueError("nodes must be [n_traj=%d, n_steps=%d] integers, got %r %s" % (nt, K, nd.shape, nd.dtype))
        nd = np.ascontiguousarray(nd.astype(np.int32).reshape(-1, order="F"))
    Xf = np.empty((nt, D))
    cost = np.empty(nt)
    flat, paths = _path_buffers(nt, keep_path, ("X_path", D, K + 1), ("U_path", nu, K), ("L_path", 1, K), ("V_path", 1, K))
    _check(lib, None, lib.hjb_rollout_lookahead_host(D, (C.c_int32 * max(D, 1))(*n), _f64p(kcat), int(n_labels), int(nu), _f64p(ut),
                                                     _f64p(_f64_colmajor(A, D, D)), _f64p(_f64_colmajor(B, D, nu)), _f64p(_f64_vec(c, D)),
                                                     _f64p(_f64_vec(q, D)), _f64p(_f64_vec(r, nu)), dtype, 0 if v is None else v.size // nS,
                                                     None if v is None else v.ctypes.data, K, _i32p(ps), nt, _f64p(X), _f64p(Xf), _f64p(cost),
                                                     *map(_f64p, flat), _DIST_MODE[mode], off.shape[1], _f64p(offc), _f64p(w), _i32p(nd),
                                                     int(Wf), _f64p(fo)))
    if keep_path:
        paths["L_path"] = paths["L_path"][:, 0, :].astype(np.int32) + np.int32(index_base)
        paths["V_path"] = paths["V_path"][:, 0, :]
    return {"X_final": Xf.T, "cost": cost, **paths}


def control_lookahead_host(knots, u_table, A, B, J, X0, value_plane_of_step, offsets, weights=None, mode="expect", c=None, q=None, r=None,
                           index_base=0, nodes=None, eps=None, base=None, keep_path=False):
    """ControlLookaheadRollout.run_control_lookahead on the CPU (hjb_rollout_control_lookahead_host; no device, no object):
    lookahead_host's arguments with the per-control set as set_control_lookahead takes it (offsets [D, W, n_labels]), and
    optionally the actuator plant as GIVEN nodes - nodes [n_traj, n_steps] int32 (noise_draw's output) of the set eps [W_f] or
    [W_f, n_u] and base [D, W_f] or None (set_actuator_noise's arguments); nodes None flies the nominal plant.  Returns
    run_greedy's dict without device_ms; L_path holds label + index_base, U_path the commanded controls."""
    lib = load_library()
    ks = [np.ascontiguousarray(k, dtype=np.float64).reshape(-1) for k in knots]
    D = len(ks)
    n = [len(k) for k in ks]
    nS = int(np.prod(n, dtype=np.int64)) if ks else 1
    ut = np.asarray(u_table, dtype=np.float64)
    ut = ut.reshape(-1, 1) if ut.ndim == 1 else ut
    n_labels, nu = ut.shape
    ut = np.ascontiguousarray(ut.reshape(-1, order="F"))
    kcat = np.ascontiguousarray(np.concatenate(ks) if ks else np.zeros(0))
    v, dtype = (None, _abi.HJB_F64) if J is None else _value_planes(J, nS)
    X = _starts(X0, D)
    nt = X.shape[0]
    ps = _int32_vector(value_plane_of_step, "value_plane_of_step")
    K = int(ps.size)
    off, w, mode = check_control_disturbance(D, (n_labels,), offsets, weights, mode)
    offc = np.ascontiguousarray(off.reshape(-1, order="F"))
    nd = ec = bc = None
    Wf = 0
    if nodes is not None:
        if eps is None:
            raise ValueError("nodes need eps [W_f] or [W_f, n_u]")
        e = np.array(eps, dtype=np.float64)
        if e.ndim == 1:
            e = np.repeat(e[:, None], nu, axis=1)
        if e.ndim != 2 or e.shape[1] != nu:
            raise ValueError("eps must be [W_f] or [W_f, n_u=%d], got %r" % (nu, e.shape))
        Wf = e.shape[0]
        ec = np.ascontiguousarray(e.reshape(-1))              # [W_f, n_u] row-major is [n_u, W_f] column-major
        if base is not None:
            b = np.array(base, dtype=np.float64, ndmin=2)
            if b.shape != (D, Wf):
                raise ValueError("base must be [D=%d, W_f=%d], got %r" % (D, Wf, b.shape))
            bc = np.ascontiguousarray(b.reshape(-1, order="F"))
        nd = np.asarray(nodes)
        if nd.shape != (nt, K) or nd.dtype.kind not in "iu":
            raise ValueError("nodes must be [n_traj=%d, n_steps=%d] integers, got %r %s" % (nt, K, nd.shape, nd.dtype))
        nd = np.ascontiguousarray(nd.astype(np.int32).reshape(-1, order="F"))
    Xf = np.empty((nt, D))
    cost = np.empty(nt)
    flat, paths = _path_buffers(nt, keep_path, ("X_path", D, K + 1), ("U_path", nu, K), ("L_path", 1, K), ("V_path", 1, K))
    _check(lib, None, lib.hjb_rollout_control_lookahead_host(
        D, (C.c_int32 * max(D, 1))(*n), _f64p(kcat), int(n_labels), int(nu), _f64p(ut), _f64p(_f64_colmajor(A, D, D)),
        _f64p(_f64_colmajor(B, D, nu)), _f64p(_f64_vec(c, D)), _f64p(_f64_vec(q, D)), _f64p(_f64_vec(r, nu)), dtype,
        0 if v is None else v.size // nS, None if v is None else v.ctypes.data, K, _i32p(ps), nt, _f64p(X), _f64p(Xf), _f64p(cost),
        *map(_f64p, flat), _DIST_MODE[mode], off.shape[1], off.shape[2], _f64p(offc), _f64p(w), _i32p(nd), int(Wf), _f64p(ec), _f64p(bc)))
    if keep_path:
        paths["L_path"] = paths["L_path"][:, 0, :].astype(np.int32) + np.int32(index_base)
        paths["V_path"] = paths["V_path"][:, 0, :]
    return {"X_final": Xf.T, "cost": cost, **paths}


def lookahead_campaign_host(knots, u_table, A, B, J, X0, value_plane_of_step, n_samples, offsets, flight_offsets, weights=None,
                            mode="expect", flight_weights=None, c=None, q=None, r=None, seed=0, first_stream=0, cost_threshold=None,
                            settle_tol=None):
    """Rollout.run_lookahead_campaign on the CPU (hjb_rollout_lookahead_campaign_host; no device, no object): lookahead_host's
    problem and lookahead set (offsets, weights, mode), the plant's node set as set_noise takes it (flight_offsets [D, W_f],
    flight_weights or None), and run_lookahead_campaign's arguments.  One start's samples at a time: the nodes drawn as
    noise_draw draws them, the flight as lookahead_host flies it, the statistics as campaign_reduce forms them.  Returns
    campaign_reduce's dict."""
    lib = load_library()
    ks = [np.ascontiguousarray(k, dtype=np.float64).reshape(-1) for k in knots]
    D = len(ks)
    n = [len(k) for k in ks]
    nS = int(np.prod(n, dtype=np.int64)) if ks else 1
    ut = np.asarray(u_table, dtype=np.float64)
    ut = ut.reshape(-1, 1) if ut.ndim == 1 else ut
    n_labels, nu = ut.shape
    ut = np.ascontiguousarray(ut.reshape(-1, order="F"))
    kcat = np.ascontiguousarray(np.concatenate(ks) if ks else np.zeros(0))
    v, dtype = (None, _abi.HJB_F64) if J is None else _value_planes(J, nS)
    X = _starts(X0, D)
    ns = X.shape[0]
    ps = _int32_vector(value_plane_of_step, "value_plane_of_step")
    off, w, mode = check_disturbance(D, offsets, weights, mode)
    offc = np.ascontiguousarray(off.reshape(-1, order="F"))
    fo2 = np.array(flight_offsets, dtype=np.float64, ndmin=2).reshape(D, -1)
    fo = np.ascontiguousarray(fo2.reshape(-1, order="F"))
    fw = None if flight_weights is None else _f64_vec(flight_weights, fo2.shape[1])
    thr, tol = _campaign_bounds(ns, D, cost_threshold, settle_tol)
    stats = np.empty((ns, _abi.HJB_CAMPAIGN_NSTAT))
    _check(lib, None, lib.hjb_rollout_lookahead_campaign_host(
        D, (C.c_int32 * max(D, 1))(*n), _f64p(kcat), int(n_labels), int(nu), _f64p(ut), _f64p(_f64_colmajor(A, D, D)),
        _f64p(_f64_colmajor(B, D, nu)), _f64p(_f64_vec(c, D)), _f64p(_f64_vec(q, D)), _f64p(_f64_vec(r, nu)), dtype,
        0 if v is None else v.size // nS, None if v is None else v.ctypes.data, int(ps.size), _i32p(ps), _DIST_MODE[mode], off.shape[1],
        _f64p(offc), _f64p(w), int(fo2.shape[1]), _f64p(fo), _f64p(fw), ns, int(n_samples), _f64p(X), int(seed) & (2 ** 64 - 1),
        int(first_stream), _f64p(thr), _f64p(tol), _f64p(stats)))
    return _campaign_dict(stats, int(n_samples))


def attitude_linear_response(inertia, h, K, C_gain, X0, n_steps, qc=None, u_limit=None, integrator="RK4", cost_form="quat",
                             weights=None, keep_path=False, chunk=0, device=0):
    """hjb_attitude_linear_response: the closed loop of the linear attitude controller U = -K qe(1:3) - C w
    (attitude-control/Solver_attitude.m:508-591) from many initial attitudes at once on the GPU (K21).  No policy, so no object.
    inertia = (J1, J2, J3), step h, K and C_gain [3, 3], qc [4, 4] (None: identity), u_limit [3] >= 0 (None: no limit), integrator
    'taylor' or 'RK4', X0 [7, n_traj] (X = [w1 w2 w3 q1 q2 q3 q4], q4 scalar).  cost_form 'quat': weights = q [7] then r [3], the
    stage cost of Rollout.run_attitude; 'angle': weights = qw [3], qt [3], r [3] (a tenth entry is ignored), that of
    Rollout.run_attitude_simplified; None: zeros.  Returns what Rollout.run_attitude returns: X_final [7, n_traj], cost [n_traj],
    X_path [n_traj, 7, n_steps+1], U_path [n_traj, 3, n_steps], A_path [n_traj, 3, n_steps] (yaw, pitch, roll in radians; the
    paths None unless keep_path) and device_ms."""
    lib = load_library()
    form = {"quat": _abi.HJB_ATTL_COST_QUAT, "angle": _abi.HJB_ATTL_COST_ANGLE}[cost_form]
    wt = None
    if weights is not None:
        wt = np.zeros(10)
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.size not in ((10,) if form == _abi.HJB_ATTL_COST_QUAT else (9, 10)):
            raise ValueError("weights: %d entries (cost_form 'quat' takes 10, 'angle' 9 or 10)" % w.size)
        wt[:w.size] = w
    X = _starts(X0, 7)
    nt = X.shape[0]
    Kn = int(n_steps)
    Xf = np.empty((nt, 7))
    cost = np.empty(nt)
    flat, paths = _path_buffers(nt, keep_path and Kn >= 0, ("X_path", 7, Kn + 1), ("U_path", 3, Kn), ("A_path", 3, Kn))
    ms = C.c_double(0.0)
    st = lib.hjb_attitude_linear_response(int(device), _f64p(_f64_vec(inertia, 3)), float(h), _ATT_INTEGRATOR[integrator],
                                          _f64p(_f64_colmajor(K, 3, 3)), _f64p(_f64_colmajor(C_gain, 3, 3)), _f64p(_f64_colmajor(qc, 4, 4)),
                                          _f64p(_f64_vec(u_limit, 3)), form, _f64p(wt), Kn, nt, _f64p(X), _f64p(Xf), _f64p(cost),
                                          *map(_f64p, flat), int(chunk), C.byref(ms))
    if st != _abi.HJB_OK:
        msg = lib.hjb_rollout_last_error(None)
        raise HjbError(st, (msg or b"").decode() or lib.hjb_status_string(st).decode())
    return {"X_final": Xf.T, "cost": cost, **paths, "device_ms": ms.value}


class DeviceBuffer:
    """A device allocation owned through the library (hjb_device_malloc): what a host without a HIP binding of its
    own hands to Backup.backup_stage_device.  `ptr` is an ordinary HIP device pointer."""

    def __init__(self, nbytes, device=0):
        self.lib = load_library()
        self.device, self.nbytes = int(device), int(nbytes)
        p = C.c_void_p()
        _check(self.lib, None, self.lib.hjb_device_malloc(self.device, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def __int__(self):
        return self.ptr

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        _check(self.lib, None, self.lib.hjb_device_copy(self.device, self.ptr, a.ctypes.data, a.nbytes, _abi.HJB_COPY_H2D))

    def download(self, dtype, count=None):
        dt = np.dtype(dtype)
        out = np.empty(self.nbytes // dt.itemsize if count is None else int(count), dtype=dt)
        _check(self.lib, None, self.lib.hjb_device_copy(self.device, out.ctypes.data, self.ptr, out.nbytes, _abi.HJB_COPY_D2H))
        return out

    def gather(self, dtype, sel):
        """out[i] = buffer[sel[i]] (elements of `dtype`): sample a device-resident array."""
        dt = np.dtype(dtype)
        s = np.ascontiguousarray(sel, dtype=np.int64)
        out = np.empty(s.size, dtype=dt)
        _check(self.lib, None, self.lib.hjb_device_gather(self.device, self.ptr, dt.itemsize,
                                                          s.ctypes.data_as(C.POINTER(C.c_int64)), s.size, out.ctypes.data))
        return out

    def free(self):
        if getattr(self, "ptr", None):
            self.lib.hjb_device_free(self.device, self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_mem_info(device=0):
    lib = load_library()
    f, t = C.c_int64(), C.c_int64()
    _check(lib, None, lib.hjb_device_mem_info(int(device), C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)


def _fill_separable(obj, fn, vecs, dJ, stream):
    """The body of Backup.fill_separable and RankSlab.fill_separable: the vectors in the spec's arithmetic type, their addresses,
    one library call.  (dJ is required: None is refused as int() refuses it.)"""
    vs = [np.ascontiguousarray(v, dtype=obj.spec.dtype) for v in vecs]
    ptrs = (C.c_void_p * len(vs))(*[v.ctypes.data for v in vs])
    obj._check(fn(getattr(obj, obj._handle), ptrs, int(_ptr(dJ)), _stream(stream)))


def _probe_block(spec, probe, n_planes):
    """probe = {"lo", "hi", "control", "want"} -> (the zeroed arrays the taps are written to, by name, and the hjb_probe that
    points at them); n_planes: the trailing stage axis of a sweep, 0 for one stage."""
    D = spec.D
    pb = _abi.hjb_probe()
    ext = []
    for a in range(D):
        pb.lo[a], pb.hi[a] = int(probe["lo"][a]), int(probe["hi"][a])
        ext.append(pb.hi[a] - pb.lo[a])
    for c in range(spec.C):
        pb.control[c] = int(probe["control"][c])
    want = probe.get("want", ("g", "x_next", "j_interp"))
    tail = (n_planes,) if n_planes else ()
    out = {}
    for name, mid in (("g", ()), ("x_next", (D,)), ("j_interp", ())):
        if name in want:
            out[name] = np.zeros(tuple(ext) + mid + tail, dtype=spec.dtype, order="F")
            setattr(pb, name, out[name].ctypes.data)
    return out, pb


def _sweep_args(spec, n_stages, terminal=None, keep_J=False, keep_idx=False, monitor_period=0, monitor_tol=0.0, progress=None,
                progress_every_stage=False, probe=None, monitor_single=False):
    """What a sweep call (hjb_solve, hjb_solve_multi, a member of hjb_solve_batch) is handed: -> (the filled hjb_solve_opts, out,
    keep).  out: the arrays the library writes - J and idx [nS], J_stages and idx_stages [nS, n_stages] in Fortran order,
    zeroed, or None, probe the taps' arrays or None.  keep: everything the struct points to - out, the terminal vector, the
    ctypes callback, the probe block; the caller holds it until the library call has returned."""
    nS, dt, it = spec.nS, spec.j_dtype, spec.idx_np_dtype
    o = _abi.hjb_solve_opts()
    o.n_stages, o.monitor_period, o.monitor_tol = int(n_stages), int(monitor_period), float(monitor_tol)
    o.progress_every_stage, o.monitor_single = 1 if progress_every_stage else 0, 1 if monitor_single else 0
    out = {}
    keep = [out]
    if terminal is not None:
        t = _j_vector(terminal, dt, nS, "terminal")
        keep.append(t)
        o.terminal = t.ctypes.data
    out["J"], out["idx"] = np.empty(nS, dtype=dt), np.empty(nS, dtype=it)
    out["J_stages"] = np.zeros((nS, n_stages), dtype=dt, order="F") if keep_J else None
    out["idx_stages"] = np.zeros((nS, n_stages), dtype=it, order="F") if keep_idx else None
    o.J_final, o.idx_final = out["J"].ctypes.data, out["idx"].ctypes.data
    o.J_stages = None if out["J_stages"] is None else out["J_stages"].ctypes.data
    o.idx_stages = None if out["idx_stages"] is None else out["idx_stages"].ctypes.data
    if progress is not None:
        cb = _abi.hjb_progress_fn(lambda user, k_s, e, e2, sec: progress(k_s, e, e2, sec))
        keep.append(cb)
        o.progress = cb
    out["probe"] = None
    if probe is not None:
        out["probe"], pb = _probe_block(spec, probe, n_stages)
        keep.append(pb)
        o.probe = C.pointer(pb)
    return o, out, keep


def _sweep_result(out, res):
    """The dict of a sweep: the arrays of _sweep_args and the hjb_result the library filled."""
    return {"J": out["J"], "idx": out["idx"], "J_stages": out["J_stages"], "idx_stages": out["idx_stages"],
            "stages_done": res.stages_done, "stopped_early": bool(res.stopped_early), "sweep_ms": res.sweep_ms, "last_e": res.last_e,
            "last_e2": res.last_e2, "probe": out["probe"]}


class Backup(_Handle):
    """A problem resident on one GPU.  Mirrors the C handle one to one."""
    _handle, _destroy, _last_error = "_h", "hjb_destroy", "hjb_last_error"

    def __init__(self, spec: ProblemSpec, device=0, slab=None, variant=None):
        self.lib = load_library()
        self.spec = spec
        self._cprob, self._keep = spec.to_c(slab)
        self._h = C.c_void_p()
        self._created(self.lib.hjb_create(C.byref(self._cprob), int(device), C.byref(self._h)))
        self.device = int(device)
        if variant is not None:
            self.set_option("variant", variant)
        if spec.disturbance is not None:
            try:
                self.set_disturbance(*spec.disturbance)
            except Exception:
                self.close()
                raise
        if spec.control_disturbance is not None:
            try:
                self.set_control_disturbance(*spec.control_disturbance)
            except Exception:
                self.close()
                raise

    # -- queries ----------------------------------------------------------
    def info(self):
        """hjb_get_info's fields, plus the disturbance in effect: dist_nodes (0: none), dist_mode ("expect" / "worst" / None), dist_axes,
        dist_ctrl (True: the per-control one, set_control_disturbance)."""
        inf = _abi.hjb_info()
        self._check(self.lib.hjb_get_info(self._h, C.byref(inf)))
        out = {k: getattr(inf, k) for k, _ in inf._fields_}
        out["dist_nodes"] = self.get_option("dist_nodes")
        out["dist_mode"] = ("expect", "worst")[self.get_option("dist_mode")] if out["dist_nodes"] else None
        out["dist_axes"] = self.get_option("dist_axes")
        out["dist_ctrl"] = bool(self.get_option("dist_ctrl"))
        return out

    # -- the disturbance the handle's stages carry (hjb_set_disturbance: kernel variant 8) ----------------------------
    def set_disturbance(self, offsets, weights=None, mode="expect"):
        """Every stage this handle launches from now on - backup_stage, solve, evaluate* - takes the expected value
        (mode "expect", weights [W] or None = equal) or the worst case ("worst") of J_next over the W next states
        x_next + offsets[:, w].  offsets [D, W], row a for state axis a of THIS handle's spec."""
        off, w, mode = check_disturbance(self.spec.D, offsets, weights, mode)
        offc = np.asfortranarray(off)
        self._check(self.lib.hjb_set_disturbance(self._h, _abi.HJB_DIST_WORST if mode == "worst" else _abi.HJB_DIST_EXPECT, off.shape[1],
                                                 _f64p(offc), _f64p(w)))

    def set_control_disturbance(self, offsets, weights=None, mode="expect"):
        """set_disturbance with a node set per candidate control (hjb_set_control_disturbance): the W next states of the
        control with 0-based column-major label l are x_next + offsets[:, w, l].  offsets [D, W, nU], or [D, W, *m] (flattened
        column-major); weights and mode as set_disturbance.  The two settings replace each other; hjbdp.actuator_nodes builds
        the table of an actuator that delivers u * (1 + eps_w)."""
        off, w, mode = check_control_disturbance(self.spec.D, self.spec.m, offsets, weights, mode)
        offc = np.asfortranarray(off)
        self._check(self.lib.hjb_set_control_disturbance(self._h, _abi.HJB_DIST_WORST if mode == "worst" else _abi.HJB_DIST_EXPECT,
                                                         off.shape[1], off.shape[2], _f64p(offc), _f64p(w)))

    def clear_disturbance(self):
        """Back to the nominal backup, from either setting: the launch the handle had, the same bits as before."""
        self._check(self.lib.hjb_set_disturbance(self._h, _abi.HJB_DIST_EXPECT, 0, None, None))

    def set_option(self, key, value):
        self._check(self.lib.hjb_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int64()
        self._check(self.lib.hjb_get_option(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    # -- one stage, host buffers -------------------------------------------
    def backup_stage(self, J_next):
        """[J_k, idx] = min(g + F(x_next), [], ctrl): J_next/J_k in the (haloed)
        column-major J layout, idx int32 labels of the owned states."""
        inf = self.info()
        Jn = _j_vector(J_next, self.spec.j_dtype, inf["j_elems"], "J_next")
        Jo = np.empty_like(Jn)
        idx = np.empty(inf["n_states"], dtype=self.spec.idx_np_dtype)
        self._check(self.lib.hjb_backup_stage(self._h, Jn.ctypes.data, Jo.ctypes.data, idx.ctypes.data))
        return Jo, idx

    # -- one stage, device buffers (torch tensors or raw pointers) -----------
    def backup_stage_device(self, dJ_next, dJ_out, d_idx=None, stream=0):
        self._check(self.lib.hjb_backup_stage_device(self._h, _ptr(dJ_next), _ptr(dJ_out), _ptr(d_idx), _stream(stream)))

    def fill_separable(self, vecs, dJ, stream=0):
        """dJ[s] = ((vecs[0][i0] + vecs[1][i1]) + ...) over the whole grid (hjb_device_fill_separable)."""
        _fill_separable(self, self.lib.hjb_device_fill_separable, vecs, dJ, stream)

    def check_device_status(self, stream=0):
        self._check(self.lib.hjb_check_device_status(self._h, _stream(stream)))

    # -- the whole sweep -----------------------------------------------------
    def solve(self, n_stages, terminal=None, keep_J=False, keep_idx=False, monitor_period=0, monitor_tol=0.0,
              progress=None, progress_every_stage=False, probe=None, monitor_single=False):
        """Backward sweep of n_stages backups.  Returns a dict with J (final), idx
        (final), optional J_stages/idx_stages [nS, n_stages] with reference stage
        k_s at column k_s-1, stages_done, stopped_early, sweep_ms.
        probe = {"lo": [..D], "hi": [..D], "control": [..C], "want": ("g", "x_next", "j_interp")} (0-based,
        half-open) asks for the reference's debug taps (Dynamic_Solver.m:212-219) of every stage: out["probe"]
        holds g [block..., n_stages], x_next [block..., D, n_stages], j_interp [block..., n_stages]."""
        o, out, keep = _sweep_args(self.spec, n_stages, terminal=terminal, keep_J=keep_J, keep_idx=keep_idx, monitor_period=monitor_period,
                                   monitor_tol=monitor_tol, progress=progress, progress_every_stage=progress_every_stage, probe=probe,
                                   monitor_single=monitor_single)                # keep: alive until hjb_solve has returned
        res = _abi.hjb_result()
        self._check(self.lib.hjb_solve(self._h, C.byref(o), C.byref(res)))
        return _sweep_result(out, res)

    # -- the cost of a GIVEN policy -------------------------------------------
    def _labels(self, labels, shapes):
        """labels as a flat column-major array after the checks evaluate* share: dtype spec.idx_np_dtype, one of `shapes`."""
        lab = np.asarray(labels)
        if lab.dtype != np.dtype(self.spec.idx_np_dtype):
            raise ValueError("labels must be %s (spec.idx_np_dtype), got %s" % (np.dtype(self.spec.idx_np_dtype), lab.dtype))
        if lab.shape not in shapes:
            raise ValueError("labels of shape %r: expected %s" % (lab.shape, " or ".join(repr(s) for s in shapes)))
        return np.ascontiguousarray(lab.reshape(-1, order="F"))

    def evaluate_stage(self, J_next, labels):
        """J_k = g(x, u(x)) + F(x_next(x, u(x))) for the given labels (hjb_evaluate_stage): no min.  J_next / J_k in the (haloed)
        column-major J layout; labels [n_states] of spec.idx_np_dtype as backup_stage returns them.  On backup_stage's own
        labels the result is backup_stage's J, bit for bit."""
        inf = self.info()
        lab = self._labels(labels, [(int(inf["n_states"]),)])
        Jn = _j_vector(J_next, self.spec.j_dtype, inf["j_elems"], "J_next")
        Jo = np.empty_like(Jn)
        self._check(self.lib.hjb_evaluate_stage(self._h, Jn.ctypes.data, lab.ctypes.data, Jo.ctypes.data))
        return Jo

    def evaluate_stage_device(self, dJ_next, d_labels, dJ_out, stream=0):
        """hjb_evaluate_stage_device: the same on device buffers (torch tensors, DeviceBuffers or raw pointers), asynchronous.
        A label out of range stores NaN for its state and makes the next check_device_status raise (HJB_E_INVALID)."""
        self._check(self.lib.hjb_evaluate_stage_device(self._h, _ptr(dJ_next), _ptr(d_labels), _ptr(dJ_out), _stream(stream)))

    def evaluate(self, n_stages, labels, terminal=None, keep_J=False):
        """The sweep of a fixed policy (hjb_evaluate): n_stages evaluations from `terminal` (None: zeros).  labels [nS]: one
        stationary policy used at every stage; labels [nS, n_stages]: the stage with reference index k_s reads column k_s - 1
        (solve's idx_stages).  Returns {"J": the last stage's cost [nS], "J_stages": [nS, n_stages] (column k_s - 1) or None,
        "sweep_ms"}."""
        nS, dt = self.spec.nS, self.spec.j_dtype
        n_stages = int(n_stages)
        lab = self._labels(labels, [(nS,), (nS, n_stages)])
        per_stage = 1 if np.ndim(labels) == 2 else 0
        t = None if terminal is None else _j_vector(terminal, dt, nS, "terminal")
        J = np.empty(nS, dtype=dt)
        Js = np.zeros((nS, max(n_stages, 0)), dtype=dt, order="F") if keep_J else None
        ms = C.c_double(0.0)
        self._check(self.lib.hjb_evaluate(self._h, n_stages, None if t is None else t.ctypes.data, lab.ctypes.data, per_stage,
                                          J.ctypes.data, None if Js is None else Js.ctypes.data, C.byref(ms)))
        return {"J": J, "J_stages": Js, "sweep_ms": ms.value}

    def probe_stage(self, probe, J_next=None):
        """One stage of the debug taps from a host J_next (hjb_probe_stage)."""
        out, pb = _probe_block(self.spec, probe, 0)
        if J_next is None and "j_interp" in out:
            raise ValueError("j_interp needs J_next")
        Jn = None if J_next is None else _j_vector(J_next, self.spec.j_dtype, None, "J_next")     # of any size: this call asks for none
        self._check(self.lib.hjb_probe_stage(self._h, None if Jn is None else Jn.ctypes.data, C.byref(pb)))
        return out


class MultiBackup(_Handle):
    """A problem partitioned along its last state axis over several devices of THIS process (hjb_create_multi /
    hjb_solve_multi): per stage the halo planes travel device to device while the interior planes are computed.
    `devices` may repeat a device (several slabs on one GPU: how the path is tested on a 1-GPU box)."""

    _handle, _destroy, _last_error = "_m", "hjb_destroy_multi", "hjb_multi_last_error"

    def __init__(self, spec: ProblemSpec, devices):
        self.lib = load_library()
        self.spec = spec
        self._cprob, self._keep = spec.to_c()
        self._m = C.c_void_p()
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        self._created(self.lib.hjb_create_multi(C.byref(self._cprob), len(devices), devs, C.byref(self._m)))
        self.n_slabs = len(devices)

    def slab_info(self, i):
        v = [C.c_int32() for _ in range(6)]
        self._check(self.lib.hjb_multi_slab_info(self._m, int(i), *[C.byref(x) for x in v]))
        return dict(zip(("begin", "end", "halo_lo", "halo_hi", "split", "kernel_variant"), (x.value for x in v)))

    def set_option(self, key, value):
        self._check(self.lib.hjb_multi_set_option(self._m, key.encode(), int(value)))

    def solve(self, n_stages, terminal=None, keep_J=False, keep_idx=False, monitor_period=0, monitor_tol=0.0, progress=None,
              progress_every_stage=False):
        o, out, keep = _sweep_args(self.spec, n_stages, terminal=terminal, keep_J=keep_J, keep_idx=keep_idx, monitor_period=monitor_period,
                                   monitor_tol=monitor_tol, progress=progress, progress_every_stage=progress_every_stage)
        res = _abi.hjb_result()                                                 # keep: alive until hjb_solve_multi has returned
        self._check(self.lib.hjb_solve_multi(self._m, C.byref(o), C.byref(res)))
        ret = _sweep_result(out, res)
        del ret["probe"]                                                        # hjb_solve_multi takes no probe: its dict has no such key
        return ret


class RankSlab(_Handle):
    """One rank's share of a sweep partitioned over `world` processes, one per GPU (hjb_rank_create / hjb_rank_stage):
    the library builds the slab handle and - with overlap and an interior - the interior and strip handles, and enqueues
    a whole stage (interior on the compute stream, strips behind the halos on streams of their own) in one call."""

    _handle, _destroy, _last_error = "_r", "hjb_rank_destroy", "hjb_rank_last_error"

    def __init__(self, spec: ProblemSpec, device, rank, world, overlap=True):
        self.lib = load_library()
        self.spec = spec
        self._cprob, self._keep = spec.to_c()
        self._r = C.c_void_p()
        self._created(self.lib.hjb_rank_create(C.byref(self._cprob), int(device), int(rank), int(world), 1 if overlap else 0,
                                               C.byref(self._r)))
        self.refresh()

    def refresh(self):
        """Re-read what the library reports for this rank (the kernel variant changes with set_option)."""
        v = (C.c_int32 * 10)()
        self._check(self.lib.hjb_rank_info(self._r, v))
        (self.begin, self.end, self.halo_lo, self.halo_hi, self.split, self.kernel_variant, self.need_lo, self.need_hi,
         self.idx_bytes, self.n_planes) = (int(x) for x in v)

    def stage(self, dJ_in, dJ_out, d_idx, compute_stream=0, halo_stream=0):
        self._check(self.lib.hjb_rank_stage(self._r, _ptr(dJ_in), _ptr(dJ_out), _ptr(d_idx), _stream(compute_stream), _stream(halo_stream)))

    def fill_separable(self, vecs, dJ, stream=0):
        """dJ (this rank's haloed buffer) = ((vecs[0][i0] + vecs[1][i1]) + ...) on the rank's planes, halos included; vecs are the
        GLOBAL vectors (hjb_rank_fill_separable)."""
        _fill_separable(self, self.lib.hjb_rank_fill_separable, vecs, dJ, stream)

    def stage_post(self, dJ_in, dJ_out, d_idx, compute_stream=0, halo_stream=0):
        """The stage with the boundary strips first (hjb_rank_stage_post): their halos are already in dJ_in."""
        self._check(self.lib.hjb_rank_stage_post(self._r, _ptr(dJ_in), _ptr(dJ_out), _ptr(d_idx), _stream(compute_stream),
                                                 _stream(halo_stream)))

    def wait_strips(self, stream):
        """`stream` waits for the last stage's boundary strips; -> True when they cover every plane a neighbour needs."""
        cov = C.c_int32(0)
        self._check(self.lib.hjb_rank_wait_strips(self._r, _stream(stream), C.byref(cov)))
        return bool(cov.value)

    def set_option(self, key, value):
        self._check(self.lib.hjb_rank_set_option(self._r, key.encode(), int(value)))
        self.refresh()

    def get_option(self, key):
        v = C.c_int64()
        self._check(self.lib.hjb_rank_get_option(self._r, key.encode(), C.byref(v)))
        return int(v.value)

    def check_device_status(self, stream=0):
        self._check(self.lib.hjb_rank_check_status(self._r, _stream(stream)))


def suggest_axis_order(spec):
    """The labelling of the state axes under which the library runs its fastest stage kernel on `spec`
    (hjb_problem_suggest_order, the call a MATLAB host makes through matlab/hjbdp_solve.m): a tuple for
    `permute_state_axes`, or None when there is nothing to gain.  Needs the library, not a GPU."""
    lib = load_library()
    if spec.model is not None:
        return None
    b = C.c_void_p()
    n = (C.c_int32 * spec.D)(*spec.n)
    m = (C.c_int32 * spec.C)(*spec.m)
    dt = _abi.HJB_F64 if spec.dtype == np.float64 else _abi.HJB_F32

    def ok(st):
        if st != _abi.HJB_OK:
            msg = lib.hjb_problem_last_error(b)
            raise HjbError(st, (msg or b"").decode())
    ok(lib.hjb_problem_new(spec.D, spec.C, n, m, dt, spec.index_base, C.byref(b)))
    try:
        if spec.table_dtype is not None:
            ok(lib.hjb_problem_set_types(b, _abi.HJB_IDX_I32, _abi.HJB_TAB_F64))
        for a in range(spec.D):
            k = np.ascontiguousarray(spec.knots[a], dtype=np.float64)
            ok(lib.hjb_problem_set_knots(b, a, k.ctypes.data_as(C.POINTER(C.c_double)), k.size))
            for t in spec.next_terms[a]:
                v = np.ascontiguousarray(np.asarray(t.data, dtype=spec.table_dtype or spec.dtype).reshape(-1, order="F"))
                ok(lib.hjb_problem_add_next_term(b, a, sum(1 << d for d in t.dims), v.ctypes.data, v.size))
        order = (C.c_int32 * spec.D)()
        found = C.c_int32(0)
        ok(lib.hjb_problem_suggest_order(b, order, C.byref(found)))
        return tuple(order) if found.value else None
    finally:
        lib.hjb_problem_free(b)


def _batch_groups(variants, group_axes, specs):
    """Which problems of a solve_batch call share a launch: the ordered groups of member indices.  variants: every handle's kernel
    variant; group_axes: its column sweep's group axis (read only where the variant is 7).  Column-sweep problems (variant 7)
    share by (group axis, float64 cost or not), table-kernel problems (variant 5) of D <= 4 by (J type, D); every other problem
    is alone."""
    groups = {}
    for i, (v, s) in enumerate(zip(variants, specs)):
        if v == 7:
            key = ("colsweep", group_axes[i], s.cost_dtype is not None)
        elif v == 5 and s.D <= 4:
            key = ("tabled", np.dtype(s.j_dtype).str, s.D)
        else:
            key = ("alone", i)
        groups.setdefault(key, []).append(i)
    # The table kernel is one state per thread: a batch pays off while ALL its states are resident at once (a launch-bound stage);
    # beyond one round of the wave slots (256 CUs x 32 waves x 64 lanes) the launches run round after round and three chains on
    # three streams overlap better than one launch (Solver_attitude.simplified_run's 3 x 3e5 states: 130 ms batched, 82 ms as
    # chains - profiles/r06_batch_attitude.log).  Such a group is dissolved; its members go behind the groups that stay.
    for key in [k for k in groups if k[0] == "tabled"]:
        if len(groups[key]) > 1 and sum(specs[i].nS for i in groups[key]) > 256 * 32 * 64:
            for i in groups.pop(key):
                groups[("alone", i)] = [i]
    return list(groups.values())


def _batch_cs_split(specs, variants, own_splits, any_cost64):
    """Parts per column for the column-sweep problems (variant 7) of a solve_batch call, 0 to leave every handle its own.  A handle
    alone picks as many parts as fill the device (it is one wave's chain of round trips), and every part primes its rows again: up
    to twice the work per column.  These problems are in flight TOGETHER, so the parts are what lets all their columns fill about
    one round of the wave slots - the library does the same inside a batch for the columns it sees; here every chain of the call
    is counted (profiles/r06_batch_split.log).  own_splits: the cs_split each of those problems chose, in their order (read only
    as far as the answer needs); any_cost64: one of them has a float64 cost."""
    cols = sum(-(-s.n[0] // 60) * s.n[2] * s.n[3] for s, v in zip(specs, variants) if v == 7)
    slots = (5 if any_cost64 else 6) * 4 * 256          # waves per SIMD of the form that runs (86 / 80 registers) x SIMDs
    split = max(1, slots // max(cols, 1))
    return split if all(split < own for own in own_splits) else 0


def _solve_group(lib, bks, members, n_stages, kw):
    """One group of solve_batch on the calling thread -> (its members' dicts in order, the sizes of the launches they ran in):
    several members as ONE hjb_solve_batch call; a member alone in its shape, or a group the library does not take
    (HJB_E_UNSUPPORTED), as plain sweeps side by side."""
    from concurrent.futures import ThreadPoolExecutor
    if len(members) > 1:
        m = len(members)
        built = [_sweep_args(bks[i].spec, n_stages, **kw) for i in members]     # alive until hjb_solve_batch has returned
        ress = [_abi.hjb_result() for _ in members]
        hs = (C.c_void_p * m)(*[bks[i]._h for i in members])
        optp = (C.POINTER(_abi.hjb_solve_opts) * m)(*[C.pointer(o) for o, _, _ in built])
        resp = (C.POINTER(_abi.hjb_result) * m)(*[C.pointer(r) for r in ress])
        st = lib.hjb_solve_batch(m, hs, optp, resp)
        if st == _abi.HJB_OK:
            return [_sweep_result(out, r) for (_, out, _), r in zip(built, ress)], [m]
        if st != _abi.HJB_E_UNSUPPORTED:
            _check(lib, None, st)
        with ThreadPoolExecutor(max_workers=m) as ex:
            return list(ex.map(lambda i: bks[i].solve(n_stages, **kw), members)), [1] * m
    return [bks[members[0]].solve(n_stages, **kw)], [1]


def solve_batch(specs, n_stages, device=0, monitor_period=0, monitor_tol=0.0, progress=None, monitor_single=False, cs_split=None,
                options=None):
    """Independent sweeps side by side with as few launch chains as the library can make of them (the four channels of
    Solver_pos_att.simplified_run, pos-att/Solver_pos_att.m:197-242): problems that run on the column-sweep kernel with the same group
    axis, or on the table kernel's 32-bit form with one (dtype, D), share ONE launch per stage (hjb_solve_batch); each such group, and
    every problem that is alone in its shape, gets a host thread and a stream of its own (the device runs two launch chains at full rate: three channels + one is two chains).  Every
    problem keeps its own monitor sums and stop decision; results equal Backup.solve's bit for bit.
    options: one dict per problem of hjb_set_option keys and values, set on its handle right after it is created.
    -> (outs, wall_ms, variants, group sizes)"""
    import time
    from concurrent.futures import ThreadPoolExecutor
    t0 = time.perf_counter()
    lib = load_library()
    n = len(specs)
    kw = dict(monitor_period=monitor_period, monitor_tol=monitor_tol, progress=progress, monitor_single=monitor_single)
    with ThreadPoolExecutor(max_workers=max(1, n)) as ex:
        bks = list(ex.map(lambda s: Backup(s, device=device), specs))
    t_made = time.perf_counter()
    t_run = t_made
    try:
        for bk, o in zip(bks, options or ()):
            for k, v in (o or {}).items():
                bk.set_option(k, v)
        variants = [bk.info()["kernel_variant"] for bk in bks]
        groups = _batch_groups(variants, [bk.get_option("cs_group_axis") if v == 7 else None for bk, v in zip(bks, variants)], specs)
        cs = [i for i in range(n) if variants[i] == 7]
        if cs_split is None and len(cs) > 1:
            cs_split = _batch_cs_split(specs, variants, (bks[i].get_option("cs_split") for i in cs),
                                       any(specs[i].cost_dtype is not None for i in cs))

        def run(members):
            for i in members:
                if cs_split and variants[i] == 7:
                    bks[i].set_option("cs_split", int(cs_split))
            return _solve_group(lib, bks, members, n_stages, kw)
        outs = [None] * n
        sizes = []
        with ThreadPoolExecutor(max_workers=max(1, len(groups))) as ex:
            for members, (res, ms) in zip(groups, ex.map(run, groups)):
                sizes += ms
                for i, r in zip(members, res):
                    outs[i] = r
        t_run = time.perf_counter()
    finally:
        for bk in bks:
            bk.close()
    t_end = time.perf_counter()
    solve_batch.last_phases_ms = {"create": (t_made - t0) * 1e3, "sweep": (t_run - t_made) * 1e3, "close": (t_end - t_run) * 1e3}
    return outs, (t_end - t0) * 1e3, variants, sizes


def store_channel_results(solver, built, outs, n_st, keep_policy, u_vector):
    """Shared end of Solver_position.simplified_run and Solver_attitude.simplified_run: what the three channels' sweeps leave on
    `solver`.  built[ch] = (spec, the channel's two grid vectors), outs[ch] its sweep's dict.  Per channel F_values and U_idx
    (1-based) on the grid, sweep_ms, and U<ch+1>_Opt, the 'nearest' policy over U_vector[U_idx - 1]; with keep_policy the labels
    of all n_st stages U_idx_stages[ch] [n_a, n_b, n_st] and their values U_Opt_stages[ch] = u_vector[labels - 1], else None."""
    from .solver_position import NearestPolicy
    solver.U_Opt_stages = solver.U_idx_stages = None
    if keep_policy:
        solver.U_idx_stages = [out["idx_stages"].reshape(len(s_a), len(s_b), n_st, order="F") for (_, s_a, s_b), out in zip(built, outs)]
        solver.U_Opt_stages = [u_vector[ix - 1] for ix in solver.U_idx_stages]
    for ch, ((_, s_a, s_b), out) in enumerate(zip(built, outs)):
        shape = (len(s_a), len(s_b))
        solver.F_values[ch] = out["J"].reshape(shape, order="F")
        solver.U_idx[ch] = out["idx"].reshape(shape, order="F")
        solver.sweep_ms[ch] = out["sweep_ms"]
        setattr(solver, "U%d_Opt" % (ch + 1), NearestPolicy([s_a, s_b], solver.U_vector[solver.U_idx[ch] - 1]))


def channel_policy_cost(solver, build, n_stages, stationary):
    """Shared body of Solver_position.policy_cost and Solver_attitude.policy_cost_simplified: the cost over the grid of flying the
    labels a simplified_run left on `solver`, per channel (Backup.evaluate; no min, terminal cost zero).  build(ch) -> the channel's
    ProblemSpec ON THE GRID THE RUN USED.  stationary: U_idx[ch] at every one of n_stages stages (None: N_stage - 1); else the
    per-stage U_idx_stages of simplified_run(keep_policy=True).  The three channels run in turn: an evaluation stage is a fraction
    of a backup.  Leaves the device times in solver.policy_cost_ms."""
    if stationary:
        n_st = solver.N_stage - 1 if n_stages is None else int(n_stages)
        labels = [np.asarray(solver.U_idx[ch]) for ch in range(3)]
    else:
        if solver.U_idx_stages is None:
            raise RuntimeError("stationary=False needs simplified_run(keep_policy=True)")
        n_st = solver.U_idx_stages[0].shape[-1]
        if n_stages is not None and int(n_stages) != n_st:
            raise ValueError("the run kept %d stages of labels, n_stages=%d" % (n_st, int(n_stages)))
        labels = [np.asarray(ix) for ix in solver.U_idx_stages]
    out = []
    solver.policy_cost_ms = [None] * 3
    for ch in range(3):
        spec = build(ch)
        lab = labels[ch].reshape((spec.nS,) if stationary else (spec.nS, n_st), order="F").astype(spec.idx_np_dtype)
        with Backup(spec, device=solver.device) as bk:
            res = bk.evaluate(n_st, np.asfortranarray(lab))
        solver.policy_cost_ms[ch] = res["sweep_ms"]
        out.append(res["J"].reshape(spec.n, order="F"))
    return out


def solve_many(specs, n_stages, device=0, **solve_kw):
    """Independent sweeps (the three axis channels of Solver_position / Solver_attitude.simplified_run, the four
    runs of Solver_pos_att.simplified_run) in flight together: one handle and one host thread per sweep, each on
    its handle's own HIP stream.  A channel's stage kernel fills a few percent of the chip and the sweep is a
    chain of thousands of dependent launches, so running channels side by side costs nothing and divides the
    wall time.  `solve_kw` values may be lists (one entry per spec).  Returns (outs, wall_ms, variants)."""
    import time
    from concurrent.futures import ThreadPoolExecutor

    def one(i):
        kw = {k: (v[i] if isinstance(v, (list, tuple)) else v) for k, v in solve_kw.items()}
        with Backup(specs[i], device=device) as bk:
            out = bk.solve(n_stages, **kw)
            return out, bk.info()["kernel_variant"]
    t0 = time.perf_counter()
    if len(specs) == 1:
        res = [one(0)]
    else:
        with ThreadPoolExecutor(max_workers=len(specs)) as ex:
            res = list(ex.map(one, range(len(specs))))
    wall_ms = (time.perf_counter() - t0) * 1e3
    return [r[0] for r in res], wall_ms, [r[1] for r in res]

