"""A Dynamic_Solver whose results are set by hand and a recording stand-in for hjbdp.core.Rollout: what the solver's campaign
methods call on the object they open, in order, with no run() and no device.  The shim tests compare the record with the MATLAB
shims' calllib sequences (as_entry_points, shim_order)."""
import numpy as np


def hand_set_solver():
    """N = 3 stages on a 3-knot grid, two controls, a two-node disturbance: what run() would have left, typed in"""
    import hjbdp
    ds = hjbdp.Dynamic_Solver(precision="double")
    ds.N, ds.S = 3, 2
    ds.A, ds.B = np.array([[1.0, 0.1], [0.0, 1.0]]), np.array([[0.0], [0.1]])
    ds.Q, ds.R = np.diag([1.0, 0.5]), 0.25
    ds.s_r = np.array([-1.0, 0.0, 1.0])
    ds._U_mesh = np.array([-1.0, 1.0])
    ds.J_star = np.arange(27, dtype=np.float64).reshape(3, 3, 3)
    ds.u_star_idxs = np.ones((3, 3, 2), dtype=np.int32)
    ds.disturbance = (np.array([[0.0, 0.125], [0.0, -0.25]]), [0.75, 0.25], "expect")
    return ds


class RecordingRollout:
    """Stands where hjbdp.core.Rollout stands.  Every call is appended to RecordingRollout.calls as (name, args, kwargs),
    construction as "create" and close as "destroy"; the campaign methods return dicts of the real shapes (zero records), any
    other run_* is recorded and refused."""
    calls = []

    def __init__(self, knots, labels, u_table, index_base=1, device=0):
        self.D = len(knots)
        self._rec("create", knots, labels, u_table, index_base=index_base, device=device)

    def _rec(self, name, *args, **kw):
        type(self).calls.append((name, args, kw))

    def close(self):
        self._rec("destroy")

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __getattr__(self, name):                      # set_model, set_values, set_lookahead, set_noise, and whatever else is tried
        def call(*args, **kw):
            self._rec(name, *args, **kw)
            if name.startswith("run"):
                raise AssertionError("the campaign methods must not call %s" % name)
        return call

    def _campaign(self, X0, n_samples, hist=None):
        from hjbdp import core
        ns = np.asarray(X0).reshape(self.D, -1).shape[1]
        stats = np.zeros((ns, 8))
        stats[:, 3] = 1.0                             # min 0, max 1: the two-pass methods need a range
        out = {**core._campaign_dict(stats, int(n_samples)), "device_ms": 0.0}
        if hist is not None:
            lo, hi, nb, counts = core._campaign_hist_args(ns, hist)
            counts[:, 1] = int(n_samples)
            out.update(hist=counts, hist_lo=lo, hist_hi=hi)
        return out

    def run_campaign(self, X0, plane_of_step, n_samples, **kw):
        self._rec("run_campaign" if kw.get("hist") is None else "run_campaign_hist", X0, plane_of_step, n_samples, **kw)
        return self._campaign(X0, n_samples, kw.get("hist"))

    def run_lookahead_campaign(self, X0, value_plane_of_step, n_samples, **kw):
        self._rec("run_lookahead_campaign", X0, value_plane_of_step, n_samples, **kw)
        return self._campaign(X0, n_samples)

    def run_lookahead_campaign_hist(self, X0, value_plane_of_step, n_samples, hist, **kw):
        self._rec("run_lookahead_campaign_hist", X0, value_plane_of_step, n_samples, hist, **kw)
        return self._campaign(X0, n_samples, hist)

    def run_campaign_pair(self, X0, a, b, n_samples, **kw):
        from hjbdp import core
        self._rec("run_campaign_pair", X0, a, b, n_samples, **kw)
        one = self._campaign(X0, n_samples)
        one.pop("device_ms")
        return {"a": one, "b": dict(one), **core._campaign_pair_dict(np.zeros_like(one["stats"]), int(n_samples)), "device_ms": 0.0}


def record(monkeypatch, method, *args, **kw):
    """hand_set_solver().<method>(*args, **kw) on the stand-in -> (the result, the calls made)"""
    import hjbdp.core
    monkeypatch.setattr(hjbdp.core, "Rollout", RecordingRollout)
    monkeypatch.setattr(RecordingRollout, "calls", [])
    out = getattr(hand_set_solver(), method)(*args, **kw)
    return out, list(RecordingRollout.calls)


def as_entry_points(calls):
    """the record as the library's entry points: hjb_rollout_ in front of every name"""
    return ["hjb_rollout_" + name for name, _, _ in calls]


def shim_order(body):
    """A shim's calllib sequence in the order the calls RUN: it registers the destroy as an onCleanup right behind the create, so
    the text has it second and the run has it last"""
    assert body[:2] == ["hjb_rollout_create", "hjb_rollout_destroy"], body
    return body[:1] + body[2:] + body[1:2]
