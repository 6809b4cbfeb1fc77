"""Dynamic_Solver - host mirror of the reference's Kirk Ch.3 two-state example
(test/Dynamic_Solver.m).  Same property names, same methods:

    objA = Dynamic_Solver(); objA.run(); objA.get_optimal_path()

`run` (Dynamic_Solver.m:66-105) builds the grid vectors and hands the backward
sweep - the `for k=1:N-1` loop around J_state_M (:202-220) - to libhjbdp; the
dx*dx*du tables of a_D_M (:184-188) and g_D (:196-200) are never materialised,
they are passed as 1-D broadcast terms evaluated in MATLAB's left-to-right order.

precision='single' is the committed revision's typing (s_r = single(linspace..),
:69; single tables, double U_mesh); precision='double' is the revision that
produced test/obj_1.mat (test/test_coder.m:19-36), used for the parity fixture.
"""
from __future__ import annotations

import contextlib

import numpy as np

from .core import Backup
from .disturbance import actuator_nodes
from .matlab_compat import interp_linear_point, linspace
from .problem import ProblemSpec, Term


class Dynamic_Solver:
    def __init__(self, precision="single"):
        # Dynamic_Solver.m:47-64
        self.checkstagesXJF = 1
        self.Q = np.array([[0.25, 0.0], [0.0, 0.05]])
        self.A = np.array([[0.9974, 0.0539], [-0.1078, 1.1591]])
        self.B = np.array([[0.0013], [0.0539]])
        self.R = 0.05
        self.N = 200
        self.S = 2
        self.C = 1
        self.dx = 100
        self.du = 1000
        self.x_max = 3.0
        self.x_min = -2.5
        self.u_max = 10.0
        self.u_min = -40.0
        self.H = None  # unused by the reference too (terminal cost is 0, :83-84)
        self.precision = precision
        self.device = 0
        self.disturbance = None   # (offsets [2, W], weights or None, 'expect' / 'worst'): run() and policy_cost() under it (ProblemSpec.disturbance)
        self.actuator_noise = None   # (eps [W], weights or None, 'expect' / 'worst'): the actuator delivers u (1 + eps_w) - run() and policy_cost() under d_w(l) = B U_mesh[l] eps[w] (ProblemSpec.control_disturbance); not with self.disturbance
        # results
        self.s_r = None
        self.u_star = None
        self.u_star_idx = None
        self.J_star = None
        self.X1_mesh = None
        self.X2_mesh = None
        self.F_values = None  # obj.F.Values after the sweep (= J at stage 1)
        self.sweep_ms = None
        self.X_path = None
        self.U_path = None
        self.u_star_idxs = None

    # ------------------------------------------------------------------
    def build_spec(self):
        """Grid + broadcast terms with MATLAB's typing rules."""
        A, B, Q, R = self.A, self.B, self.Q, self.R
        if self.precision == "single":
            dt = np.float32
            s_r = linspace(self.x_min, self.x_max, self.dx).astype(np.float32)  # :69
            U_mesh = linspace(self.u_min, self.u_max, self.du)                  # :72 (double)
            f = np.float32
            # A(1)*X1 (double scalar * single array -> single), B(1)*U (double) cast on the add
            nxt = [[Term((0,), f(A[0, 0]) * s_r), Term((1,), f(A[0, 1]) * s_r), Term((2,), (B[0, 0] * U_mesh).astype(f))],
                   [Term((0,), f(A[1, 0]) * s_r), Term((1,), f(A[1, 1]) * s_r), Term((2,), (B[1, 0] * U_mesh).astype(f))]]
            cost = [Term((0,), f(Q[0, 0]) * s_r ** 2), Term((1,), f(Q[1, 1]) * s_r ** 2),
                    Term((2,), (R * U_mesh ** 2).astype(f))]  # :198-199 (Q(1), Q(4): diagonal only)
        elif self.precision == "double":
            dt = np.float64
            s_r = linspace(self.x_min, self.x_max, self.dx)                    # test_coder.m:19
            U_mesh = linspace(self.u_min, self.u_max, self.du)
            nxt = [[Term((0,), A[0, 0] * s_r), Term((1,), A[0, 1] * s_r), Term((2,), B[0, 0] * U_mesh)],
                   [Term((0,), A[1, 0] * s_r), Term((1,), A[1, 1] * s_r), Term((2,), B[1, 0] * U_mesh)]]
            cost = [Term((0,), Q[0, 0] * s_r ** 2), Term((1,), Q[1, 1] * s_r ** 2), Term((2,), R * U_mesh ** 2)]
        else:
            raise ValueError("precision must be 'single' or 'double'")
        self.s_r = s_r
        self._U_mesh = U_mesh
        cdist = None
        if self.actuator_noise is not None:
            if self.disturbance is not None:
                raise ValueError("Dynamic_Solver takes `disturbance` or `actuator_noise`, not both")
            eps, wts = self.actuator_noise[0], self.actuator_noise[1] if len(self.actuator_noise) > 1 else None
            off, wts = actuator_nodes(B, np.asarray(U_mesh, dtype=np.float64), eps, wts)
            cdist = (off, wts, self.actuator_noise[2] if len(self.actuator_noise) > 2 else "expect")
        return ProblemSpec([s_r, s_r], [self.du], nxt, cost, dtype=dt, index_base=1, disturbance=self.disturbance,
                           control_disturbance=cdist)

    def run(self):
        spec = self.build_spec()
        s_r, U_mesh = self.s_r, self._U_mesh
        self.X1_mesh, self.X2_mesh = np.meshgrid(s_r, s_r, indexing="ij")  # ndgrid, :70
        n_st = self.N - 1                                                  # for k=1:N-1, :86
        # Dynamic_Solver.m:212-219 (`checkstagesXJF`, default 1): per stage the reference copies the fixed sub-block
        # (50:55, 52:57, 105) of J_current_state, X_next_M1 and X_next_M2; the library evaluates that block on the GPU
        # (hjb_probe).  MATLAB raises an index error when dx < 57 or du < 105; the mirror leaves the taps None instead
        # (the fixture revision test/test_coder.m has no taps and runs at dx = 35).
        probe = None
        if self.checkstagesXJF and self.dx >= 57 and self.du >= 105 and self.disturbance is None and self.actuator_noise is None:    # (the taps are the nominal next state's)
            probe = {"lo": (49, 51), "hi": (55, 57), "control": (104,), "want": ("g", "x_next", "j_interp")}
        with Backup(spec, device=self.device) as bk:
            out = bk.solve(n_st, keep_J=True, keep_idx=True, probe=probe)
        self.J_current_state_check = self.X_next_M1_check = self.X_next_M2_check = self.J_F_next_check = None
        if probe is not None:
            # plane k_s - 1 holds stage k_s; the reference indexes its taps by the loop counter k = N - k_s
            flip = lambda a: a[..., ::-1]
            self.J_current_state_check = flip(out["probe"]["g"])
            self.X_next_M1_check = flip(out["probe"]["x_next"][:, :, 0, :])
            self.X_next_M2_check = flip(out["probe"]["x_next"][:, :, 1, :])
            self.J_F_next_check = flip(out["probe"]["j_interp"])        # commented out in the reference (:215)
        self.sweep_ms = out["sweep_ms"]
        dt = spec.dtype
        shape = (self.dx, self.dx, self.N)
        # stage k_s lives in column k_s-1; stage N = terminal (zeros)  (:77-80,:100)
        self.J_star = np.zeros(shape, dtype=dt)
        self.u_star = np.zeros(shape, dtype=dt)
        self.J_star[:, :, : n_st] = out["J_stages"].reshape((self.dx, self.dx, n_st), order="F")
        idx = out["idx_stages"].reshape((self.dx, self.dx, n_st), order="F")  # 1-based
        self.u_star[:, :, : n_st] = U_mesh[idx - 1].astype(dt)               # u_star(:,:,k_s) = U_mesh(u_star_idx)
        self.u_star_idx = idx[:, :, 0].copy()      # value left in obj.u_star_idx after the loop (k_s = 1)
        self.u_star_idxs = idx                     # every stage's labels, [dx, dx, N-1] (:100)
        self.F_values = self.J_star[:, :, 0].copy()
        return self

    def policy_cost(self):
        """The cost of the stored per-stage policy (u_star_idxs) over the whole grid, from the terminal cost run() used (zeros):
        [dx, dx, N-1] with stage k_s in plane k_s - 1, by the fixed-label sweep (Backup.evaluate) - no min is taken.  On the
        policy run() itself left it equals J_star[:, :, :N-1] bit for bit; edit u_star_idxs (or the cost weights) first to
        judge another policy (or this one under another cost)."""
        if self.u_star_idxs is None:
            raise RuntimeError("run() first")
        spec = self.build_spec()
        idx = np.asarray(self.u_star_idxs)
        n_st = idx.shape[-1]
        lab = np.ascontiguousarray(idx.reshape(-1, n_st, order="F").astype(spec.idx_np_dtype), dtype=spec.idx_np_dtype)
        with Backup(spec, device=self.device) as bk:
            out = bk.evaluate(n_st, np.asfortranarray(lab), keep_J=True)
        self.policy_cost_ms = out["sweep_ms"]
        return out["J_stages"].reshape((self.dx, self.dx, n_st), order="F")

    # ------------------------------------------------------------------
    def a_D(self, X1, X2, Ui):
        # Dynamic_Solver.m:191-194
        return self.A @ np.array([X1, X2], dtype=np.float64) + self.B[:, 0] * Ui

    def get_optimal_path(self, X0=None, mode="Nssu", ssu_num=1):
        """Dynamic_Solver.m:108-181: closed-loop rollout with the stored policy.
        mode 'ssu' freezes the policy of stage `ssu_num` (1-based).  Returns
        (X [S,N], U [N]) instead of plotting."""
        if X0 is None:
            X0, mode, ssu_num = np.array([2.0, 1.0]), "Nssu", 1
        if self.u_star is None:
            raise RuntimeError("run() first")
        N = self.N
        knots = [np.asarray(self.s_r, dtype=np.float64)] * 2
        X = np.zeros((self.S, N))
        U = np.zeros(N)
        X[:, 0] = np.asarray(X0, dtype=np.float64).reshape(-1)
        for k in range(N - 1):
            USM = self.u_star[:, :, ssu_num - 1] if mode == "ssu" else self.u_star[:, :, k]
            U[k] = interp_linear_point(knots, USM, X[:, k])
            X[:, k + 1] = self.a_D(X[0, k], X[1, k], U[k])
        self.X_path, self.U_path = X, U
        if mode == "ssu":
            USTAR_OPT = self.u_star[:, :, 0].astype(np.float64)
            USM = self.u_star[:, :, ssu_num - 1].astype(np.float64)
            self.ssu_tol = float(np.sum(np.sum(USTAR_OPT - USM, axis=0) ** 2))
            self.ssu_err_first = abs(interp_linear_point(knots, USTAR_OPT, X[:, 0]) -
                                     interp_linear_point(knots, USM, X[:, 0]))
        return X, U

    def get_optimal_paths(self, X0s, mode="Nssu", ssu_num=1, method="linear"):
        """get_optimal_path (Dynamic_Solver.m:108-181) for many initial states at once, on the GPU (hjbdp.Rollout): X0s [S, n]
        (one initial state per column).  Returns X [S, N, n] and U [N, n] (U[N-1] = 0, as get_optimal_path leaves it); the
        closed-loop costs sum_k x'Qx + R u^2 over the N-1 steps are left in self.paths_cost [n].  The policy of stage k_s is
        U_mesh(u_star_idxs(:,:,k_s)) in the problem's precision, looked up in double on the double grid vectors, as
        get_optimal_path does; mode 'ssu' freezes stage ssu_num (1..N-1)."""
        opening = self._rollout("get_optimal_paths")
        N, S = self.N, self.S
        n_st = N - 1
        planes = self._stage_planes(mode, ssu_num)
        X0s = np.asarray(X0s, dtype=np.float64)
        X0s = X0s.reshape(S, -1)
        with opening as ro:
            out = ro.run(X0s, planes, method=method, keep_path=True)
        X = np.ascontiguousarray(out["X_path"].transpose(1, 2, 0))     # [n, S, N] -> [S, N, n]
        U = np.zeros((N, X0s.shape[1]))
        U[:n_st] = out["U_path"][:, 0, :].T
        self.paths_cost = out["cost"]
        return X, U

    def get_noisy_paths(self, X0s, n_samples, seed=0, mode="Nssu", ssu_num=1, method="linear"):
        """The stored policy flown under sampled process noise, on the GPU (hjbdp.Rollout.run_noisy): every start of X0s [S, n]
        n_samples times under self.disturbance's nodes - x+ = A x + B u + d_w, node w drawn per step with the set's weights; a
        'worst' set (no weights) is sampled uniformly.  Sample j of start i runs on stream i * n_samples + j of `seed`.
        Returns the closed-loop costs [n, n_samples] (sum_k x'Qx + R u^2 over the N-1 steps, of the states actually visited) and
        leaves their mean, standard deviation and maximum per start in self.noisy_cost_mean / _std / _max [n].  Beside
        policy_cost() on the same disturbance this is "promised against paid" in two calls."""
        opening = self._rollout("get_noisy_paths", noise=True)
        planes = self._stage_planes(mode, ssu_num)
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError("n_samples must be at least 1")
        X0s = np.asarray(X0s, dtype=np.float64).reshape(self.S, -1)
        n = X0s.shape[1]
        with opening as ro:
            out = ro.run_noisy(np.repeat(X0s, n_samples, axis=1), planes, seed=seed, first_stream=0, method=method)
        cost = out["cost"].reshape(n, n_samples)
        self.noisy_cost_mean, self.noisy_cost_std, self.noisy_cost_max = cost.mean(axis=1), cost.std(axis=1), cost.max(axis=1)
        self.noisy_paths_ms = out["device_ms"]
        return cost

    def _stage_planes(self, mode, ssu_num, values=False):
        """The plane every one of the N-1 steps reads, as `mode` / `ssu_num` choose it.  values=False, the label planes: step k
        (0-based) reads plane k, 'ssu' freezes plane ssu_num - 1.  values=True, the value planes behind the steps: step k reads
        plane k + 1 of J_star, 'ssu' freezes plane ssu_num."""
        n_st, first = self.N - 1, int(bool(values))
        if mode == "ssu":
            if not 1 <= int(ssu_num) <= n_st:
                raise ValueError("ssu_num must lie in 1..N-1 = %d" % n_st)
            return np.full(n_st, int(ssu_num) - 1 + first, dtype=np.int32)
        if mode == "Nssu":
            return np.arange(first, n_st + first, dtype=np.int32)
        raise ValueError("mode must be 'Nssu' or 'ssu'")

    def _rollout(self, who, values=False, lookahead=False, noise=False, actuator=False):
        """What `who` flies on: refuses at once what it cannot fly - no run() yet, no self.disturbance where the flight needs one,
        an unknown `lookahead` - and returns a context manager that opens an hjbdp.Rollout on the stored policy and closes it on
        the way out, whatever happens (an hjbdp.ActuatorRollout with `actuator`).  On the open object, in this order: set_model; set_values(J_star) with `values`;
        set_lookahead unless `lookahead` is False - 'disturbed': self.disturbance's set in its own mode, 'nominal': one zero node of weight
        1; set_noise(self.disturbance's nodes) with `noise`; set_actuator_noise(self.actuator_noise's eps and weights) with
        `actuator` (the flights of get_actuator_paths and its campaign forms, which need self.actuator_noise)."""
        from .core import ActuatorRollout, Rollout
        if actuator and self.actuator_noise is None:
            raise RuntimeError("%s needs self.actuator_noise = (eps [W], weights or None, mode)" % who)
        if self.u_star_idxs is None or (values and self.J_star is None):
            raise RuntimeError("run() first")
        if (lookahead is not False or noise) and self.actuator_noise is not None:
            raise RuntimeError("%s believes and flies an additive node set; under control-dependent noise (self.actuator_noise) the "
                               "flights are get_actuator_paths (the stored labels) and get_actuator_lookahead_paths (the value "
                               "function), with their campaign forms" % who)
        if (lookahead is not False or noise) and self.disturbance is None:
            raise RuntimeError("%s needs self.disturbance = (offsets [2, W], weights or None, mode)" % who)
        if lookahead is not False and lookahead not in ("disturbed", "nominal"):
            raise ValueError("lookahead must be 'disturbed' or 'nominal'")

        @contextlib.contextmanager
        def opened():
            s_r = np.asarray(self.s_r, dtype=np.float64)
            u_table = np.asarray(self._U_mesh).astype(self.J_star.dtype).astype(np.float64)
            with (ActuatorRollout if actuator else Rollout)([s_r, s_r], self.u_star_idxs, u_table, index_base=1, device=self.device) as ro:
                ro.set_model(self.A, self.B, q=np.diag(self.Q), r=[self.R])
                if values:
                    ro.set_values(self.J_star)
                if lookahead == "disturbed":
                    ro.set_lookahead(self.disturbance[0], self.disturbance[1], self.disturbance[2] if len(self.disturbance) > 2 else "expect")
                elif lookahead == "nominal":
                    ro.set_lookahead(np.zeros((self.S, 1)), [1.0], "expect")
                if noise:
                    ro.set_noise(self.disturbance[0], self.disturbance[1])
                if actuator:
                    ro.set_actuator_noise(self.actuator_noise[0], self.actuator_noise[1] if len(self.actuator_noise) > 1 else None)
                yield ro
        return opened()

    def get_noisy_cost_statistics(self, X0s, n_samples, seed=0, mode="Nssu", ssu_num=1, method="linear", cost_threshold=None,
                                  settle_tol=None):
        """get_noisy_paths' flights reduced per start on the GPU (hjbdp.Rollout.run_campaign): every start of X0s [S, n] flown
        n_samples times under self.disturbance's nodes, sample j of start i on stream i * n_samples + j of `seed`
        (get_noisy_paths' numbering: the same costs), and nothing of length n * n_samples exists on the host or on the device.
        Returns run_campaign's dict, one entry per start: stats [n, 8], mean, var, std, min, max, n_exceed (cost >
        cost_threshold), n_left (the flight left the grid), n_settled (|x_final| <= settle_tol on every axis), mean_settled,
        device_ms.  `mode` / `ssu_num` / `method` as in get_noisy_paths."""
        if int(n_samples) < 1:
            raise ValueError("n_samples must be at least 1")
        opening = self._rollout("get_noisy_cost_statistics", noise=True)
        planes = self._stage_planes(mode, ssu_num)
        with opening as ro:
            return ro.run_campaign(np.asarray(X0s, dtype=np.float64).reshape(self.S, -1), planes, int(n_samples), seed=seed,
                                   first_stream=0, method=method, cost_threshold=cost_threshold, settle_tol=settle_tol)

    def noisy_cost_map(self, n_samples, seed=0, mode="Nssu", ssu_num=1, method="linear", cost_threshold=None, settle_tol=None):
        """get_noisy_cost_statistics at every grid node: each entry shaped like the grid, [dx, dx] (stats [dx, dx, 8]), node
        (i, j) = (s_r[i], s_r[j]) flown from stream (i + dx * j) * n_samples on.  Beside policy_cost() on the same disturbance
        this is "promised against paid" over the whole grid: policy_cost()'s plane 0 is what the policy promises at a node,
        the map's mean (and, for a 'worst' set, its max) is what n_samples flights from that node paid."""
        return self._grid_map(self.get_noisy_cost_statistics(self._grid_starts(), n_samples, seed=seed, mode=mode, ssu_num=ssu_num,
                                                             method=method, cost_threshold=cost_threshold, settle_tol=settle_tol))

    def get_actuator_paths(self, X0s, n_samples, seed=0, mode="Nssu", ssu_num=1, method="linear"):
        """The stored policy flown under sampled ACTUATOR noise, on the GPU (hjbdp.ActuatorRollout.run_actuator): every start of X0s
        [S, n] n_samples times under self.actuator_noise - x+ = A x + B u (1 + eps_w), node w drawn per step with the set's
        weights; a 'worst' set (no weights) is sampled uniformly.  Sample j of start i runs on stream i * n_samples + j of `seed`
        (get_noisy_paths' numbering).  Returns the closed-loop costs [n, n_samples] (on the commanded controls and the states
        actually visited) and leaves their mean, standard deviation and maximum per start in self.actuator_cost_mean / _std /
        _max [n].  Beside policy_cost() under the same self.actuator_noise this is "promised against paid" in two calls."""
        opening = self._rollout("get_actuator_paths", actuator=True)
        planes = self._stage_planes(mode, ssu_num)
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError("n_samples must be at least 1")
        X0s = np.asarray(X0s, dtype=np.float64).reshape(self.S, -1)
        n = X0s.shape[1]
        with opening as ro:
            out = ro.run_actuator(np.repeat(X0s, n_samples, axis=1), planes, seed=seed, first_stream=0, method=method)
        cost = out["cost"].reshape(n, n_samples)
        self.actuator_cost_mean, self.actuator_cost_std, self.actuator_cost_max = cost.mean(axis=1), cost.std(axis=1), cost.max(axis=1)
        self.actuator_paths_ms = out["device_ms"]
        return cost

    def get_actuator_cost_statistics(self, X0s, n_samples, seed=0, mode="Nssu", ssu_num=1, method="linear", cost_threshold=None,
                                     settle_tol=None):
        """get_actuator_paths' flights reduced per start on the GPU (hjbdp.ActuatorRollout.run_actuator_campaign): the same streams, so
        the same costs, and nothing of length n * n_samples exists on the host or on the device.  Returns
        get_noisy_cost_statistics' dict, one entry per start."""
        if int(n_samples) < 1:
            raise ValueError("n_samples must be at least 1")
        opening = self._rollout("get_actuator_cost_statistics", actuator=True)
        planes = self._stage_planes(mode, ssu_num)
        with opening as ro:
            return ro.run_actuator_campaign(np.asarray(X0s, dtype=np.float64).reshape(self.S, -1), planes, int(n_samples), seed=seed,
                                            first_stream=0, method=method, cost_threshold=cost_threshold, settle_tol=settle_tol)

    def actuator_cost_map(self, n_samples, seed=0, mode="Nssu", ssu_num=1, method="linear", cost_threshold=None, settle_tol=None):
        """get_actuator_cost_statistics at every grid node: noisy_cost_map's shape and stream numbering - each entry [dx, dx]
        (stats [dx, dx, 8]), node (i, j) = (s_r[i], s_r[j]) flown from stream (i + dx * j) * n_samples on - under
        self.actuator_noise's eps and weights (a 'worst' set is sampled uniformly).  Beside policy_cost() this is "promised
        against paid" over the whole grid for the actuator-noise design: plane 0 of policy_cost() is the promise, the map's mean
        (for a 'worst' set its max) is what n_samples flights paid."""
        return self._grid_map(self.get_actuator_cost_statistics(self._grid_starts(), n_samples, seed=seed, mode=mode, ssu_num=ssu_num,
                                                                method=method, cost_threshold=cost_threshold, settle_tol=settle_tol))

    def _actuator_lookahead_rollout(self, who):
        """What the three actuator-lookahead flights fly on, beside _rollout (whose lookahead flights keep refusing
        self.actuator_noise: they believe and fly an additive set): refuses at once no self.actuator_noise and no run() yet, and
        returns a context manager that opens an hjbdp.ControlLookaheadRollout on the stored policy with set_model,
        set_values(J_star), set_control_lookahead(the table build_spec gives the backup, in the set's own mode) and
        set_actuator_noise(eps, weights): what was designed under is what is believed and what is flown."""
        from .core import ControlLookaheadRollout
        if self.actuator_noise is None:
            raise RuntimeError("%s needs self.actuator_noise = (eps [W], weights or None, mode)" % who)
        if self.u_star_idxs is None or self.J_star is None:
            raise RuntimeError("run() first")

        @contextlib.contextmanager
        def opened():
            off, wts, dist_mode = self.build_spec().control_disturbance
            s_r = np.asarray(self.s_r, dtype=np.float64)
            u_table = np.asarray(self._U_mesh).astype(self.J_star.dtype).astype(np.float64)
            with ControlLookaheadRollout([s_r, s_r], self.u_star_idxs, u_table, index_base=1, device=self.device) as ro:
                ro.set_model(self.A, self.B, q=np.diag(self.Q), r=[self.R])
                ro.set_values(self.J_star)
                ro.set_control_lookahead(off, wts, dist_mode)
                ro.set_actuator_noise(self.actuator_noise[0], self.actuator_noise[1] if len(self.actuator_noise) > 1 else None)
                yield ro
        return opened()

    def get_actuator_lookahead_paths(self, X0s, n_samples=None, seed=0, mode="Nssu", ssu_num=1):
        """The closed loop of the cost-to-go designed under ACTUATOR noise, on the GPU
        (hjbdp.ControlLookaheadRollout.run_control_lookahead): get_lookahead_paths for self.actuator_noise - the control of U_mesh
        that minimises x'Qx + R u^2 + E_w J_{k+1}(A x + B u (1 + eps_w)) (or max_w, in the set's own mode) at the state actually
        visited, the controller run() under self.actuator_noise is exactly optimal for.  Planes and `mode` / `ssu_num` as in
        get_greedy_paths.
        n_samples None: the nominal plant; returns X [S, N, n] and U [N, n] as get_greedy_paths does and leaves the costs in
        self.actuator_lookahead_cost [n].  n_samples given: every start flown n_samples times on get_actuator_paths' plant,
        sample j of start i on stream i * n_samples + j of `seed` (get_actuator_paths' numbering: common random numbers with the
        stored labels); returns the closed-loop costs [n, n_samples], on the commanded controls, and leaves their mean, standard
        deviation and maximum per start in self.actuator_lookahead_cost_mean / _std / _max [n].  The kernel's time:
        self.actuator_lookahead_paths_ms."""
        opening = self._actuator_lookahead_rollout("get_actuator_lookahead_paths")
        N, S = self.N, self.S
        n_st = N - 1
        planes = self._stage_planes(mode, ssu_num, values=True)
        if n_samples is not None and int(n_samples) < 1:
            raise ValueError("n_samples must be at least 1")
        X0s = np.asarray(X0s, dtype=np.float64).reshape(S, -1)
        n = X0s.shape[1]
        with opening as ro:
            if n_samples is None:
                out = ro.run_control_lookahead(X0s, planes, keep_path=True)
            else:
                out = ro.run_control_lookahead(np.repeat(X0s, int(n_samples), axis=1), planes, actuator=True, seed=seed, first_stream=0)
        self.actuator_lookahead_paths_ms = out["device_ms"]
        if n_samples is not None:
            cost = out["cost"].reshape(n, int(n_samples))
            self.actuator_lookahead_cost_mean, self.actuator_lookahead_cost_std = cost.mean(axis=1), cost.std(axis=1)
            self.actuator_lookahead_cost_max = cost.max(axis=1)
            return cost
        X = np.ascontiguousarray(out["X_path"].transpose(1, 2, 0))     # [n, S, N] -> [S, N, n]
        U = np.zeros((N, n))
        U[:n_st] = out["U_path"][:, 0, :].T
        self.actuator_lookahead_cost = out["cost"]
        return X, U

    def get_actuator_lookahead_cost_statistics(self, X0s, n_samples, seed=0, mode="Nssu", ssu_num=1, cost_threshold=None, settle_tol=None):
        """get_actuator_lookahead_paths' flown flights reduced per start on the GPU
        (hjbdp.ControlLookaheadRollout.run_control_lookahead_campaign): the same streams, so the same costs, and nothing of length
        n * n_samples exists on the host or on the device.  The streams pair with get_actuator_cost_statistics /
        actuator_cost_map: with the same seed and n_samples the stored labels and the value function fly common random numbers.
        Returns get_noisy_cost_statistics' dict, one entry per start."""
        if int(n_samples) < 1:
            raise ValueError("n_samples must be at least 1")
        opening = self._actuator_lookahead_rollout("get_actuator_lookahead_cost_statistics")
        planes = self._stage_planes(mode, ssu_num, values=True)
        with opening as ro:
            return ro.run_control_lookahead_campaign(np.asarray(X0s, dtype=np.float64).reshape(self.S, -1), planes, int(n_samples),
                                                     seed=seed, first_stream=0, cost_threshold=cost_threshold, settle_tol=settle_tol)

    def actuator_lookahead_cost_map(self, n_samples, seed=0, mode="Nssu", ssu_num=1, cost_threshold=None, settle_tol=None):
        """get_actuator_lookahead_cost_statistics at every grid node: actuator_cost_map's starts on actuator_cost_map's streams -
        each entry [dx, dx] (stats [dx, dx, 8]), node (i, j) = (s_r[i], s_r[j]) flown from stream (i + dx * j) * n_samples on.
        With the same seed and n_samples this map's mean minus actuator_cost_map's is what the interpolated labels lose to the
        value function they came from under actuator noise, node by node, with the sampling noise largely cancelled; beside
        J_star's first plane it is "promised against paid" for the controller the design is exactly optimal for."""
        return self._grid_map(self.get_actuator_lookahead_cost_statistics(self._grid_starts(), n_samples, seed=seed, mode=mode,
                                                                          ssu_num=ssu_num, cost_threshold=cost_threshold,
                                                                          settle_tol=settle_tol))

    def get_greedy_paths(self, X0s, mode="Nssu", ssu_num=1):
        """The closed loop of the cost-to-go itself, on the GPU (hjbdp.Rollout.run_greedy): at every step the control of U_mesh
        that minimises x'Qx + R u^2 + J_{k+1}(A x + B u), J_{k+1} the plane of J_star behind the step blended linearly at the
        next state - one-step lookahead at the state actually visited, with no label table in between.  X0s [S, n].  Step k
        (0-based) reads plane k + 1 of J_star, whose last plane is the zero terminal; mode 'ssu' freezes plane ssu_num
        (1..N-1).  Returns X [S, N, n] and U [N, n] as get_optimal_paths does (U[N-1] = 0); leaves the closed-loop costs in
        self.greedy_cost [n] - beside self.paths_cost what the stored labels lose to the value function they came from - and
        the kernel's time in self.greedy_paths_ms.  The lookahead is NOMINAL even when self.disturbance is set: J_star then
        is the disturbed handle's cost-to-go, but the candidate's next state carries no node - get_lookahead_paths is the loop
        that looks ahead under self.disturbance."""
        opening = self._rollout("get_greedy_paths", values=True)
        N, S = self.N, self.S
        n_st = N - 1
        planes = self._stage_planes(mode, ssu_num, values=True)
        X0s = np.asarray(X0s, dtype=np.float64).reshape(S, -1)
        with opening as ro:
            out = ro.run_greedy(X0s, planes, keep_path=True)
        X = np.ascontiguousarray(out["X_path"].transpose(1, 2, 0))     # [n, S, N] -> [S, N, n]
        U = np.zeros((N, X0s.shape[1]))
        U[:n_st] = out["U_path"][:, 0, :].T
        self.greedy_cost = out["cost"]
        self.greedy_paths_ms = out["device_ms"]
        return X, U

    def get_lookahead_paths(self, X0s, n_samples=None, seed=0, mode="Nssu", ssu_num=1):
        """The closed loop of the DISTURBED cost-to-go, on the GPU (hjbdp.Rollout.run_lookahead): get_greedy_paths with
        self.disturbance's E_w (or max_w, in that set's own mode) inside every candidate - the control of U_mesh that minimises
        x'Qx + R u^2 + E_w J_{k+1}(A x + B u + d_w) at the state actually visited, the controller the disturbed solve is exactly
        optimal for.  Planes and `mode` / `ssu_num` as in get_greedy_paths.
        n_samples None: the nominal plant; returns X [S, N, n] and U [N, n] as get_greedy_paths does and leaves the costs in
        self.lookahead_cost [n].  n_samples given: every start flown n_samples times under the same nodes, sample j of start i
        on stream i * n_samples + j of `seed` (get_noisy_paths' numbering; a 'worst' set is sampled uniformly); returns the
        closed-loop costs [n, n_samples] and leaves their mean, standard deviation and maximum per start in
        self.lookahead_cost_mean / _std / _max [n].  The kernel's time: self.lookahead_paths_ms."""
        opening = self._rollout("get_lookahead_paths", values=True, lookahead="disturbed", noise=n_samples is not None)
        N, S = self.N, self.S
        n_st = N - 1
        planes = self._stage_planes(mode, ssu_num, values=True)
        if n_samples is not None and int(n_samples) < 1:
            raise ValueError("n_samples must be at least 1")
        X0s = np.asarray(X0s, dtype=np.float64).reshape(S, -1)
        n = X0s.shape[1]
        with opening as ro:
            if n_samples is None:
                out = ro.run_lookahead(X0s, planes, keep_path=True)
            else:
                out = ro.run_lookahead(np.repeat(X0s, int(n_samples), axis=1), planes, noisy=True, seed=seed, first_stream=0)
        self.lookahead_paths_ms = out["device_ms"]
        if n_samples is not None:
            cost = out["cost"].reshape(n, int(n_samples))
            self.lookahead_cost_mean, self.lookahead_cost_std, self.lookahead_cost_max = cost.mean(axis=1), cost.std(axis=1), cost.max(axis=1)
            return cost
        X = np.ascontiguousarray(out["X_path"].transpose(1, 2, 0))     # [n, S, N] -> [S, N, n]
        U = np.zeros((N, n))
        U[:n_st] = out["U_path"][:, 0, :].T
        self.lookahead_cost = out["cost"]
        return X, U

    def get_lookahead_cost_statistics(self, X0s, n_samples, seed=0, mode="Nssu", ssu_num=1, lookahead="disturbed", cost_threshold=None,
                                      settle_tol=None):
        """get_lookahead_paths' noisy flights reduced per start on the GPU (hjbdp.Rollout.run_lookahead_campaign): every start of
        X0s [S, n] flown n_samples times under self.disturbance's nodes by the one-step lookahead on J_star, sample j of start i
        on stream i * n_samples + j of `seed` (get_lookahead_paths' numbering: the same costs), and nothing of length
        n * n_samples exists on the host or on the device.  lookahead 'disturbed': the controller looks ahead under
        self.disturbance (get_lookahead_paths' controller); 'nominal': under one zero node (get_greedy_paths' controller).  In
        both self.disturbance is the plant.  The streams pair with get_noisy_cost_statistics / noisy_cost_map: with the same
        seed and n_samples, sample j of start i draws the same node at every step under the stored labels and under either
        lookahead (common random numbers), so the per-start means can be differenced with the sampling noise largely cancelled.
        Returns run_campaign's dict, one entry per start (get_noisy_cost_statistics').  Planes and `mode` / `ssu_num` as in
        get_lookahead_paths."""
        opening = self._rollout("get_lookahead_cost_statistics", values=True, lookahead=lookahead, noise=True)
        planes = self._stage_planes(mode, ssu_num, values=True)
        if int(n_samples) < 1:
            raise ValueError("n_samples must be at least 1")
        with opening as ro:
            return ro.run_lookahead_campaign(np.asarray(X0s, dtype=np.float64).reshape(self.S, -1), planes, int(n_samples), seed=seed,
                                             first_stream=0, cost_threshold=cost_threshold, settle_tol=settle_tol)

    def lookahead_cost_map(self, n_samples, seed=0, mode="Nssu", ssu_num=1, lookahead="disturbed", cost_threshold=None, settle_tol=None):
        """get_lookahead_cost_statistics at every grid node: each entry shaped like the grid, [dx, dx] (stats [dx, dx, 8]), node
        (i, j) = (s_r[i], s_r[j]) flown from stream (i + dx * j) * n_samples on - noisy_cost_map's starts on noisy_cost_map's
        streams.  The streams pair with noisy_cost_map: with the same seed and n_samples the two maps fly common random
        numbers, so this map's mean minus noisy_cost_map's is what the stored labels lose to the value function they came from,
        node by node, with the sampling noise largely cancelled.  Beside J_star's first plane it is "promised against paid"
        for the controller the disturbed solve is exactly optimal for."""
        return self._grid_map(self.get_lookahead_cost_statistics(self._grid_starts(), n_samples, seed=seed, mode=mode, ssu_num=ssu_num,
                                                                 lookahead=lookahead, cost_threshold=cost_threshold,
                                                                 settle_tol=settle_tol))

    @staticmethod
    def _two_pass_quantiles(campaign, n_samples, q, n_bins):
        """The two passes of the quantile methods.  campaign(hist) flies one campaign of the method's starts, seed and streams
        (hist None: the plain one).  Pass 1 is the plain campaign: every start's min and max.  Pass 2 flies the same samples
        again - the streams are counter-based - and bins them between lo = min and hi = nextafter(max, +inf) (hi = lo + 1 where
        min = max, or where a start's costs are not finite), so the range fits every start exactly: nothing under, nothing over.
        Returns pass 2's dict (its stats are pass 1's bits) plus quantiles [n, len(q)], clipped to [min, max], and q."""
        from .core import campaign_quantiles
        if int(n_samples) < 1:
            raise ValueError("n_samples must be at least 1")
        qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
        first = campaign(None)
        lo = np.array(first["min"], dtype=np.float64)
        hi = np.nextafter(np.array(first["max"], dtype=np.float64), np.inf)
        flat = ~(np.isfinite(lo) & np.isfinite(hi) & (lo < hi)) | (first["min"] == first["max"])
        lo = np.where(np.isfinite(lo), lo, 0.0)
        hi = np.where(flat, lo + 1.0, hi)
        out = campaign((lo, hi, int(n_bins)))
        out["device_ms"] = out["device_ms"] + first["device_ms"]
        out["quantiles"] = campaign_quantiles(out["hist"], out["hist_lo"], out["hist_hi"], qs, cmin=out["min"], cmax=out["max"])
        out["q"] = qs
        return out

    def get_noisy_cost_quantiles(self, X0s, n_samples, q=(0.5, 0.95, 0.99), n_bins=64, seed=0, mode="Nssu", ssu_num=1, method="linear",
                                 cost_threshold=None, settle_tol=None):
        """Quantiles of get_noisy_cost_statistics' costs per start, from histograms reduced on the GPU
        (hjbdp.Rollout.run_campaign with hist): two campaigns on the same seed and streams, the first for every start's min and
        max, the second binning the same samples in n_bins equal bins between them (_two_pass_quantiles), and nothing of length
        n * n_samples on the host or on the device.  Returns get_noisy_cost_statistics' dict plus hist [n, n_bins + 2], hist_lo,
        hist_hi, q and quantiles [n, len(q)]: hjbdp.campaign_quantiles' upper bounds, each at most one bin width (max - min) /
        n_bins above the order statistic of rank ceil(q * n_samples); q = 1 gives max exactly.  hjbdp.campaign_tail_mean of the
        same hist estimates the tail mean above a quantile."""
        opening = self._rollout("get_noisy_cost_quantiles", noise=True)
        planes = self._stage_planes(mode, ssu_num)
        X = np.asarray(X0s, dtype=np.float64).reshape(self.S, -1)
        with opening as ro:
            return self._two_pass_quantiles(lambda hist: ro.run_campaign(X, planes, int(n_samples), seed=seed, first_stream=0, method=method,
                                                                         cost_threshold=cost_threshold, settle_tol=settle_tol, hist=hist),
                                            n_samples, q, n_bins)

    def _grid_starts(self):
        """Every grid node as a start, [S, dx * dx]: node (i, j) is start i + dx * j"""
        s_r = np.asarray(self.s_r, dtype=np.float64)
        dx = s_r.size
        return np.stack([np.tile(s_r, dx), np.repeat(s_r, dx)])                 # axis 0 fastest, as the labels are stored

    def _grid_map(self, out):
        """A campaign's dict over _grid_starts' starts with every per-start array shaped like the grid, [dx, dx, ...]; q (the
        quantile levels) and the scalars stay, the pair's a and b dicts are shaped the same way."""
        dx = np.asarray(self.s_r).size
        return {key: (self._grid_map(v) if isinstance(v, dict) else
                      v.reshape((dx, dx) + v.shape[1:], order="F") if isinstance(v, np.ndarray) and key != "q" else v)
                for key, v in out.items()}

    def noisy_cost_quantile_map(self, n_samples, q=(0.5, 0.95, 0.99), n_bins=64, seed=0, mode="Nssu", ssu_num=1, method="linear",
                                cost_threshold=None, settle_tol=None):
        """get_noisy_cost_quantiles at every grid node, beside policy_cost(): each per-start entry shaped like the grid, [dx, dx]
        (quantiles [dx, dx, len(q)], hist [dx, dx, n_bins + 2]), node (i, j) = (s_r[i], s_r[j]) on noisy_cost_map's streams.
        Every node's bins lie between that node's own min and max: the cost spans orders of magnitude over the grid."""
        return self._grid_map(self.get_noisy_cost_quantiles(self._grid_starts(), n_samples, q=q, n_bins=n_bins, seed=seed, mode=mode,
                                                            ssu_num=ssu_num, method=method, cost_threshold=cost_threshold,
                                                            settle_tol=settle_tol))

    def get_lookahead_cost_quantiles(self, X0s, n_samples, q=(0.5, 0.95, 0.99), n_bins=64, seed=0, mode="Nssu", ssu_num=1,
                                     lookahead="disturbed", cost_threshold=None, settle_tol=None):
        """get_noisy_cost_quantiles for get_lookahead_cost_statistics' controller (hjbdp.Rollout.run_lookahead_campaign_hist): the
        same two passes on the same streams, so the quantiles of the stored labels and of either lookahead come from common
        random numbers.  `lookahead`, planes and `mode` / `ssu_num` as in get_lookahead_cost_statistics."""
        opening = self._rollout("get_lookahead_cost_quantiles", values=True, lookahead=lookahead, noise=True)
        planes = self._stage_planes(mode, ssu_num, values=True)
        X = np.asarray(X0s, dtype=np.float64).reshape(self.S, -1)
        with opening as ro:
            def campaign(hist):
                if hist is None:
                    return ro.run_lookahead_campaign(X, planes, int(n_samples), seed=seed, first_stream=0, cost_threshold=cost_threshold,
                                                     settle_tol=settle_tol)
                return ro.run_lookahead_campaign_hist(X, planes, int(n_samples), hist, seed=seed, first_stream=0,
                                                      cost_threshold=cost_threshold, settle_tol=settle_tol)
            return self._two_pass_quantiles(campaign, n_samples, q, n_bins)

    def lookahead_cost_quantile_map(self, n_samples, q=(0.5, 0.95, 0.99), n_bins=64, seed=0, mode="Nssu", ssu_num=1, lookahead="disturbed",
                                    cost_threshold=None, settle_tol=None):
        """get_lookahead_cost_quantiles at every grid node: noisy_cost_quantile_map's starts on its streams."""
        return self._grid_map(self.get_lookahead_cost_quantiles(self._grid_starts(), n_samples, q=q, n_bins=n_bins, seed=seed, mode=mode,
                                                                ssu_num=ssu_num, lookahead=lookahead, cost_threshold=cost_threshold,
                                                                settle_tol=settle_tol))

    _PAIR_CONTROLLERS = ("labels", "nominal", "disturbed")

    def get_paired_cost_statistics(self, X0s, n_samples, a="labels", b="disturbed", seed=0, mode="Nssu", ssu_num=1, method="linear",
                                   cost_threshold=None, settle_tol=None):
        """Two controllers flown on the same samples and their cost DIFFERENCE reduced per start on the GPU
        (hjbdp.Rollout.run_campaign_pair): every start of X0s [S, n] flown n_samples times under self.disturbance's nodes by
        controller a and by controller b, sample j of start i on stream i * n_samples + j of `seed` under both, and nothing of
        length n * n_samples on the host or on the device.  Controllers: 'labels' (get_noisy_cost_statistics' stored policy, read
        with `method`), 'disturbed' and 'nominal' (get_lookahead_cost_statistics' two lookaheads on J_star).  The planes, the
        streams and the start numbering are those methods', so the entries a and b of the result are their dicts, bit for bit.
        Returns run_campaign_pair's dict, one entry per start: a, b, stats_d [n, 8], mean_diff (b less a: negative where b paid
        less), var_diff, std_diff, se_diff, t, min_diff, max_diff, n_b_lower, n_a_lower, n_tie, n_both_in, mean_diff_both_in,
        device_ms - whether the stored labels lose to the value function they came from, with its standard error."""
        opening = self._rollout("get_paired_cost_statistics", values=True, lookahead="disturbed", noise=True)
        for name, ctl in (("a", a), ("b", b)):
            if ctl not in self._PAIR_CONTROLLERS:
                raise ValueError("%s must be one of %s" % (name, ", ".join(repr(c) for c in self._PAIR_CONTROLLERS)))
        label_planes, value_planes = self._stage_planes(mode, ssu_num), self._stage_planes(mode, ssu_num, values=True)
        if int(n_samples) < 1:
            raise ValueError("n_samples must be at least 1")
        side = {"labels": ("labels", label_planes, method), "nominal": ("greedy", value_planes), "disturbed": ("lookahead", value_planes)}
        with opening as ro:
            return ro.run_campaign_pair(np.asarray(X0s, dtype=np.float64).reshape(self.S, -1), side[a], side[b], int(n_samples), seed=seed,
                                        first_stream=0, cost_threshold=cost_threshold, settle_tol=settle_tol)

    def paired_cost_map(self, n_samples, a="labels", b="disturbed", seed=0, mode="Nssu", ssu_num=1, method="linear", cost_threshold=None,
                        settle_tol=None):
        """get_paired_cost_statistics at every grid node: each per-start entry shaped like the grid, [dx, dx] (stats_d [dx, dx, 8]; a
        and b dicts of such entries), node (i, j) = (s_r[i], s_r[j]) flown from stream (i + dx * j) * n_samples on - noisy_cost_map's
        and lookahead_cost_map's starts on their streams, so a and b equal those maps bit for bit and mean_diff is their means'
        difference WITH its standard error se_diff and the sign counts, node by node."""
        return self._grid_map(self.get_paired_cost_statistics(self._grid_starts(), n_samples, a=a, b=b, seed=seed, mode=mode,
                                                              ssu_num=ssu_num, method=method, cost_threshold=cost_threshold,
                                                              settle_tol=settle_tol))

    @staticmethod
    def compare_data(obj1, obj2):
        # Dynamic_Solver.m:266-280
        if obj1.J_star is None or obj2.J_star is None or obj1.J_star.size == 0 or obj2.J_star.size == 0:
            raise ValueError("stop throwing empty data at me")
        return bool(np.array_equal(obj1.J_star, obj2.J_star))
