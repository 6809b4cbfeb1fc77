"""Plain numpy restatement of hjb_attitude_linear_response (include/hjbdp.h, csrc/kernels_rollout_attitude_linear.h), the checker of
tests/test_gpu_rollout_attitude_linear.py, vectorised over trajectories, one IEEE float64 operation at a time:
  qe_i = ((qc[i,0]*X4 + qc[i,1]*X5) + qc[i,2]*X6) + qc[i,3]*X7, i = 0, 1, 2;
  u_i = (-((K[i,0]*qe_0 + K[i,1]*qe_1) + K[i,2]*qe_2)) - ((C[i,0]*X1 + C[i,1]*X2) + C[i,2]*X3);
  with a limit L: u_i = L_i where u_i > L_i, -L_i where u_i < -L_i, u_i otherwise (so a NaN stays);
  angles: attitude_rollout_refs.angles;
  cost 'quat': ((w0*(X1*X1) + w1*(X2*X2)) + ... + w6*(X7*X7)) + w7*(u1*u1) + w8*(u2*u2) + w9*(u3*u3), the sum of
               attitude_rollout_refs.rollout;
  cost 'angle': t_i = 2 * asinc(clamp(X[3+i], -1, 1)); g_i = (w_i*(X_i*X_i) + w_(3+i)*(t_i*t_i)) + w_(6+i)*(u_i*u_i);
                (g_0 + g_1) + g_2, the sum of attitude_simplified_rollout_refs.rollout;
  step: attitude_rollout_refs.step (taylor or RK4 with u held, then q / |q|).
Nothing here comes from the package.
"""
from __future__ import annotations

import numpy as np

from attitude_rollout_refs import angles, asinc, step


def control(X, K, C, qc=None, u_limit=None):
    """U [3, n] of X [7, n]."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    C = np.asarray(C, dtype=np.float64).reshape(3, 3)
    qc = np.eye(4) if qc is None else np.asarray(qc, dtype=np.float64).reshape(4, 4)
    qe = [((qc[i, 0] * X[3] + qc[i, 1] * X[4]) + qc[i, 2] * X[5]) + qc[i, 3] * X[6] for i in range(3)]
    u = np.stack([(-((K[i, 0] * qe[0] + K[i, 1] * qe[1]) + K[i, 2] * qe[2])) - ((C[i, 0] * X[0] + C[i, 1] * X[1]) + C[i, 2] * X[2])
                  for i in range(3)])
    if u_limit is not None:
        L = np.asarray(u_limit, dtype=np.float64).reshape(3, 1)
        u = np.where(u > L, L, np.where(u < -L, -L, u))
    return u


def rollout(inertia, h, integrator, K, C, X0, n_steps, qc=None, u_limit=None, cost_form="quat", weights=None):
    """inertia (J1, J2, J3); integrator 'taylor' or 'RK4'; K, C [3, 3]; qc [4, 4]; u_limit [3]; weights [10]; X0 [7, n].
    Returns X_final [7, n], cost [n], X_path [n, 7, N+1], U_path [n, 3, N], A_path [n, 3, N]."""
    assert cost_form in ("quat", "angle")
    w = np.zeros(10) if weights is None else np.asarray(weights, dtype=np.float64).reshape(10)
    x = np.array(np.asarray(X0, dtype=np.float64).reshape(7, -1))
    n = x.shape[1]
    N = int(n_steps)
    X_path = np.zeros((n, 7, N + 1))
    U_path = np.zeros((n, 3, N))
    A_path = np.zeros((n, 3, N))
    cost = np.zeros(n)
    X_path[:, :, 0] = x.T
    with np.errstate(all="ignore"):
        for k in range(N):
            u = control(x, K, C, qc, u_limit)
            yaw, pitch, roll = angles(x)
            if cost_form == "quat":
                g = w[0] * (x[0] * x[0])
                for a in range(1, 7):
                    g = g + w[a] * (x[a] * x[a])
                for j in range(3):
                    g = g + w[7 + j] * (u[j] * u[j])
                cost = cost + g
            else:
                s = x[3:6]
                th = 2.0 * asinc(np.where(s > 1.0, 1.0, np.where(s < -1.0, -1.0, s)))
                g = [(w[j] * (x[j] * x[j]) + w[3 + j] * (th[j] * th[j])) + w[6 + j] * (u[j] * u[j]) for j in range(3)]
                cost = cost + ((g[0] + g[1]) + g[2])
            A_path[:, :, k] = np.stack([yaw, pitch, roll], axis=1)
            U_path[:, :, k] = u.T
            x = step(x, u, inertia, h, integrator)
            X_path[:, :, k + 1] = x.T
    return x, cost, X_path, U_path, A_path
