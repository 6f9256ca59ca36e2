"""numpy restatement of the sensitivities on structured handles (include/almpc.h "The same on ALMPC_FLAG_STRUCTURED handles",
csrc/almpc_sens.hip.h k_sens_face): the Riccati recursion on the face where the inputs at a bound are held.

Stages 0-based: x_0 = x0, Qbar_k = Q for 1 <= k <= N-1, Qbar_0 = 0, P on stage N; W_k the inputs of stage k at a bound, f the free:

    P+ = P at k = N;  for k = N-1 .. 0:
      Lam = R_ff + B_f' P+ B_f                 (R as the design uses it: zero when R[1,1] == 0)
      K_k[f,:] = Lam^-1 B_f' P+ A,   K_k[W_k,:] = 0,   Acl_k = A - B K_k
      P+ <- Qbar_k + Acl_k' P+ Acl_k + K_k' R K_k            (symmetrised)
    Jacobians:  dx_0 = I,  du_k = -K_k dx_k,  dx_{k+1} = A dx_k + B du_k          (K0 = -K_0)
    VJP:        lam_N = g_x[N],  lam_k = g_x[k] - K_k' g_u[k] + Acl_k' lam_{k+1},   g_x0 = lam_0

Conventions are those of tests/sens_ref.py: J = du/dx0 is (nz, n) stage-major (row k m + i), dX is (n, N+1, n), a loss has gradients
g_u (m, N) and g_x (n, N+1); sens_ref.shaped / dx_from_du / vjp_from_jacobians apply to what comes out here.
"""
import numpy as np

ACT_TOL = 1e-7   # almpc_sensitivity_stagewise's default (act_tol <= 0): ten times what k_sdual's confirmation leaves a row off its bound


def active_rows(u, u_min, u_max, tau=ACT_TOL):
    """The contract's rule on the returned inputs u (m, N): row (k, i) is active iff u - umin <= tau w_i or umax - u <= tau w_i,
    w = umax - umin.  Returns the mask (nz,) stage-major."""
    lo, hi = np.asarray(u_min, float)[:, None], np.asarray(u_max, float)[:, None]
    w = hi - lo
    return ((u - lo <= tau * w) | (hi - u <= tau * w)).T.reshape(-1)


def distance_to_bounds(u, u_min, u_max):
    """(m, N): the distance of every input to its nearer bound, in units of the width of its box."""
    lo, hi = np.asarray(u_min, float)[:, None], np.asarray(u_max, float)[:, None]
    return np.minimum(u - lo, hi - u) / (hi - lo)


def design_R(R):
    """R as the design uses it: dropped when R[1,1] == 0 (the reference's branch rule)."""
    R = np.asarray(R, float)
    return R if R[0, 0] != 0.0 else np.zeros_like(R)


def face_gains(A, B, Q, R, P, act, N):
    """(K, Acl): the N gains (m, n) and closed-loop matrices (n, n) of the face whose held rows are `act` (nz,)."""
    n, m = B.shape
    R = design_R(R)
    Pp = 0.5 * (P + P.T)
    K, Acl = [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        f = ~act[k * m:(k + 1) * m]
        Kk = np.zeros((m, n))
        if f.any():
            Bf = B[:, f]
            c = np.linalg.cholesky(R[np.ix_(f, f)] + Bf.T @ Pp @ Bf)
            Kk[f] = np.linalg.solve(c.T, np.linalg.solve(c, Bf.T @ Pp @ A))
        Ak = A - B @ Kk
        K[k], Acl[k] = Kk, Ak
        if k > 0:
            Pp = Q + Ak.T @ Pp @ Ak + Kk.T @ R @ Kk
            Pp = 0.5 * (Pp + Pp.T)
    return K, Acl


def jacobians(A, B, Q, R, P, act, N):
    """(J, dX): du/dx0 (nz, n) and dx/dx0 (n, N+1, n)."""
    n, m = B.shape
    K, _ = face_gains(A, B, Q, R, P, act, N)
    J = np.zeros((m * N, n))
    dX = np.zeros((n, N + 1, n))
    dx = np.eye(n)
    dX[:, 0, :] = dx
    for k in range(N):
        du = -K[k] @ dx
        J[k * m:(k + 1) * m] = du
        dx = A @ dx + B @ du
        dX[:, k + 1, :] = dx
    return J, dX


def vjp(A, B, Q, R, P, act, g_u, g_x):
    """g_x0 (n,) = dL/dx0 for the loss gradients g_u (m, N), g_x (n, N+1): one backward sweep, no Jacobian."""
    N = g_u.shape[1]
    K, Acl = face_gains(A, B, Q, R, P, act, N)
    lam = g_x[:, N].copy()
    for k in range(N - 1, -1, -1):
        lam = g_x[:, k] - K[k].T @ g_u[:, k] + Acl[k].T @ lam
    return lam
