"""numpy restatement of the solution sensitivities (include/almpc.h "Sensitivities", csrc/almpc_sens.hip.h), twice:

  direct   on the face where the rows W of the solution sit at their bounds the free rows solve H_FF v_F = -f_F - H_FW b_W, so
           dv_F/dx0 = -H_FF^-1 F_F and dv_W/dx0 = 0 (unscaled H, F: no scaling, no inverse of H);
  G form   what the device computes: H' = DHD, G = H'^-1, V = -G F', S = G[W,W], dw/dx0 = V - G[:,W] S^-1 V[W,:], dv/dx0 = D dw/dx0.

Conventions: v = vec(e_u) stage-major (row j = k m + i), J = dv/dx0 = du/dx0 is nz x n; dX is (n, N+1, n) with
dX[:, k, :] = dx[:,k]/dx0; the Julia-shaped arrays of the bindings are K0 (m, n), dU (m, N, n), dX (n, N+1, n), each
[i, k, c] = d(entry i of stage k) / d x0[c].  A loss has gradients g_u (m, N) and g_x (n, N+1).
"""
import numpy as np

ACT_TOL = 1e-9   # almpc_sensitivity's default (act_tol <= 0)


def active_rows(u, u_min, u_max, d, tau=ACT_TOL):
    """The contract's rule on the returned inputs u (m, N): row (k, i) is active iff u - umin <= tau d_j or umax - u <= tau d_j."""
    m, N = u.shape
    uf = u.T.reshape(-1)
    lo, hi = np.tile(np.asarray(u_min, float), N), np.tile(np.asarray(u_max, float), N)
    return (uf - lo <= tau * d) | (hi - uf <= tau * d)


def jac_direct(H, F, act):
    nz, n = F.shape
    J = np.zeros((nz, n))
    fr = ~act
    if fr.any():
        J[fr] = -np.linalg.solve(H[np.ix_(fr, fr)], F[fr])
    return J


def g_operands(H, F, d):
    Hs = H * d[:, None] * d[None, :]
    c = np.linalg.cholesky(Hs)
    G = np.linalg.solve(c.T, np.linalg.solve(c, np.eye(H.shape[0])))
    G = 0.5 * (G + G.T)
    # V = -H'^-1 F' by the factor, not as the product -G F': the product carries G's rounding (cond(H') ~ 6.5e6 times the FP64 unit)
    # into every entry of V, and a VJP, whose two terms cancel, then misses 1e-9 of its own size (1.6e-9 measured against 8.6e-11)
    return G, -np.linalg.solve(c.T, np.linalg.solve(c, F * d[:, None]))


def jac_gform(H, F, d, act, ops=None):
    """ops: g_operands(H, F, d) computed once for a shared design."""
    G, V = ops if ops is not None else g_operands(H, F, d)
    W = np.nonzero(act)[0]
    Jw = V.copy()
    if W.size:
        Jw = V - G[:, W] @ np.linalg.solve(G[np.ix_(W, W)], V[W])
        Jw[W] = 0.0
    return d[:, None] * Jw


def dx_from_du(A, B, J, N):
    """dX (n, N+1, n) from J = du/dx0 (nz, n): dx_1 = I, dx_{k+1} = A dx_k + B du_k."""
    n, m = B.shape
    dX = np.zeros((n, N + 1, n))
    dX[:, 0, :] = np.eye(n)
    for k in range(N):
        dX[:, k + 1, :] = A @ dX[:, k, :] + B @ J[k * m:(k + 1) * m]
    return dX


def shaped(J, m, N):
    """(K0, dU) Julia-shaped from J (nz, n)."""
    dU = J.reshape(N, m, -1).transpose(1, 0, 2)
    return dU[:, 0, :], dU


def adjoint(A, B, g_u, g_x):
    """lam_1 and q = g_u + [B'lam_2; ...; B'lam_{N+1}] (nz, stage-major) of the adjoint rollout."""
    n, m = B.shape
    N = g_u.shape[1]
    lam = g_x[:, N].copy()
    q = np.zeros(m * N)
    for k in range(N - 1, -1, -1):
        q[k * m:(k + 1) * m] = g_u[:, k] + B.T @ lam
        lam = A.T @ lam + g_x[:, k]
    return lam, q


def vjp_direct(H, F, act, A, B, g_u, g_x):
    lam1, q = adjoint(A, B, g_u, g_x)
    return lam1 + jac_direct(H, F, act).T @ q


def vjp_gform(H, F, d, act, A, B, g_u, g_x, ops=None):
    lam1, q = adjoint(A, B, g_u, g_x)
    G, V = ops if ops is not None else g_operands(H, F, d)
    W = np.nonzero(act)[0]
    p = d * q
    p[W] = 0.0
    out = lam1 + V.T @ p
    if W.size:
        out = out - V[W].T @ np.linalg.solve(G[np.ix_(W, W)], G[W] @ p)
    return out


def vjp_scale(g_x0):
    """What a VJP error is measured against: max(1, max|g_x0_i|) of the instance's reference result, as max(1, max|J_i|) for a
    Jacobian.  (g_x0 = lam_1 + J'q is a sum of two terms that cancel -- 200 against a sum of 20 on the quadrotor with unit-normal loss
    gradients --, so this asks more of the evaluation than the size of its terms would.)"""
    return max(1.0, float(np.abs(g_x0).max()))


def vjp_from_jacobians(dU, dX, g_u, g_x):
    """dU' g_u + dX' g_x from Julia-shaped Jacobians (m, N, n), (n, N+1, n)."""
    return np.einsum("ikc,ik->c", dU, g_u) + np.einsum("ikc,ik->c", dX, g_x)
