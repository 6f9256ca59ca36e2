"""numpy restatement of the sensitivities of a step of a time-varying design in its initial deviation (include/almpc.h "Sensitivities
of a step of a time-varying design", csrc/almpc_sens_ltv.hip.h k_sens_ltv), twice:

  recursion  what the device computes: the Riccati recursion on the face where the inputs at a bound are held, with the stage models
             A_k, B_k.  Let p perturb the initial deviation (dx_0 = p in place of dx_0 = 0); all derivatives at p = 0.  Stages
             0-based, R, S, useR, useS as the design takes them, W_k the inputs of stage k at a bound, f the free:
               without the rate term (useS == 0)
                 P+ = sym(P) at k = N;  for k = N-1 .. 0:
                   Lam = R_ff + B_k,f' P+ B_k,f
                   K_k[f,:] = Lam^-1 B_k,f' P+ A_k,   K_k[W_k,:] = 0,   Acl_k = A_k - B_k K_k
                   P+ <- Qbar_k + Acl_k' P+ Acl_k + K_k' R K_k      (symmetrised; Qbar_k = Q for 1 <= k <= N-1)
                 Jacobians:  dx_0 = I,  du_k = -K_k dx_k,  dx_{k+1} = A_k dx_k + B_k du_k          (K0 = -K_0)
                 VJP:        lam_N = g_x[N],  lam_k = g_x[k] - K_k' g_u[k] + Acl_k' lam_{k+1},   g_x0 = lam_0
               with it: the recursion of tests/sens_face_rate_ref.py in the stage state z_k = [dx_k; du_{k-1}] with
                 At_k = [A_k 0; 0 0], Bt_k = [B_k; I], S_k = S for k >= 1 and S_0 = 0.
  direct     on the design's own QP (oracle/mpc_oracle.py::ltv_qp): with dx_0 = p the prediction is dX = Gam v + g + Phi p,
             Phi_k = A_{k-1} ... A_0, so the gradient of the QP gains F p with F = 2 Gam' Qbar Phi, and on the face
             dv_f/dp = -H_ff^-1 F_f, dv_W/dp = 0; dx by the rollout.  No recursion, no gain.

Conventions are those of tests/sens_ref.py: A (N, n, n), B (N, n, m); J = du/dp is (nz, n) stage-major (row k m + i), dX is
(n, N+1, n), a loss has gradients g_u (m, N) and g_x (n, N+1); sens_ref.shaped / vjp_from_jacobians apply to what comes out here.
"""
import numpy as np

from sens_face_ref import ACT_TOL, active_rows, distance_to_bounds   # noqa: F401  (the rule is k_sens_face's)


def branch(R, S):
    """(useR, useS) as the design takes them: R[1,1] != 0; and S given with S[1,1] != 0"""
    useR = np.asarray(R, float)[0, 0] != 0.0
    return bool(useR), bool(useR and S is not None and np.asarray(S, float)[0, 0] != 0.0)


def _sym(M):
    M = np.asarray(M, float)
    return 0.5 * (M + M.T)


def _held_solve(Lam, rhs, f):
    """K (m, w) with K[f] = Lam_ff^-1 rhs_f, zero on the held rows"""
    K = np.zeros_like(rhs)
    if f.any():
        c = np.linalg.cholesky(Lam[np.ix_(f, f)])
        K[f] = np.linalg.solve(c.T, np.linalg.solve(c, rhs[f]))
    return K


def face_gains(A, B, Q, R, S, P, act):
    """(K, Acl, w): the N gains (m, w) and closed-loop matrices (w, w) of the face whose held rows are `act` (nz,); w = n without the
    rate term, n + m with it."""
    N, n, m = B.shape
    useR, useS = branch(R, S)
    Q = _sym(Q)
    R = _sym(R) if useR else np.zeros((m, m))
    K, Acl = [None] * N, [None] * N
    if not useS:
        Pp = _sym(P)
        for k in range(N - 1, -1, -1):
            f = ~act[k * m:(k + 1) * m]
            Kk = np.zeros((m, n))
            if f.any():   # (on the free columns of B_k, as tests/sens_face_ref.py: the same operations in the same order)
                Bf = B[k][:, f]
                c = np.linalg.cholesky(R[np.ix_(f, f)] + Bf.T @ Pp @ Bf)
                Kk[f] = np.linalg.solve(c.T, np.linalg.solve(c, Bf.T @ Pp @ A[k]))
            Ak = A[k] - B[k] @ Kk
            K[k], Acl[k] = Kk, Ak
            if k > 0:
                Pp = _sym(Q + Ak.T @ Pp @ Ak + Kk.T @ R @ Kk)
        return K, Acl, n
    nt = n + m
    S = _sym(S)
    Pi = np.zeros((nt, nt)); Pi[:n, :n] = _sym(P)
    for k in range(N - 1, -1, -1):
        Sk = S if k >= 1 else np.zeros_like(S)
        At = np.zeros((nt, nt)); At[:n, :n] = A[k]
        Bt = np.vstack([B[k], np.eye(m)])
        Nt = np.vstack([np.zeros((n, m)), -Sk])
        Rt = R + Sk
        Qt = np.zeros((nt, nt))
        if k >= 1:
            Qt[:n, :n] = Q
        Qt[n:, n:] = Sk
        f = ~act[k * m:(k + 1) * m]
        Kk = _held_solve(Rt + Bt.T @ Pi @ Bt, Bt.T @ Pi @ At + Nt.T, f)
        Ak = At - Bt @ Kk
        K[k], Acl[k] = Kk, Ak
        if k > 0:
            Pi = _sym(Qt + Kk.T @ Rt @ Kk - Nt @ Kk - Kk.T @ Nt.T + Ak.T @ Pi @ Ak)
    return K, Acl, nt


def jacobians(A, B, Q, R, S, P, act):
    """(J, dX): du/dp (nz, n) and dx/dp (n, N+1, n)."""
    N, n, m = B.shape
    K, _, w = face_gains(A, B, Q, R, S, P, act)
    J = np.zeros((m * N, n))
    dX = np.zeros((n, N + 1, n))
    dz = np.vstack([np.eye(n), np.zeros((w - n, n))])
    dX[:, 0, :] = dz[:n]
    for k in range(N):
        du = -K[k] @ dz
        J[k * m:(k + 1) * m] = du
        dx = A[k] @ dz[:n] + B[k] @ du
        dz = np.vstack([dx, du]) if w > n else dx
        dX[:, k + 1, :] = dx
    return J, dX


def vjp(A, B, Q, R, S, P, act, g_u, g_x):
    """g_x0 (n,) = dL/dp for the loss gradients g_u (m, N), g_x (n, N+1): one backward sweep, no Jacobian."""
    N, n, m = B.shape
    K, Acl, w = face_gains(A, B, Q, R, S, P, act)
    z = np.zeros(w - n)
    lam = np.concatenate([g_x[:, N], z])
    for k in range(N - 1, -1, -1):
        lam = np.concatenate([g_x[:, k], z]) - K[k].T @ g_u[:, k] + Acl[k].T @ lam
    return lam[:n]


def rollout(A, B, J):
    """dX (n, N+1, n) from J = du/dp (nz, n) through the stage models: dx_0 = I, dx_{k+1} = A_k dx_k + B_k du_k."""
    N, n, m = B.shape
    dX = np.zeros((n, N + 1, n))
    dX[:, 0, :] = np.eye(n)
    for k in range(N):
        dX[:, k + 1, :] = A[k] @ dX[:, k, :] + B[k] @ J[k * m:(k + 1) * m]
    return dX


def jac_direct(A, B, Q, P, H, Gam, act):
    """(J, dX) of the direct form.  H and Gam are mo.ltv_qp's (return_prediction=True) for the same design."""
    N, n, m = B.shape
    Phi = np.zeros((n * N, n))
    row = np.eye(n)
    for k in range(N):
        row = A[k] @ row
        Phi[k * n:(k + 1) * n] = row
    Qbar = np.zeros((n * N, n * N))
    for k in range(N):
        Qbar[k * n:(k + 1) * n, k * n:(k + 1) * n] = _sym(P) if k == N - 1 else _sym(Q)
    F = 2.0 * Gam.T @ Qbar @ Phi
    J = np.zeros((m * N, n))
    fr = ~act
    if fr.any():
        J[fr] = -np.linalg.solve(H[np.ix_(fr, fr)], F[fr])
    return J, rollout(A, B, J)
