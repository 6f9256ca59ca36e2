"""numpy restatement of the sensitivities on structured handles whose design carries the input-rate weight S (include/almpc.h "The
same with the input-rate weight S", csrc/almpc_sens.hip.h k_sens_face_rate): the Riccati recursion on the face in the augmented stage
state z_k = [dx_k; du_{k-1}], nt = n + m.

Stages 0-based; R as the design uses it; S_k = S for k >= 1 and S_0 = 0 (the rate sum runs over u_k - u_{k+1}, k = 0 .. N-2: nothing
ties u_0 to an input applied before the horizon); W_k the inputs of stage k at a bound, f the free:

    At = [A 0; 0 0] (nt x nt)    Bt = [B; I] (nt x m)    Nt_k = [0; -S_k] (nt x m)    Rt_k = R + S_k
    Qt_k = blkdiag(Qbar_k, S_k),  Qbar_k = Q (1 <= k <= N-1),  Qbar_0 = 0
    Pi+ = blkdiag(sym(P), 0) at k = N;  for k = N-1 .. 0:
      Lam = (Rt_k + Bt' Pi+ Bt)_ff
      K_k[f,:] = Lam^-1 (Bt' Pi+ At + Nt_k')_f,   K_k[W_k,:] = 0   (m x nt),   Acl_k = At - Bt K_k
      Pi+ <- Qt_k + K_k' Rt_k K_k - Nt_k K_k - K_k' Nt_k' + Acl_k' Pi+ Acl_k            (symmetrised)
    Jacobians:  dz_0 = [I_n; 0],  du_k = -K_k dz_k,  dz_{k+1} = At dz_k + Bt du_k      (K0 = -K_0[:, :n])
    VJP:        lam_N = [g_x[N]; 0],  lam_k = [g_x[k]; 0] - K_k' g_u[k] + Acl_k' lam_{k+1},   g_x0 = lam_0[:n]

With S = 0 the w columns of every K_k and the w blocks of Pi+ vanish and the recursion is that of tests/sens_face_ref.py.

Conventions are those of tests/sens_face_ref.py (and tests/sens_ref.py): J = du/dx0 is (nz, n) stage-major, dX is (n, N+1, n), a loss
has gradients g_u (m, N) and g_x (n, N+1).
"""
import numpy as np

from sens_face_ref import ACT_TOL, active_rows, design_R, distance_to_bounds   # noqa: F401  (the rule is the same)


def design_S(R, S):
    """S as the design uses it: the reference drops the rate term together with R, and when S[1,1] == 0."""
    R, S = np.asarray(R, float), np.asarray(S, float)
    return S if (R[0, 0] != 0.0 and S[0, 0] != 0.0) else np.zeros_like(S)


def face_gains(A, B, Q, R, S, P, act, N):
    """(K, Acl): the N gains (m, nt) and closed-loop matrices (nt, nt) of the face whose held rows are `act` (nz,)."""
    n, m = B.shape
    nt = n + m
    S = design_S(R, S)
    R = design_R(R)
    At = np.zeros((nt, nt)); At[:n, :n] = A
    Bt = np.vstack([B, np.eye(m)])
    Pi = np.zeros((nt, nt)); Pi[:n, :n] = 0.5 * (P + P.T)
    K, Acl = [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        Sk = S if k >= 1 else np.zeros_like(S)
        Nt = np.vstack([np.zeros((n, m)), -Sk])
        Rt = R + Sk
        Qt = np.zeros((nt, nt))
        if k >= 1:
            Qt[:n, :n] = Q
        Qt[n:, n:] = Sk
        f = ~act[k * m:(k + 1) * m]
        Kk = np.zeros((m, nt))
        if f.any():
            c = np.linalg.cholesky((Rt + Bt.T @ Pi @ Bt)[np.ix_(f, f)])
            Kk[f] = np.linalg.solve(c.T, np.linalg.solve(c, (Bt.T @ Pi @ At + Nt.T)[f]))
        Ak = At - Bt @ Kk
        K[k], Acl[k] = Kk, Ak
        if k > 0:
            Pi = Qt + Kk.T @ Rt @ Kk - Nt @ Kk - Kk.T @ Nt.T + Ak.T @ Pi @ Ak
            Pi = 0.5 * (Pi + Pi.T)
    return K, Acl


def jacobians(A, B, Q, R, S, P, act, N):
    """(J, dX): du/dx0 (nz, n) and dx/dx0 (n, N+1, n)."""
    n, m = B.shape
    K, _ = face_gains(A, B, Q, R, S, P, act, N)
    J = np.zeros((m * N, n))
    dX = np.zeros((n, N + 1, n))
    dz = np.vstack([np.eye(n), np.zeros((m, n))])
    dX[:, 0, :] = dz[:n]
    for k in range(N):
        du = -K[k] @ dz
        J[k * m:(k + 1) * m] = du
        dz = np.vstack([A @ dz[:n] + B @ du, du])
        dX[:, k + 1, :] = dz[:n]
    return J, dX


def vjp(A, B, Q, R, S, P, act, g_u, g_x):
    """g_x0 (n,) = dL/dx0 for the loss gradients g_u (m, N), g_x (n, N+1): one backward sweep, no Jacobian."""
    n, m = B.shape
    N = g_u.shape[1]
    K, Acl = face_gains(A, B, Q, R, S, P, act, N)
    z = np.zeros(m)
    lam = np.concatenate([g_x[:, N], z])
    for k in range(N - 1, -1, -1):
        lam = np.concatenate([g_x[:, k], z]) - K[k].T @ g_u[:, k] + Acl[k].T @ lam
    return lam[:n]
