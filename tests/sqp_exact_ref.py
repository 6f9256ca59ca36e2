"""CPU restatement of the exact-Hessian mode of the Fnn SQP loop (almpc_sqp_fnn_set_hessian(h, ALMPC_SQP_HESSIAN_EXACT)), numpy only.

Stage Lagrangian Hessian of the Fnn layout y1 = W_in z, a_j = W_h[j] y_j + b_j, y_{j+1} = act(a_j), f = W_out y_{L+1}, z = [x; u]:
    W = d^2/dz^2 (lam' f) = sum_j M_j' diag(ybar_j * act''(a_j)) M_j,
M_j = d a_j / d z the forward Jacobian chain, ybar_j the adjoint of y_{j+1} = act(a_j) starting from W_out' lam.
Multipliers at the iterate: lam_N = 2 P e_N, lam_k = 2 Q e_k + A_k' lam_{k+1} (the adjoint walk of sqp_solve_ref); stage k's
dynamics x_{k+1} = f(z_k) carries lam_{k+1}.
Condensed exact QP: with M_k = [Gam_k; E_k] (the rows of dx_k = Gam_k v + g_k and the selector of v_k; Gam_0 = 0),
    H_ex = H_GN + sum_k M_k' W_k M_k,   q_ex = q_GN + sum_k M_k' W_k [g_k; 0].
Inertia rule: H_ex + delta diag(1_A), A the inputs on a bound at the iterate, delta the Gershgorin bound of H_ex
(max(0, max_i sum_{j != i} |H_ij| - H_ii)); if that is still not positive definite the instance takes a Gauss-Newton iteration."""
import numpy as np

import mpc_oracle as mo
import sqp_solve_ref as sref


def act2(act, a):
    """value, first and second derivative of the activation"""
    if act == "tanh":
        t = np.tanh(a)
        return t, 1.0 - t * t, -2.0 * t * (1.0 - t * t)
    if act in ("sigmoid", "swish"):
        s = 1.0 / (1.0 + np.exp(-a))
        if act == "sigmoid":
            return s, s * (1.0 - s), s * (1.0 - s) * (1.0 - 2.0 * s)
        return a * s, s * (1.0 + a * (1.0 - s)), s * (1.0 - s) * (2.0 + a * (1.0 - 2.0 * s))
    if act == "identity":
        return a, np.ones_like(a), np.zeros_like(a)
    if act == "relu":
        return np.maximum(a, 0.0), (a > 0).astype(np.float64), np.zeros_like(a)
    raise ValueError(act)


def stage_hessian(model, x, u, lam):
    """(n+m) x (n+m) Hessian of lam' f(x, u)."""
    y = model.W_in @ np.concatenate([x, u])
    J = model.W_in.copy()
    Ms, As = [], []
    for W, b in zip(model.W_h, model.b_h):
        a = W @ y + b
        M = W @ J
        y, d1, _ = act2(model.act, a)
        Ms.append(M); As.append(a)
        J = M * d1[:, None]
    yb = model.W_out.T @ lam
    Wz = np.zeros((J.shape[1], J.shape[1]))
    for j in range(len(Ms) - 1, -1, -1):
        _, d1, d2 = act2(model.act, As[j])
        Wz += Ms[j].T @ ((yb * d2)[:, None] * Ms[j])
        yb = model.W_h[j].T @ (yb * d1)
    return 0.5 * (Wz + Wz.T)


def multipliers(model, X, U, x_ref, P, Q):
    """lam_{k+1} of stage k, (n, N)"""
    n, N = X.shape[0], U.shape[1]
    L = np.zeros((n, N))
    lam = 2.0 * (0.5 * (P + P.T)) @ (X[:, N] - x_ref[:, N])
    for k in range(N - 1, -1, -1):
        L[:, k] = lam
        A, _ = model.jacobian(X[:, k], U[:, k])
        lam = A.T @ lam + (2.0 * (0.5 * (Q + Q.T)) @ (X[:, k] - x_ref[:, k]) if k > 0 else 0.0)
    return L


def exact_qp(model, X, U, A, B, c, x_ref, u_ref, Q, R, S, P, u_min, u_max):
    """(H_ex + shift, q_ex, lo, hi, H_GN, q_GN, delta)"""
    n, N = X.shape[0], U.shape[1]
    m = U.shape[0]
    nz = m * N
    H, q, lo, hi, Gam, g = mo.ltv_qp(A, B, c, X, U, x_ref, u_ref, Q, R, S, P, u_min, u_max, return_prediction=True)
    L = multipliers(model, X, U, x_ref, P, Q)
    He, qe = H.copy(), q.copy()
    for k in range(N):
        Wk = stage_hessian(model, X[:, k], U[:, k], L[:, k])
        Mk = np.zeros((n + m, nz))
        gk = np.zeros(n + m)
        if k > 0:
            Mk[:n] = Gam[(k - 1) * n:k * n]
            gk[:n] = g[(k - 1) * n:k * n]
        Mk[n:, k * m:(k + 1) * m] = np.eye(m)
        He += Mk.T @ Wk @ Mk
        qe += Mk.T @ Wk @ gk
    He = 0.5 * (He + He.T)
    delta = max(0.0, float(np.max(np.abs(He).sum(axis=1) - 2.0 * np.diag(He))))
    act = ((U <= u_min[:, None]) | (U >= u_max[:, None])).T.reshape(-1)
    Hs = He + np.diag(delta * act.astype(np.float64))
    return Hs, qe, lo, hi, H, q, delta


def sqp_solve_exact(model, x0, x_ref, u_ref, Q, R, S, P, u_min, u_max, max_iters, tol, adaptive=True):
    """sqp_solve_ref.sqp_solve with the exact-Hessian QP.  Extra key: gn_fallbacks (iterations an instance took with Gauss-Newton
    because the shifted exact Hessian was not positive definite)."""
    m, N = u_ref.shape
    U = np.clip(u_ref, u_min[:, None], u_max[:, None]).astype(np.float64)
    X = mo.fnn_rollout(model, x0, U)
    Rz = R if R[0, 0] != 0.0 else 0.0 * R
    Sz = S if (R[0, 0] != 0.0 and S[0, 0] != 0.0) else 0.0 * S
    mu = 2.0 * max(np.abs(P).max(), np.abs(Q).max())
    a, ref = 1.0, np.inf
    Xb = Ub = dXb = Vb = None
    fb = 0

    def merit(X, U, fv):
        EX, EU = X - x_ref, U - u_ref
        J = float(EX[:, N] @ P @ EX[:, N]) + sum(float(EX[:, k] @ Q @ EX[:, k] + EU[:, k] @ Rz @ EU[:, k]) for k in range(N))
        J += sum(float((U[:, k] - U[:, k + 1]) @ Sz @ (U[:, k] - U[:, k + 1])) for k in range(N - 1))
        return J + mu * float(np.abs(fv - X[:, 1:]).sum())

    it = 0
    while True:
        r, dmax, _ = sref.adjoint_residual(model, X, U, x_ref, u_ref, Q, R, S, P, u_min, u_max)
        if dmax <= sref.DEFECT_TOL and r <= tol:
            return dict(status=0, iters=it, kkt=r, X=X, U=U, gn_fallbacks=fb)
        if it == max_iters:
            return dict(status=1, iters=it, kkt=r, X=X, U=U, gn_fallbacks=fb)
        it += 1
        fv = np.stack([model.forward(X[:, k], U[:, k]) for k in range(N)], axis=1)
        if adaptive:
            phi = merit(X, U, fv)
            if (phi <= ref + 1e-12 * abs(ref) + 1e-300) or a <= 1.0 / 64.0:
                ref, a = phi, min(1.0, 2.0 * a)
            else:
                a *= 0.5
                X = Xb + a * dXb
                U = np.clip(Ub + a * Vb, u_min[:, None], u_max[:, None])
                continue
        A, B, c = [], [], []
        for k in range(N):
            Ak, Bk = model.jacobian(X[:, k], U[:, k])
            A.append(Ak); B.append(Bk); c.append(fv[:, k] - X[:, k + 1])
        He, qe, lo, hi, H, q, _ = exact_qp(model, X, U, A, B, c, x_ref, u_ref, Q, Rz, Sz, P, u_min, u_max)
        try:
            np.linalg.cholesky(He)
        except np.linalg.LinAlgError:
            He, qe = H, q
            fb += 1
        v = mo.solve_box_qp_exact(He, qe, lo, hi).reshape(N, m).T
        dX = np.zeros_like(X)
        dx = np.zeros(x0.size)
        for k in range(N):
            dx = A[k] @ dx + B[k] @ v[:, k] + c[k]
            dX[:, k + 1] = dx
        if adaptive:
            Xb, Ub, dXb, Vb = X.copy(), U.copy(), dX, v
        sc = a if adaptive else 1.0
        X, U = X + sc * dX, np.clip(U + sc * v, u_min[:, None], u_max[:, None])
