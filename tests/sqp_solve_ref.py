"""CPU restatement of almpc_sqp_fnn_solve: the Gauss-Newton SQP loop of mpc_oracle.sqp_fnn with the first-order stopping test
evaluated at the top of every iteration, at the multiple-shooting iterate (numpy only; imported by the tests beside it).

Stopping test of an instance, at its iterate (X, U):  max |f(x_k, u_k) - x_{k+1}| <= DEFECT_TOL  and
    |U - clip(U - G / (2 R_aa))|_inf <= tol,
G the adjoint gradient of the cost at the iterate: lam_N = 2 P e_N, G_k = 2 R eu_k + B_k' lam_{k+1} (+ the input-rate terms),
lam_k = 2 Q e_k + A_k' lam_{k+1}, with (A_k, B_k) the network's Jacobians at (x_k, u_k).  With zero defects this is
mpc_oracle.nlp_kkt_residual."""
import numpy as np

import mpc_oracle as mo

DEFECT_TOL = 1e-10


def adjoint_residual(model, X, U, x_ref, u_ref, Q, R, S, P, u_min, u_max):
    """(projected residual, max |defect|, G) at the multiple-shooting iterate (X (n, N+1), U (m, N))."""
    n, N = X.shape[0], U.shape[1]
    useS = S[0, 0] != 0.0
    Qs, Rs, Ss, Ps = 0.5 * (Q + Q.T), 0.5 * (R + R.T), 0.5 * (S + S.T), 0.5 * (P + P.T)
    EX, EU = X - x_ref, U - u_ref
    fv = np.stack([model.forward(X[:, k], U[:, k]) for k in range(N)], axis=1)
    defect = float(np.abs(fv - X[:, 1:]).max())
    G = np.zeros_like(U)
    lam = 2.0 * Ps @ EX[:, N]
    for k in range(N - 1, -1, -1):
        A, B = model.jacobian(X[:, k], U[:, k])
        G[:, k] = 2.0 * Rs @ EU[:, k] + B.T @ lam
        lam = A.T @ lam + (2.0 * Qs @ EX[:, k] if k > 0 else 0.0)
    if useS:
        for k in range(N - 1):
            du = 2.0 * Ss @ (U[:, k] - U[:, k + 1])
            G[:, k] += du
            G[:, k + 1] -= du
    sc = 1.0 / np.maximum(2.0 * np.diag(Rs), 1e-12)
    T = np.clip(U - sc[:, None] * G, u_min[:, None], u_max[:, None])
    return float(np.abs(U - T).max()), defect, G


def sqp_solve(model, x0, x_ref, u_ref, Q, R, S, P, u_min, u_max, max_iters, tol, adaptive=True, u_guess=None):
    """The loop of mpc_oracle.sqp_fnn (condensed QP, exact box-QP solves, optional merit rule), stopped per instance.
    Returns dict(status 0 converged / 1 iteration limit, iters = QP iterations taken, kkt = residual at the last test, X, U)."""
    m, N = u_ref.shape
    U = np.clip(u_ref if u_guess is None else u_guess, u_min[:, None], u_max[:, None]).astype(np.float64)
    X = mo.fnn_rollout(model, x0, U)
    Rz = R if R[0, 0] != 0.0 else 0.0 * R
    Sz = S if (R[0, 0] != 0.0 and S[0, 0] != 0.0) else 0.0 * S
    mu = 2.0 * max(np.abs(P).max(), np.abs(Q).max())
    a, ref = 1.0, np.inf
    Xb = Ub = dXb = Vb = None

    def merit(X, U, fv):
        EX, EU = X - x_ref, U - u_ref
        J = float(EX[:, N] @ P @ EX[:, N]) + sum(float(EX[:, k] @ Q @ EX[:, k] + EU[:, k] @ Rz @ EU[:, k]) for k in range(N))
        J += sum(float((U[:, k] - U[:, k + 1]) @ Sz @ (U[:, k] - U[:, k + 1])) for k in range(N - 1))
        return J + mu * float(np.abs(fv - X[:, 1:]).sum())

    it = 0
    while True:
        r, dmax, _ = adjoint_residual(model, X, U, x_ref, u_ref, Q, R, S, P, u_min, u_max)
        if dmax <= DEFECT_TOL and r <= tol:
            return dict(status=0, iters=it, kkt=r, X=X, U=U)
        if it == max_iters:
            return dict(status=1, iters=it, kkt=r, X=X, U=U)
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
        H, q, lo, hi = mo.ltv_qp(A, B, c, X, U, x_ref, u_ref, Q, Rz, Sz, P, u_min, u_max)
        v = mo.solve_box_qp_exact(H, q, lo, hi).reshape(N, m).T
        dX = np.zeros_like(X)
        dx = np.zeros(x0.size)
        for k in range(N):
            dx = A[k] @ dx + B[k] @ v[:, k] + c[k]
            dX[:, k + 1] = dx
        if adaptive:
            Xb, Ub, dXb, Vb = X.copy(), U.copy(), dX, v
        sc = a if adaptive else 1.0
        X, U = X + sc * dX, np.clip(U + sc * v, u_min[:, None], u_max[:, None])


def bench_setup(b=256, N=50, act="tanh", amp=0.6):
    """The benchmark batch of tests/test_gpu_sqp.py::_setup (Fnn 4-2-16x2, N 50): model, problem data, initial states."""
    f = mo.synthetic_fnn(act=act)
    n, m = 4, 2
    x_ref = np.tile(np.array([0.2, -0.1, 0.05, 0.0])[:, None], (1, N + 1))
    u_ref = np.tile(np.array([0.1, -0.2])[:, None], (1, N))
    X0 = x_ref[:, 0][None, :] + amp * mo.splitmix_normal(0x5EED0005, 0, b, n)
    kw = dict(x_ref=x_ref, u_ref=u_ref, Q=100.0 * np.eye(n), R=0.1 * np.eye(m), S=np.zeros((m, m)), P=150.0 * np.eye(n),
              u_min=-np.ones(m), u_max=np.ones(m))
    return f, kw, X0
