"""CPU restatement of the Fnn SQP loop with STATE ROWS in its stopping test and exact Hessian (almpc_sqp_fnn_set_row_multipliers),
numpy only (the certificate uses scipy.optimize.lsq_linear); imported by the tests beside it.

Every iteration's QP carries the state box / terminal equality as rows of dX = Gam v + g (mpc_oracle.ltv_state_rows) and is solved by
mpc_oracle.solve_qp_dual_active_set in the Jacobi-scaled variables; the multipliers of its state rows, lam[nz:], are mu: mu[i, k] belongs
to the row of x_{k+1}[i], > 0 on an upper bound, < 0 on a lower bound, free on a terminal-equality row, 0 outside the working set, in the
units of the gradient of the cost (the rows themselves are not scaled).  They enter the adjoint walk,
    lam_N = 2 P e_N + mu_N,   G_k = 2 R eu_k + B_k' lam_{k+1},   lam_k = 2 Q e_k + A_k' lam_{k+1} + mu_k,
and the residual of the stopping test is the maximum of
    the projected residual |U - clip(U - G / (2 R_aa))|_inf with that adjoint,
    the complementarity |x - bound| over the box rows with mu != 0 (side by sign),
    the primal violation of the box, and |x_{N+1} - x_ref| under the terminal equality (whose rows replace the box rows of that stage).
The same lam are the multipliers of the exact Lagrangian Hessian (sqp_exact_ref.stage_hessian): state rows are linear, no curvature of
their own."""
import numpy as np

import mpc_oracle as mo
import sqp_exact_ref as xr
import sqp_solve_ref as sref

DEFECT_TOL = sref.DEFECT_TOL


def adjoint_residual_rows(model, X, U, x_ref, u_ref, Q, R, S, P, u_min, u_max, mu, x_min=None, x_max=None, terminal="none"):
    """(residual, max |defect|, G, (projected, complementarity, primal)) at the iterate (X (n, N+1), U (m, N)) with the row multipliers
    mu (n, N).  With mu = 0 and no rows this is sqp_solve_ref.adjoint_residual bit for bit."""
    n, N = X.shape[0], U.shape[1]
    useS = S[0, 0] != 0.0
    Qs, Rs, Ss, Ps = 0.5 * (Q + Q.T), 0.5 * (R + R.T), 0.5 * (S + S.T), 0.5 * (P + P.T)
    EX, EU = X - x_ref, U - u_ref
    fv = np.stack([model.forward(X[:, k], U[:, k]) for k in range(N)], axis=1)
    defect = float(np.abs(fv - X[:, 1:]).max())
    G = np.zeros_like(U)
    lam = 2.0 * Ps @ EX[:, N] + mu[:, N - 1]
    for k in range(N - 1, -1, -1):
        A, B = model.jacobian(X[:, k], U[:, k])
        G[:, k] = 2.0 * Rs @ EU[:, k] + B.T @ lam
        lam = A.T @ lam + (2.0 * Qs @ EX[:, k] + mu[:, k - 1] if k > 0 else 0.0)
    if useS:
        for k in range(N - 1):
            du = 2.0 * Ss @ (U[:, k] - U[:, k + 1])
            G[:, k] += du
            G[:, k + 1] -= du
    sc = 1.0 / np.maximum(2.0 * np.diag(Rs), 1e-12)
    T = np.clip(U - sc[:, None] * G, u_min[:, None], u_max[:, None])
    proj = float(np.abs(U - T).max())
    comp = prim = 0.0
    Xs = X[:, 1:]
    nb = N - 1 if terminal == "equality" else N   # stages whose rows are box rows
    if x_min is not None and nb > 0:
        Xb, mb = Xs[:, :nb], mu[:, :nb]
        comp = max(float(np.where(mb > 0, np.abs(Xb - x_max[:, None]), 0.0).max()), float(np.where(mb < 0, np.abs(Xb - x_min[:, None]), 0.0).max()))
        prim = max(0.0, float((Xb - x_max[:, None]).max()), float((x_min[:, None] - Xb).max()))
    if terminal == "equality":
        prim = max(prim, float(np.abs(X[:, N] - x_ref[:, N]).max()))
    return max(proj, comp, prim), defect, G, (proj, comp, prim)


def rows_qp(A, B, c, X, U, x_ref, u_ref, Q, R, S, P, u_min, u_max, x_min, x_max, terminal, H=None, q=None):
    """One iteration's QP with its state rows, solved exactly: (v (m, N), mu (n, N), status of solve_qp_dual_active_set).  H, q: the
    Hessian and gradient to use in place of the Gauss-Newton ones (exact mode)."""
    n, N = X.shape[0], U.shape[1]
    m = U.shape[0]
    Hg, qg, lo, hi, Gam, g = mo.ltv_qp(A, B, c, X, U, x_ref, u_ref, Q, R, S, P, u_min, u_max, return_prediction=True)
    if H is None:
        H, q = Hg, qg
    C, a0, lo_c, hi_c, eq_c = mo.ltv_state_rows(Gam, g, X, x_ref, x_min, x_max, terminal)
    nz = H.shape[0]
    d = mo.jacobi_scaling(H)
    Hs = H * d[:, None] * d[None, :]
    Am = np.vstack([np.eye(nz), C * d[None, :]])
    Gi = np.linalg.inv(Hs)
    Ghat = Am @ Gi @ Am.T
    v0 = -Gi @ (q * d)
    s0 = Am @ v0 + np.concatenate([np.zeros(nz), a0])
    rr = mo.solve_qp_dual_active_set(Ghat, s0, np.concatenate([lo / d, lo_c]), np.concatenate([hi / d, hi_c]),
                                     np.concatenate([np.zeros(nz, dtype=bool), eq_c]))
    if rr["status"] != 0:
        return None, None, rr["status"]
    v = np.clip(rr["s"][:nz] * d, lo, hi).reshape(N, m).T
    mu = np.zeros((N, n))
    if x_min is not None:
        mu[:] = rr["lam"][nz:].reshape(N, n)      # row k n + i  <->  x_{k+1}[i]
    else:
        mu[N - 1] = rr["lam"][nz:]                # the terminal equality alone: the rows of stage N + 1
    return v, mu.T.copy(), 0


def exact_hessian_rows(model, X, U, A, B, c, x_ref, u_ref, Q, R, S, P, u_min, u_max, mu):
    """sqp_exact_ref.exact_qp with the row multipliers in the adjoint: (H_ex + shift, q_ex)."""
    n, N = X.shape[0], U.shape[1]
    m = U.shape[0]
    H, q, lo, hi, Gam, g = mo.ltv_qp(A, B, c, X, U, x_ref, u_ref, Q, R, S, P, u_min, u_max, return_prediction=True)
    Qs, Ps = 0.5 * (Q + Q.T), 0.5 * (P + P.T)
    L = np.zeros((n, N))
    lam = 2.0 * Ps @ (X[:, N] - x_ref[:, N]) + mu[:, N - 1]
    for k in range(N - 1, -1, -1):
        L[:, k] = lam
        lam = A[k].T @ lam + (2.0 * Qs @ (X[:, k] - x_ref[:, k]) + mu[:, k - 1] if k > 0 else 0.0)
    He, qe = H.copy(), q.copy()
    for k in range(N):
        Wk = xr.stage_hessian(model, X[:, k], U[:, k], L[:, k])
        Mk = np.zeros((n + m, N * m))
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
    return He + np.diag(delta * act.astype(np.float64)), qe


def sqp_solve_rows(model, x0, x_ref, u_ref, Q, R, S, P, u_min, u_max, x_min, x_max, terminal, max_iters, tol, adaptive=True, exact=False):
    """The loop of sqp_solve_ref.sqp_solve with state rows in every QP and their multipliers in the stopping test (and, with `exact`, in
    the Lagrangian Hessian).  Returns dict(status 0 converged / 1 iteration limit / 3 infeasible QP, iters, kkt, kkt_plain = the residual
    WITHOUT the row multipliers at the same iterate, X, U, mu (n, N) of the last solved QP, gn_fallbacks)."""
    m, N = u_ref.shape
    n = x0.size
    U = np.clip(u_ref, u_min[:, None], u_max[:, None]).astype(np.float64)
    X = mo.fnn_rollout(model, x0, U)
    Rz = R if R[0, 0] != 0.0 else 0.0 * R
    Sz = S if (R[0, 0] != 0.0 and S[0, 0] != 0.0) else 0.0 * S
    mu = np.zeros((n, N))
    mu_m = 2.0 * max(np.abs(P).max(), np.abs(Q).max())
    a, ref = 1.0, np.inf
    Xb = Ub = dXb = Vb = None
    fb = 0

    def merit(X, U, fv):
        EX, EU = X - x_ref, U - u_ref
        J = float(EX[:, N] @ P @ EX[:, N]) + sum(float(EX[:, k] @ Q @ EX[:, k] + EU[:, k] @ Rz @ EU[:, k]) for k in range(N))
        J += sum(float((U[:, k] - U[:, k + 1]) @ Sz @ (U[:, k] - U[:, k + 1])) for k in range(N - 1))
        return J + mu_m * float(np.abs(fv - X[:, 1:]).sum())

    def out(status, it, r):
        plain = sref.adjoint_residual(model, X, U, x_ref, u_ref, Q, R, S, P, u_min, u_max)[0]
        return dict(status=status, iters=it, kkt=r, kkt_plain=plain, X=X, U=U, mu=mu, gn_fallbacks=fb)

    it = 0
    if x_min is not None and not (np.all(x0 >= x_min) and np.all(x0 <= x_max)):
        return out(3, 0, np.inf)   # stage 1 is x0 itself: never a row, a feasibility check
    while True:
        r, dmax, _, _ = adjoint_residual_rows(model, X, U, x_ref, u_ref, Q, R, S, P, u_min, u_max, mu, x_min, x_max, terminal)
        if dmax <= DEFECT_TOL and r <= tol:
            return out(0, it, r)
        if it == max_iters:
            return out(1, it, r)
        it += 1
        fv = np.stack([model.forward(X[:, k], U[:, k]) for k in range(N)], axis=1)
        if adaptive:
            phi = merit(X, U, fv)
            if (phi <= ref + 1e-12 * abs(ref) + 1e-300) or a <= 1.0 / 64.0:
                ref, a = phi, min(1.0, 2.0 * a)
            else:   # the trial point is rejected: this iteration's QP is void, the multipliers stay those of the last solved QP
                a *= 0.5
                X = Xb + a * dXb
                U = np.clip(Ub + a * Vb, u_min[:, None], u_max[:, None])
                continue
        A, B, c = [], [], []
        for k in range(N):
            Ak, Bk = model.jacobian(X[:, k], U[:, k])
            A.append(Ak); B.append(Bk); c.append(fv[:, k] - X[:, k + 1])
        He = qe = None
        if exact:
            He, qe = exact_hessian_rows(model, X, U, A, B, c, x_ref, u_ref, Q, Rz, Sz, P, u_min, u_max, mu)
            try:
                np.linalg.cholesky(He)
            except np.linalg.LinAlgError:   # still indefinite: this iteration takes the Gauss-Newton QP
                He = qe = None
                fb += 1
        v, mu_new, st = rows_qp(A, B, c, X, U, x_ref, u_ref, Q, Rz, Sz, P, u_min, u_max, x_min, x_max, terminal, He, qe)
        if st != 0:
            return out(3 if st == 3 else 1, it - 1, r)
        mu = mu_new
        dX = np.zeros_like(X)
        dx = np.zeros(n)
        for k in range(N):
            dx = A[k] @ dx + B[k] @ v[:, k] + c[k]
            dX[:, k + 1] = dx
        if adaptive:
            Xb, Ub, dXb, Vb = X.copy(), U.copy(), dX, v
        sc = a if adaptive else 1.0
        X, U = X + sc * dX, np.clip(U + sc * v, u_min[:, None], u_max[:, None])


def nlp_rows_certificate(model, x0, U, x_ref, u_ref, Q, R, S, P, u_min, u_max, x_min=None, x_max=None, terminal="none", act_tol=1e-6):
    """Method-independent first-order certificate of a candidate U (m, N) for the NLP with state rows: the single-shooting gradient
    (mpc_oracle.nlp_cost_and_gradient), the sensitivities dX/dU of the rollout, and a bounded least-squares fit of the multipliers of
    the near-active state rows (sign by side; free on terminal-equality rows) and input bounds.  Returns (max of the scaled stationarity
    residual and the primal violation of the rows, number of multipliers fitted)."""
    from scipy.optimize import lsq_linear
    m, N = U.shape
    n = x0.size
    X = mo.fnn_rollout(model, x0, U)
    _, G, _ = mo.nlp_cost_and_gradient(model, x0, U, x_ref, u_ref, Q, R, S, P)
    Gam = np.zeros((N * n, N * m))
    Ak, Bk = [], []
    for k in range(N):
        A, B = model.jacobian(X[:, k], U[:, k])
        Ak.append(A); Bk.append(B)
    for j in range(N):
        blk = Bk[j]
        Gam[j * n:(j + 1) * n, j * m:(j + 1) * m] = blk
        for k in range(j + 1, N):
            blk = Ak[k] @ blk
            Gam[k * n:(k + 1) * n, j * m:(j + 1) * m] = blk
    g = G.T.reshape(-1)   # stage-major
    cols, lb, ub = [], [], []
    Xs = X[:, 1:]
    prim = 0.0
    for k in range(N):
        for i in range(n):
            if terminal == "equality" and k == N - 1:
                cols.append(Gam[k * n + i]); lb.append(-np.inf); ub.append(np.inf)
                prim = max(prim, abs(Xs[i, k] - x_ref[i, N]))
            elif x_min is not None:
                prim = max(prim, Xs[i, k] - x_max[i], x_min[i] - Xs[i, k])
                if Xs[i, k] >= x_max[i] - act_tol:
                    cols.append(Gam[k * n + i]); lb.append(0.0); ub.append(np.inf)
                elif Xs[i, k] <= x_min[i] + act_tol:
                    cols.append(Gam[k * n + i]); lb.append(-np.inf); ub.append(0.0)
    Uf = U.T.reshape(-1)
    for t in range(N * m):
        a = t % m
        e = np.zeros(N * m)
        e[t] = 1.0
        if Uf[t] >= u_max[a] - act_tol:
            cols.append(e); lb.append(0.0); ub.append(np.inf)
        elif Uf[t] <= u_min[a] + act_tol:
            cols.append(e); lb.append(-np.inf); ub.append(0.0)
    sc = np.tile(1.0 / np.maximum(2.0 * np.diag(R), 1e-12), N)
    if not cols:
        return max(float(np.abs(sc * g).max()), float(prim)), 0
    M = np.array(cols).T
    res = lsq_linear(M * sc[:, None], -g * sc, bounds=(np.array(lb), np.array(ub)), tol=1e-14)
    rvec = sc * (g + M @ res.x)
    return max(float(np.abs(rvec).max()), float(prim)), len(cols)


def state_box_fixture(b=24, N=20, first=40):
    """The batch of tests/test_gpu_sqp.py::test_sqp_with_state_box (Fnn 4-2-16x2 tanh, N 20, 24 instances; instances 9, 18, 19 have an
    infeasible first QP): model, problem data, box, initial states.  `first`, `b`: the splitmix stream continues for larger batches."""
    f = mo.synthetic_fnn(act="tanh")
    n, m = 4, 2
    x_ref = np.tile(np.array([0.2, -0.1, 0.05, 0.0])[:, None], (1, N + 1))
    u_ref = np.tile(np.array([0.1, -0.2])[:, None], (1, N))
    kw = dict(x_ref=x_ref, u_ref=u_ref, Q=100.0 * np.eye(n), R=0.1 * np.eye(m), S=np.zeros((m, m)), P=150.0 * np.eye(n),
              u_min=-np.ones(m), u_max=np.ones(m))
    xlo, xhi = np.array([-0.12, -0.58, -0.25, -0.35]), np.array([0.25, 0.09, 0.07, 0.22])
    X0 = x_ref[:, 0][None, :] + 0.5 * mo.splitmix_normal(0x5EED0005, first, b, n)
    X0 = np.clip(X0, xlo + 0.02 * (xhi - xlo), xhi - 0.02 * (xhi - xlo))
    return f, kw, xlo, xhi, X0


def terminal_equality_fixture(b=16, N=8):
    """Terminal equality at an equilibrium of the network: x_ref = its fixed point under u_ref = (0.1, -0.2) (500 applications from 0),
    N 8, X0 = x_ref + 0.3 * normals; no box."""
    f = mo.synthetic_fnn(act="tanh")
    n, m = 4, 2
    ur = np.array([0.1, -0.2])
    x = np.zeros(n)
    for _ in range(500):
        x = f.forward(x, ur)
    x_ref = np.tile(x[:, None], (1, N + 1))
    u_ref = np.tile(ur[:, None], (1, N))
    kw = dict(x_ref=x_ref, u_ref=u_ref, Q=100.0 * np.eye(n), R=0.1 * np.eye(m), S=np.zeros((m, m)), P=150.0 * np.eye(n),
              u_min=-np.ones(m), u_max=np.ones(m))
    X0 = x[None, :] + 0.3 * mo.splitmix_normal(0x5EED0005, 40, b, n)
    return f, kw, X0
