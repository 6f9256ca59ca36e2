"""numpy restatement of the adjoint of P = DARE(A, B, Q, R) (include/almpc.h almpc_dare_vjp, csrc/almpc_dare_vjp.hip.h), twice:

  lyap      the formulas with scipy.linalg.solve_discrete_lyapunov:
            Sm = R + B'PB, K = Sm^-1 B'PA, Acl = A - B K, X = Acl X Acl' + gP,
            gQ = X, gR = K X K', gA = 2 P Acl X, gB = -2 P Acl X K';
  doubling  what the kernel and hm::dare_vjp compute, statement by statement: the residual test of k_dare (status 3), the pivot
            test of Sm (status 1), X_0 = gP, A_0 = Acl, D = A_j X_j A_j', X_{j+1} = sym(X_j + D), A_{j+1} = A_j A_j until
            max|D| <= 1e-13 max(1, max|X_{j+1}|), at most 64 doublings (status 2 beyond, or when X is not finite).

gP is the symmetric matrix with dL = sum_ij gP_ij dP_ij for symmetric dP; gQ and gR follow the same convention.
"""
import numpy as np
import scipy.linalg as sla

GROUPS = ("A", "B", "Q", "R")
MAX_DOUBLINGS = 64
RTOL = 1e-9   # the relative bound the project holds k_dare to (tests/test_gpu_dare.py P_RTOL)


def _sym(M):
    return 0.5 * (M + M.T)


def gain(A, B, R, P):
    return np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A)


def dare_vjp_lyap(A, B, Q, R, P, gP):
    K = gain(A, B, R, P)
    Acl = A - B @ K
    X = sla.solve_discrete_lyapunov(Acl, gP)
    PAX = P @ Acl @ X
    return {"A": 2.0 * PAX, "B": -2.0 * PAX @ K.T, "Q": X, "R": K @ X @ K.T}


def dare_vjp_doubling(A, B, Q, R, P, gP):
    """(status, {group: gradient} or None, doublings)."""
    A, B, Q, R, P, gP = (np.asarray(a, dtype=np.float64) for a in (A, B, Q, R, P, gP))
    PA, PB = P @ A, P @ B
    Sm = B.T @ PB + R
    with np.errstate(all="ignore"):
        try:
            K = np.linalg.solve(Sm, B.T @ PA)
        except np.linalg.LinAlgError:
            return 1, None, 0
        if not np.all(np.isfinite(K)):
            return 1, None, 0
        res = A.T @ PA + (Q - P - (A.T @ PB) @ K)
        if not np.abs(res).max() <= 1e-7 * max(1.0, np.abs(P).max(), np.abs(Q).max()):
            return 3, None, 0
        Aj = A - B @ K
        PAcl = P @ Aj
        X = gP.copy()
        for it in range(MAX_DOUBLINGS):
            D = Aj @ X @ Aj.T
            X = _sym(X + D)
            Aj = Aj @ Aj
            if not np.all(np.isfinite(X)):
                return 2, None, it + 1
            if np.abs(D).max() <= 1e-13 * max(1.0, np.abs(X).max()):
                PAX = PAcl @ X
                return 0, {"A": 2.0 * PAX, "B": -2.0 * PAX @ K.T, "Q": X, "R": _sym(K @ X @ K.T)}, it + 1
    return 2, None, MAX_DOUBLINGS


def slow_mode_model(lam):
    """A = diag(lam, .5, .5, .5) with A[1, 2] = .3, row 0 of B zero: a stable mode of radius lam no input reaches (n 4, m 2), so the
    closed loop keeps it and the doubling needs log2(log(1e-13) / log(lam)) steps.  Returns A, B, Q, R."""
    A = np.diag([lam, 0.5, 0.5, 0.5])
    A[1, 2] = 0.3
    B = np.random.default_rng(3).standard_normal((4, 2))
    B[0, :] = 0.0
    return A, B, 100.0 * np.eye(4), 0.1 * np.eye(2)


def random_symmetric(rng, n):
    return _sym(rng.standard_normal((n, n)))


def worst_gap(got, ref):
    """max over the groups of |got - ref|_max / max(1, max|ref group|), and the group."""
    gaps = {k: float(np.abs(np.asarray(got[k]) - ref[k]).max()) / max(1.0, float(np.abs(ref[k]).max())) for k in ref}
    k = max(gaps, key=gaps.get)
    return gaps[k], k
