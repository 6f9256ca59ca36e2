"""numpy restatement of the certificate of a step (include/almpc.h "Certificate of the last step"; k_cert): the cost, the costates,
the input gradient and the KKT residual of one instance from (A, B, Q, R, S, P, umin, umax, e_x, e_u, u), with the error bound of
every value.

Stages 0-based, e_k = e_x[:, k], v_k = e_u[:, k], u_k = u[:, k], d_i = u_i - u_{i+1}; Q, R, S, P symmetrised as 0.5 (M + M');
useR = R[0,0] != 0, useS = useR and S[0,0] != 0 (the reference's branch rule, src/sub/design_mpc.jl:436-465):
    J     = e_N'P e_N + sum_{k<N} (e_k'Q e_k + [useR] v_k'R v_k) + [useS] sum_{i<N-1} d_i'S d_i
    lam_N = 2 P e_N,  lam_k = 2 Q e_k + A'lam_{k+1}
    g_k   = B'lam_{k+1} + [useR] 2 R v_k + [useS]([k < N-1] 2 S d_k - [k > 0] 2 S d_{k-1})
    res   = max |u_k - clip(u_k - g_k, umin, umax)|

Error bounds.  Next to each value the same recursion is run with the absolute value of every operand and every term (`mag`), and
`ops` bounds the number of roundings on any path from an input to the output.  Whatever the order of the sums, and with or without
fused multiply-adds (which only remove roundings), a computed value differs from the exact one by at most gamma_ops mag,
gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1 and section 3.1).  Two such
computations therefore differ by at most
    tol = 2 ops u mag / (1 - ops u).
The counts (multiplications by 0.5 and 2 are exact):
    a symmetrised entry: 1;  a product row of length c: 1 + (c - 1);  so one level of the costate recursion costs at most
    1 (sym) + n (product) + 1 (the add of 2 Q e_k) <= n + 3, and  ops_lam[k] = (N - k + 1)(n + 3);
    g_k:  ops_lam[k+1] + (n + 1) for B'lam, the weight terms <= 1 (d) + 1 (sym) + m (product) each, 3 adds:
          ops_grad[k] = ops_lam[k+1] + n + m + 7;
    cost: a term 0.5 a.b with b one product: <= max(n, m) + 4; the sum of T = (N + 1) n + 2 N m terms in any order, a butterfly
          included: <= T more:  ops_cost = max(n, m) + 4 + T;
    res:  u - g, the clip (exact) and the difference: each at most one rounding of a number no larger than |u| + |g|, on top of
          the error of g:  tol_res = max(tol_grad) + 2^-52 max(|u| + |g|).
"""
import numpy as np

U = 2.0 ** -53


def tol_of(ops, mag):
    ops = np.asarray(ops, dtype=np.float64)
    return 2.0 * ops * U * np.asarray(mag) / (1.0 - ops * U)


def sym(M):
    M = np.asarray(M, dtype=np.float64)
    return 0.5 * (M + M.T)


def branch(R, S):
    useR = np.asarray(R)[0, 0] != 0.0
    return bool(useR), bool(useR and S is not None and np.asarray(S)[0, 0] != 0.0)


def _recursion(A, B, Q, R, S, P, e_x, e_u, u, useR, useS, absval):
    """cost, lam (n, N+1), g (m, N); absval: every operand and every term by its absolute value (differences become sums)."""
    a = np.abs if absval else (lambda x: x)
    A, B, Q, P, e_x, e_u, u = a(A), a(B), a(Q), a(P), a(e_x), a(e_u), a(u)
    R = a(R) if useR else None
    S = a(S) if useS else None
    n, N = e_x.shape[0], e_u.shape[1]
    m = e_u.shape[0]
    lam = np.zeros((n, N + 1))
    g = np.zeros((m, N))
    lam[:, N] = 2.0 * (P @ e_x[:, N])
    cost = 0.5 * float(e_x[:, N] @ lam[:, N])
    d = (u[:, :-1] + u[:, 1:]) if absval else (u[:, :-1] - u[:, 1:])   # d_i, i = 0 .. N-2
    s = 2.0 * (S @ d) if useS else np.zeros((m, max(N - 1, 0)))        # 2 S d_i
    if useS:
        cost += 0.5 * float(np.sum(d * s))
    for k in range(N - 1, -1, -1):
        q = 2.0 * (Q @ e_x[:, k])
        lam[:, k] = q + A.T @ lam[:, k + 1]
        cost += 0.5 * float(e_x[:, k] @ q)
        gk = B.T @ lam[:, k + 1]
        if useR:
            r = 2.0 * (R @ e_u[:, k])
            gk = gk + r
            cost += 0.5 * float(e_u[:, k] @ r)
        if useS:
            if k < N - 1:
                gk = gk + s[:, k]
            if k > 0:
                gk = gk + s[:, k - 1] if absval else gk - s[:, k - 1]
        g[:, k] = gk
    return cost, lam, g


def certificate(A, B, Q, R, S, P, umin, umax, e_x, e_u, u, useR=None, useS=None):
    """The four quantities of one instance and their bounds.  e_x (n, N+1), e_u and u (m, N).  Returns a dict with cost, res,
    grad (m, N), costate (n, N+1); mag_* and ops_* of cost, grad, costate; tol_* of all four (see the module's docstring)."""
    A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    e_x = np.asarray(e_x, dtype=np.float64); e_u = np.asarray(e_u, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    n, m, N = A.shape[0], B.shape[1], e_u.shape[1]
    bR, bS = branch(R, S)
    useR = bR if useR is None else bool(useR)
    useS = bS if useS is None else bool(useS)
    Qs, Ps = sym(Q), sym(P)
    Rs = sym(R) if useR else None
    Ss = sym(S) if useS else None
    cost, lam, g = _recursion(A, B, Qs, Rs, Ss, Ps, e_x, e_u, u, useR, useS, False)
    mcost, mlam, mg = _recursion(A, B, Qs, Rs, Ss, Ps, e_x, e_u, u, useR, useS, True)
    lo = np.asarray(umin, dtype=np.float64).reshape(m, 1); hi = np.asarray(umax, dtype=np.float64).reshape(m, 1)
    res = float(np.max(np.abs(u - np.clip(u - g, lo, hi))))
    ops_lam = (N - np.arange(N + 1) + 1) * (n + 3)               # [N+1]
    ops_grad = ops_lam[1:] + n + m + 7                           # [N]
    ops_cost = max(n, m) + 4 + (N + 1) * n + 2 * N * m
    out = dict(cost=cost, res=res, grad=g, costate=lam, mag_cost=mcost, mag_grad=mg, mag_costate=mlam,
               ops_cost=ops_cost, ops_grad=np.broadcast_to(ops_grad, (m, N)).copy(), ops_costate=np.broadcast_to(ops_lam, (n, N + 1)).copy())
    out["tol_cost"] = float(tol_of(ops_cost, mcost))
    out["tol_grad"] = tol_of(out["ops_grad"], mg)
    out["tol_costate"] = tol_of(out["ops_costate"], mlam)
    with np.errstate(invalid="ignore"):
        out["tol_res"] = float(np.max(out["tol_grad"]) + 2.0 ** -52 * np.max(np.abs(u) + np.abs(g)))
    return out


def condensed_bound(A, B, Q, R, S, P, N, e0, v, u_ref, useR, useS):
    """Error bound of the condensed forms of oracle/mpc_oracle.py (condense, condensed_qp) at (e0, v): the same construction on absolute
    values (D'SD with every block positive) gives the magnitudes, and `ops` bounds the roundings on a path to an entry of H v + f:
    A^k (k n), times B (n), Qbar Gamma (n), Gamma'(..) (n N), the R and S blocks, the symmetrisation and their sum (4), H v (m N) or
    F e0 through Phi (no longer), the add of f (2), and with S the 2 D'Sbar D u_ref term (2 m + m N).
    Returns dict(mag_grad (m, N) = 2 |H||v| + |f|, ops, Phi, H, f): the last three on absolute values, H without the factor 2."""
    aA, aB, aQ, aP = np.abs(A), np.abs(B), np.abs(sym(Q)), np.abs(sym(P))
    n, m = B.shape
    Phi = np.zeros((n * N, n)); Gam = np.zeros((n * N, m * N))
    Ak = np.eye(n); G = []
    for k in range(N):
        G.append(Ak @ aB); Ak = Ak @ aA; Phi[k * n:(k + 1) * n] = Ak
    for i in range(N):
        for j in range(i + 1):
            Gam[i * n:(i + 1) * n, j * m:(j + 1) * m] = G[i - j]
    Qbar = np.kron(np.eye(N), aQ); Qbar[-n:, -n:] = aP
    H = Gam.T @ Qbar @ Gam
    if useR:
        H = H + np.kron(np.eye(N), np.abs(sym(R)))
    f = 2.0 * Gam.T @ Qbar @ Phi @ np.abs(e0)
    if useS and N > 1:
        D = np.zeros((m * (N - 1), m * N))
        for i in range(N - 1):
            D[i * m:(i + 1) * m, i * m:(i + 1) * m] = np.eye(m); D[i * m:(i + 1) * m, (i + 1) * m:(i + 2) * m] = np.eye(m)
        DSD = D.T @ np.kron(np.eye(N - 1), np.abs(sym(S))) @ D
        H = H + DSD
        f = f + 2.0 * DSD @ np.abs(u_ref).T.reshape(-1)
    mag = 2.0 * H @ np.abs(v) + f
    ops = 2 * n * N + 2 * n + m * N + 6 + (2 * m + m * N if useS else 0)
    return dict(mag_grad=mag.reshape(N, m).T, ops=ops, Phi=Phi, H=H, f=f)


def gamma(ops):
    return ops * U / (1.0 - ops * U)
