"""numpy restatement of the certificate of a step of a time-varying design (include/almpc.h "Certificate of a step of a time-varying
design"; k_cert_ltv): the predicted states, the cost, the costates, the input gradient and the KKT residual of one instance from the
stage models (A_k, B_k, c_k), the trajectory (xbar), the references, the weights, the box and the step's (v, u), with the error bound
of every value.

Stages 0-based, v_k = e_u[:, k], u_k = u[:, k], w_k = u_k - uref_k, d_i = u_i - u_{i+1}; Q, R, S, P symmetrised as 0.5 (M + M');
useR = R[0,0] != 0, useS = useR and S[0,0] != 0:
    forward   dx_0 = 0,  dx_{k+1} = A_k dx_k + B_k v_k + c_k,  x_k = xbar_k + dx_k,  e_k = x_k - xref_k
    cost      J = e_N'P e_N + sum_{k<N} (e_k'Q e_k + [useR] w_k'R w_k) + [useS] sum_{i<N-1} d_i'S d_i
    backward  lam_N = 2 P e_N,  lam_k = 2 Q e_k + A_k'lam_{k+1}
              g_k = B_k'lam_{k+1} + [useR] 2 R w_k + [useS]([k < N-1] 2 S d_k - [k > 0] 2 S d_{k-1})
    res       max |u_k - clip(u_k - g_k, umin, umax)|

Error bounds, built as tests/cert_ref.py builds its own: next to each value the same recursion runs on the absolute value of every operand
and every term (`mag`; a difference becomes a sum), and `ops` bounds the number of roundings on any path from an input to the output.
Whatever the order of the sums, with or without fused multiply-adds, a computed value differs from the exact one by at most
gamma_ops mag, gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Lemma 3.1), so two computations differ by at most
    tol = 2 ops u mag / (1 - ops u).
The counts (multiplications by 0.5 and 2 are exact; a product row of length c costs c roundings):
    forward:  one level dx_k -> dx_{k+1} is a row of A_k (n), a row of B_k (m), the add of the two sums and the add of c_k:
              <= n + m + 2, so ops_dx[k] = k (n + m + 2);  x_k = xbar_k + dx_k: ops_x[k] = ops_dx[k] + 1;  e_k = x_k - xref_k:
              ops_e[k] = ops_dx[k] + 2.  Every e_k has at most ops_e[N] = N (n + m + 2) + 2 =: F.
    backward: a path to lam_k starts at some e_j (<= F), then one level of the recursion per stage j .. k, each <= 1 (sym) + n (product)
              + 1 (the add of 2 Q e) = n + 3:  ops_lam[k] = F + (N - k + 1)(n + 3);
    g_k:      ops_lam[k+1] + (n + 1) for B_k'lam, the weight terms <= 1 (w or d) + 1 (sym) + m (product) each, 3 adds:
              ops_grad[k] = ops_lam[k+1] + n + m + 7;
    cost:     a term 0.5 a.b with b one product of a: both factors carry the roundings of a (<= F each, the factor w or d one), the product
              and the term <= max(n, m) + 4, and the sum of T = (N + 1) n + 2 N m terms in any order, a butterfly included, <= T more:
              ops_cost = 2 F + max(n, m) + 4 + T;
    res:      u - g, the clip (exact) and the difference: each at most one rounding of a number no larger than |u| + |g|, on top of
              the error of g:  tol_res = max(tol_grad) + 2^-52 max(|u| + |g|).
"""
import numpy as np

from cert_ref import U, branch, gamma, sym, tol_of   # noqa: F401  (re-exported for the tests)


def _sweeps(A, B, c, xbar, xref, uref, Q, R, S, P, v, u, useR, useS, absval):
    """x, e (n, N+1), cost, lam (n, N+1), g (m, N); absval: every operand and every term by its absolute value"""
    a = np.abs if absval else (lambda z: z)
    A, B, xbar, xref, uref, Q, P, v, u = a(A), a(B), a(xbar), a(xref), a(uref), a(Q), a(P), a(v), a(u)
    N, n, m = A.shape[0], A.shape[1], B.shape[2]
    c = np.zeros((N, n)) if c is None else a(c)
    R = a(R) if useR else None
    S = a(S) if useS else None
    x = np.zeros((n, N + 1)); e = np.zeros((n, N + 1))
    dx = np.zeros(n)
    x[:, 0] = xbar[:, 0]
    for k in range(N):
        dx = A[k] @ dx + B[k] @ v[:, k] + c[k]
        x[:, k + 1] = xbar[:, k + 1] + dx
    e = x + xref if absval else x - xref
    w = u + uref if absval else u - uref
    lam = np.zeros((n, N + 1)); g = np.zeros((m, N))
    lam[:, N] = 2.0 * (P @ e[:, N])
    cost = 0.5 * float(e[:, N] @ lam[:, N])
    d = (u[:, :-1] + u[:, 1:]) if absval else (u[:, :-1] - u[:, 1:])   # d_i, i = 0 .. N-2
    s = 2.0 * (S @ d) if useS else np.zeros((m, max(N - 1, 0)))        # 2 S d_i
    if useS:
        cost += 0.5 * float(np.sum(d * s))
    for k in range(N - 1, -1, -1):
        q = 2.0 * (Q @ e[:, k])
        lam[:, k] = q + A[k].T @ lam[:, k + 1]
        cost += 0.5 * float(e[:, k] @ q)
        gk = B[k].T @ lam[:, k + 1]
        if useR:
            r = 2.0 * (R @ w[:, k])
            gk = gk + r
            cost += 0.5 * float(w[:, k] @ r)
        if useS:
            if k < N - 1:
                gk = gk + s[:, k]
            if k > 0:
                gk = gk + s[:, k - 1] if absval else gk - s[:, k - 1]
        g[:, k] = gk
    return x, e, cost, lam, g


def certificate_ltv(A, B, c, xbar, xref, uref, Q, R, S, P, umin, umax, v, u, useR=None, useS=None):
    """The six quantities of one instance and their bounds.  A (N, n, n), B (N, n, m), c (N, n) or None, xbar (n, N+1), xref (n, N+1) or
    None, uref (m, N) or None, v = e_u and u (m, N).  Returns a dict with cost, res, grad (m, N), costate (n, N+1), x, e_x (n, N+1);
    mag_*, ops_* and tol_* of each (see the module's docstring)."""
    A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    c = None if c is None else np.asarray(c, dtype=np.float64)
    xbar = np.asarray(xbar, dtype=np.float64); v = np.asarray(v, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    N, n, m = A.shape[0], A.shape[1], B.shape[2]
    xref = np.zeros((n, N + 1)) if xref is None else np.asarray(xref, dtype=np.float64)
    uref = np.zeros((m, N)) if uref is None else np.asarray(uref, dtype=np.float64)
    bR, bS = branch(R, S)
    useR = bR if useR is None else bool(useR)
    useS = bS if useS is None else bool(useS)
    Qs, Ps = sym(Q), sym(P)
    Rs = sym(R) if useR else None
    Ss = sym(S) if useS else None
    x, e, cost, lam, g = _sweeps(A, B, c, xbar, xref, uref, Qs, Rs, Ss, Ps, v, u, useR, useS, False)
    mx, me, mcost, mlam, mg = _sweeps(A, B, c, xbar, xref, uref, Qs, Rs, Ss, Ps, v, u, useR, useS, True)
    lo = np.asarray(umin, dtype=np.float64).reshape(m, 1); hi = np.asarray(umax, dtype=np.float64).reshape(m, 1)
    res = float(np.max(np.abs(u - np.clip(u - g, lo, hi))))
    ks = np.arange(N + 1)
    ops_dx = ks * (n + m + 2)
    F = int(ops_dx[N]) + 2
    ops_lam = F + (N - ks + 1) * (n + 3)
    ops_grad = ops_lam[1:] + n + m + 7
    ops_cost = 2 * F + max(n, m) + 4 + (N + 1) * n + 2 * N * m
    bc = lambda o, rows: np.broadcast_to(o, (rows, len(o))).copy()
    out = dict(cost=cost, res=res, grad=g, costate=lam, x=x, e_x=e, mag_cost=mcost, mag_grad=mg, mag_costate=mlam, mag_x=mx, mag_e_x=me,
               ops_cost=ops_cost, ops_grad=bc(ops_grad, m), ops_costate=bc(ops_lam, n), ops_x=bc(ops_dx + 1, n), ops_e_x=bc(ops_dx + 2, n))
    out["tol_cost"] = float(tol_of(ops_cost, mcost))
    for k in ("grad", "costate", "x", "e_x"):
        out["tol_" + k] = tol_of(out["ops_" + k], out["mag_" + k])
    with np.errstate(invalid="ignore"):
        out["tol_res"] = float(np.max(out["tol_grad"]) + 2.0 ** -52 * np.max(np.abs(u) + np.abs(g)))
    return out


def qp_bound(mo, A, B, c, xbar, ubar, xref, uref, Q, R, S, P, umin, umax, useR, useS):
    """Error bound of oracle/mpc_oracle.py::ltv_qp: the same construction on absolute values, with the differences xbar - xref and
    ubar - uref turned into sums by the sign of the references, and D'SD with every block positive (added here: the oracle's D has -I
    blocks).  `ops` bounds the roundings on a path to an entry of H v + q or Gam v + g: the rows of Gam (n per stage: n N), Qbar Gam (n),
    Gam'(..) (n N), the R and S blocks, the symmetrisation and their sums (6), H v or Gam v (m N), g + ebar and the add of q (3), and with
    S the D'SD ubar term (2 m + m N).  Returns dict(H, q, Gam, g, ops): the first four on absolute values."""
    N, n, m = A.shape[0], A.shape[1], B.shape[2]
    xr = np.zeros((n, N + 1)) if xref is None else -np.abs(xref)
    ur = np.zeros((m, N)) if uref is None else -np.abs(uref)
    aR = np.abs(sym(R)) if useR else np.zeros((m, m))
    H, q, _, _, Gam, g = mo.ltv_qp(np.abs(A), np.abs(B), None if c is None else np.abs(c), np.abs(xbar), np.abs(ubar), xr, ur,
                                   np.abs(sym(Q)), aR, np.zeros((m, m)), np.abs(sym(P)), umin, umax, return_prediction=True)
    if useS and N > 1:
        D = np.zeros((m * (N - 1), m * N))
        for i in range(N - 1):
            D[i * m:(i + 1) * m, i * m:(i + 1) * m] = np.eye(m); D[i * m:(i + 1) * m, (i + 1) * m:(i + 2) * m] = np.eye(m)
        DSD = D.T @ np.kron(np.eye(N - 1), np.abs(sym(S))) @ D
        H = H + 2.0 * DSD
        q = q + 2.0 * DSD @ np.abs(ubar).T.reshape(-1)
    ops = 2 * n * N + n + m * N + 9 + (2 * m + m * N if useS else 0)
    return dict(H=H, q=q, Gam=Gam, g=g, ops=ops)
