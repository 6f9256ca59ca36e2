"""numpy restatement of the solution sensitivities for designs with state rows (include/almpc.h "Rows form",
csrc/almpc_sens.hip.h), three times:

  direct     the KKT system of the face  [[H, A_W'], [A_W, 0]] [dv; dlam] = [-F; -Phi_W]  on the unscaled H, F: A_W holds a unit row for
             every input row of W and the row of Gamma for every state row (Phi_W: its row of Phi, zero for an input row).  No inverse
             of H, no scaling;
  G form     what the device computes: Ghat = A G A' with A = [I; C'], C' = Gamma_rows D, T1 = A V + [0; Phi_rows], S = Ghat[W,W],
             dw/dx0 = T1[0:nz] - Ghat[0:nz, W] S^-1 T1[W], dv/dx0 = D dw/dx0 (input rows of W zero);
  projected  the same in the quantities projected on the terminal-equality rows E: Ghat_p = Ghat - Ghat[:,E] Ghat_EE^-1 Ghat[E,:],
             T1_p = T1 - Ghat[:,E] Ghat_EE^-1 T1[E], W' = W \\ E.

Conventions are those of tests/sens_ref.py (J = du/dx0 is nz x n, stage-major; x is (n, N+1) with x[:,0] = x0).  State rows come in the
handle's order: stage by stage (stages 2..N+1 of the trajectory, columns 1..N of x), state by state; with a box every stage has its n
rows, the last stage's being equality rows where the terminal equality is on; without a box only those n rows exist.
"""
import numpy as np

import sens_ref as sr

ACT_TOL_X = 1e-7   # almpc_sensitivity_rows' default for state rows (act_tol_x <= 0)
NO_BOX = 1e300     # a bound of at least this size (or not finite) is never active


def state_rows(n, N, box, terminal_eq):
    """(stage, state, is_eq) arrays of the state rows; stage k = column k of x (1..N)."""
    st, ix, eq = [], [], []
    for k in range(1, N + 1):
        for i in range(n):
            is_eq = terminal_eq and k == N
            if box or is_eq:
                st.append(k); ix.append(i); eq.append(is_eq)
    return np.array(st, dtype=int), np.array(ix, dtype=int), np.array(eq, dtype=bool)


def row_tables(A, B, N, stage, state):
    """(Gamma_rows (mc, nz), Phi_rows (mc, n)) of x[state, stage] = (Phi e0 + Gamma v)_row + reference terms."""
    n, m = B.shape
    pw = [np.eye(n)]
    for _ in range(N):
        pw.append(A @ pw[-1])
    Gam = np.zeros((len(stage), m * N))
    Phi = np.zeros((len(stage), n))
    for r, (k, i) in enumerate(zip(stage, state)):
        Phi[r] = pw[k][i]
        for j in range(k):
            Gam[r, j * m:(j + 1) * m] = (pw[k - 1 - j] @ B)[i]
    return Gam, Phi


def active_state_rows(x, x_min, x_max, stage, state, eq, tau=ACT_TOL_X):
    """The contract's rule on the returned states x (n, N+1): every equality row; a box row iff x - xmin <= tau max(1, |xmin|) or
    xmax - x <= tau max(1, |xmax|), a bound that is not finite or at least 1e300 in size never."""
    act = np.array(eq, dtype=bool).copy()
    if x_min is None:
        return act
    for r, (k, i) in enumerate(zip(stage, state)):
        if eq[r]:
            continue
        lo, hi, v = float(x_min[i]), float(x_max[i]), x[i, k]
        act[r] = bool((abs(lo) < NO_BOX and v - lo <= tau * max(1.0, abs(lo))) or (abs(hi) < NO_BOX and hi - v <= tau * max(1.0, abs(hi))))
    return act


def bound_gaps(x, x_min, x_max, stage, state, eq):
    """Distance of every box row from its nearer bound over max(1, |bound|) (inf for an equality row or a bound that is none)."""
    out = np.full(len(stage), np.inf)
    if x_min is None:
        return out
    for r, (k, i) in enumerate(zip(stage, state)):
        if eq[r]:
            continue
        for b, dist in ((float(x_min[i]), x[i, k] - x_min[i]), (float(x_max[i]), x_max[i] - x[i, k])):
            if abs(b) < NO_BOX:
                out[r] = min(out[r], dist / max(1.0, abs(b)))
    return out


# ---- (a) direct ------------------------------------------------------------------------------------------------------------------
def jac_direct(H, F, Gam, Phi, act_u, act_x):
    nz, n = F.shape
    Wu, Wx = np.nonzero(act_u)[0], np.nonzero(act_x)[0]
    AW = np.vstack([np.eye(nz)[Wu], Gam[Wx]])
    PW = np.vstack([np.zeros((Wu.size, n)), Phi[Wx]])
    k = AW.shape[0]
    K = np.block([[H, AW.T], [AW, np.zeros((k, k))]])
    sol = np.linalg.solve(K, np.vstack([-F, -PW]))
    J = sol[:nz]
    J[Wu] = 0.0
    return J


def vjp_direct(H, F, Gam, Phi, act_u, act_x, A, B, g_u, g_x):
    lam1, q = sr.adjoint(A, B, g_u, g_x)
    return lam1 + jac_direct(H, F, Gam, Phi, act_u, act_x).T @ q


# ---- (b) G form ------------------------------------------------------------------------------------------------------------------
def rows_operands(H, F, d, Gam, Phi):
    """(Ghat (R, R), T1 (R, n)) of a design, once."""
    G, V = sr.g_operands(H, F, d)
    Aall = np.vstack([np.eye(H.shape[0]), Gam * d[None, :]])
    Ghat = Aall @ G @ Aall.T
    T1 = Aall @ V + np.vstack([np.zeros_like(V), Phi])
    return 0.5 * (Ghat + Ghat.T), T1


def project(Ghat, T1, E):
    """The operands projected on the rows E (rows / columns E exactly zero)."""
    GE = Ghat[:, E]
    Y = np.linalg.solve(Ghat[np.ix_(E, E)], np.hstack([GE.T, T1[E]]))
    R = Ghat.shape[0]
    Gp, Tp = Ghat - GE @ Y[:, :R], T1 - GE @ Y[:, R:]
    Gp[E, :] = 0.0; Gp[:, E] = 0.0; Tp[E] = 0.0
    return 0.5 * (Gp + Gp.T), Tp


def _gform(Ghat, T1, d, W, nz):
    Jw = T1[:nz].copy()
    if W.size:
        Jw = Jw - Ghat[:nz][:, W] @ np.linalg.solve(Ghat[np.ix_(W, W)], T1[W])
        Jw[W[W < nz]] = 0.0
    return d[:, None] * Jw


def jac_gform(ops, d, act_u, act_x):
    Ghat, T1 = ops
    return _gform(Ghat, T1, d, np.nonzero(np.concatenate([act_u, act_x]))[0], d.size)


def jac_projected(ops_p, d, act_u, act_x, eq):
    """ops_p = project(*ops, nz + nonzero(eq)); the equality rows leave W."""
    Ghat, T1 = ops_p
    return _gform(Ghat, T1, d, np.nonzero(np.concatenate([act_u, act_x & ~eq]))[0], d.size)


def _vjp_gform(Ghat, T1, d, W, A, B, g_u, g_x):
    nz = d.size
    lam1, q = sr.adjoint(A, B, g_u, g_x)
    p = d * q
    p[W[W < nz]] = 0.0
    out = lam1 + T1[:nz].T @ p
    if W.size:
        out = out - T1[W].T @ np.linalg.solve(Ghat[np.ix_(W, W)], Ghat[W][:, :nz] @ p)
    return out


def vjp_gform(ops, d, act_u, act_x, A, B, g_u, g_x):
    return _vjp_gform(ops[0], ops[1], d, np.nonzero(np.concatenate([act_u, act_x]))[0], A, B, g_u, g_x)


def vjp_projected(ops_p, d, act_u, act_x, eq, A, B, g_u, g_x):
    return _vjp_gform(ops_p[0], ops_p[1], d, np.nonzero(np.concatenate([act_u, act_x & ~eq]))[0], A, B, g_u, g_x)


def cond_S(ops, act_u, act_x):
    W = np.nonzero(np.concatenate([act_u, act_x]))[0]
    return float(np.linalg.cond(ops[0][np.ix_(W, W)])) if W.size else 1.0
