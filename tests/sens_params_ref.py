"""numpy restatement of the parameter gradients of the solution (include/almpc.h "Parameter gradients", csrc/almpc_sens.hip.h), twice:

  direct   z_F = -H_FF^-1 q_F with the unscaled H (no scaling, no inverse), nu_W = q_W + (H z)_W;
  G form   what the device computes: G = (DHD)^-1, p = d o q (zero on W), t = S^-1 G[W,:] p, z = -d o (G p - G[:,W] t) (zero on W),
           nu_j = q_j + t_a / d_j for j = W[a].

Both share the stage recursions (zeta forward, mu and alpha backward) and the outer-product sums.  Conventions as tests/sens_ref.py:
rows stage-major (j = k m + i), a loss has gradients g_u (m, N), g_x (n, N+1); e_x (n, N+1), v = e_u (m, N), u (m, N) are the step's
results.  A symmetric matrix gradient G_Q is the symmetric matrix with dL = sum_ij (G_Q)_ij dQ_ij for symmetric dQ; P is data (its
dependence on A, B, Q, R through a DARE is not followed); where the design drops R or S (the [1,1] rule) that gradient is zero.
"""
import numpy as np

import sens_ref as sr

GROUPS = ("x0", "f", "u_ref", "u_min", "u_max", "Q", "P", "A", "R", "S", "B")


def sides(u, u_min, u_max, d, tau=sr.ACT_TOL):
    """(act, lower) of the contract's rule on the returned inputs u (m, N): a row at both bounds counts as lower."""
    m, N = u.shape
    uf = u.T.reshape(-1)
    lower = uf - np.tile(np.asarray(u_min, float), N) <= tau * d
    return sr.active_rows(u, u_min, u_max, d, tau), lower


def z_nu_direct(H, act, q):
    fr = ~act
    z = np.zeros_like(q)
    if fr.any():
        z[fr] = -np.linalg.solve(H[np.ix_(fr, fr)], q[fr])
    nu = np.where(act, q + H @ z, 0.0)
    return z, nu


def z_nu_gform(G, d, act, q):
    """G = (DHD)^-1 (sens_ref.g_operands(H, F, d)[0])."""
    W = np.nonzero(act)[0]
    p = d * q
    p[W] = 0.0
    Gp = G @ p
    nu = np.zeros_like(q)
    if W.size:
        t = np.linalg.solve(G[np.ix_(W, W)], Gp[W])
        Gp = Gp - G[:, W] @ t
        nu[W] = q[W] + t / d[W]
    z = -d * Gp
    z[W] = 0.0
    return z, nu


def gradients(prob, act, lower, res, g_u, g_x, z, nu):
    """Everything behind (z, nu).  prob: A, B, Q, P, S and the flags useR, useS of the design; res: e_x, e_u, u of the step."""
    A, B, Q, P, S = (np.asarray(prob[k], float) for k in ("A", "B", "Q", "P", "S"))
    n, m = B.shape
    N = g_u.shape[1]
    ex, v, u = res["e_x"], res["e_u"], res["u"]
    Z = z.reshape(N, m).T                                   # (m, N)
    sym = lambda a, b: np.outer(a, b) + np.outer(b, a)
    Qbar = lambda k: np.zeros((n, n)) if k == 0 else (P if k == N else Q)   # 0-based state stage
    zeta = np.zeros((n, N + 1))
    for k in range(N):
        zeta[:, k + 1] = A @ zeta[:, k] + B @ Z[:, k]
    mu, al = np.zeros((n, N + 1)), np.zeros((n, N + 1))
    mu[:, N] = g_x[:, N] + 2 * P @ zeta[:, N]
    al[:, N] = 2 * P @ ex[:, N]
    for k in range(N - 1, -1, -1):
        mu[:, k] = A.T @ mu[:, k + 1] + g_x[:, k] + 2 * Qbar(k) @ zeta[:, k]
        al[:, k] = A.T @ al[:, k + 1] + 2 * Qbar(k) @ ex[:, k]
    out = {"mu1": mu[:, 0].copy(), "f": Z.copy()}
    out["Q"] = sum((sym(zeta[:, k], ex[:, k]) for k in range(1, N)), np.zeros((n, n)))
    out["P"] = sym(zeta[:, N], ex[:, N])
    out["R"] = sum((sym(Z[:, k], v[:, k]) for k in range(N)), np.zeros((m, m))) if prob["useR"] else np.zeros((m, m))
    dz, du = Z[:, :-1] - Z[:, 1:], u[:, :-1] - u[:, 1:]
    out["S"] = sum((sym(dz[:, k], du[:, k]) for k in range(N - 1)), np.zeros((m, m))) if prob["useS"] else np.zeros((m, m))
    out["A"] = sum(np.outer(mu[:, k + 1], ex[:, k]) + np.outer(al[:, k + 1], zeta[:, k]) for k in range(N))
    out["B"] = sum(np.outer(mu[:, k + 1], v[:, k]) + np.outer(al[:, k + 1], Z[:, k]) for k in range(N))
    NU = nu.reshape(N, m).T
    ur = g_u - NU
    if prob["useS"]:
        Sd = 2 * (0.5 * (S + S.T)) @ dz                    # (m, N-1): 2 S (z_k - z_{k+1})
        ur[:, :-1] += Sd
        ur[:, 1:] -= Sd
    out["u_ref"] = ur
    L = lower.reshape(N, m).T
    Aw = act.reshape(N, m).T
    out["u_min"] = np.where(Aw & L, NU, 0.0).sum(axis=1)
    out["u_max"] = np.where(Aw & ~L, NU, 0.0).sum(axis=1)
    return out


def params_direct(prob, H, F, act, lower, res, g_u, g_x):
    """x0 is lam_1 + F'z (sens_ref.vjp_direct's expression); mu1, the recursion's first costate, is the same number."""
    lam1, q = sr.adjoint(prob["A"], prob["B"], g_u, g_x)
    z, nu = z_nu_direct(H, act, q)
    out = gradients(prob, act, lower, res, g_u, g_x, z, nu)
    out["x0"] = lam1 + F.T @ z
    return out


def params_gform(prob, ops, d, act, lower, res, g_u, g_x):
    """ops = sens_ref.g_operands(H, F, d); x0 is sens_ref.vjp_gform, the expression of almpc_sensitivity_vjp."""
    _, q = sr.adjoint(prob["A"], prob["B"], g_u, g_x)
    z, nu = z_nu_gform(ops[0], d, act, q)
    out = gradients(prob, act, lower, res, g_u, g_x, z, nu)
    out["x0"] = sr.vjp_gform(None, None, d, act, prob["A"], prob["B"], g_u, g_x, ops)
    return out


def prob_of(p):
    """The design data of an oracle MPCProblem, with the reference's [1,1] rule for R and S."""
    useR = bool(p.R[0, 0] != 0.0)
    return dict(A=p.A, B=p.B, Q=p.Q, P=p.P, S=p.S, useR=useR, useS=bool(useR and p.S[0, 0] != 0.0))


def group_scale(ref):
    return max(1.0, float(np.abs(ref).max()))


def worst_gaps(got, ref):
    """Per group, |got - ref|_max over max(1, max|ref group|) of one instance."""
    return {k: float(np.abs(np.asarray(got[k]) - np.asarray(ref[k])).max()) / group_scale(ref[k]) for k in GROUPS}
