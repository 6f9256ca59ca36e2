"""numpy restatement of k_ltv_stage_prepare (csrc/almpc_ltv_stage.hip.h): the vectors the stage-wise solvers read from a caller's
trajectory, in the order of operations of the two host loops of almpc_design_ltv (csrc/almpc_api.hip) -- plain Python sums over the
second index of the symmetrised weight, the R term first, then the rate pair (k-1, k) with -, then the pair (k, k+1) with +.

prepare(...) takes one instance in the binding's shapes (xbar (n, N+1), ubar (m, N), x_ref (n, N+1) / u_ref (m, N) or None) and returns
    ebar (N, n)   xbar_{k+1} - x_ref_{k+1}
    qadd (N, m)   2 Rbar (ubar - u_ref) + 2 D'Sbar D ubar, with the branch rules (R[0,0] == 0 drops both, S[0,0] == 0 the rate term)
    eqt  (n,)     x_ref_N, the terminal-equality target in absolute coordinates
    mag  (N, m)   sum of the absolute values of qadd's terms: the scale of its rounding bound
"""
import numpy as np


def prepare(xbar, ubar, x_ref, u_ref, R, S):
    xbar, ubar = np.asarray(xbar, dtype=np.float64), np.asarray(ubar, dtype=np.float64)
    n, N1 = xbar.shape
    N = N1 - 1
    m = ubar.shape[0]
    xr = np.zeros((n, N + 1)) if x_ref is None else np.asarray(x_ref, dtype=np.float64)
    ur = np.zeros((m, N)) if u_ref is None else np.asarray(u_ref, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    S = np.zeros((m, m)) if S is None else np.asarray(S, dtype=np.float64)
    Rs, Ss = 0.5 * (R + R.T), 0.5 * (S + S.T)
    useR = R[0, 0] != 0.0
    useS = useR and S[0, 0] != 0.0
    ebar = np.empty((N, n))
    for k in range(N):
        for j in range(n):
            ebar[k, j] = xbar[j, k + 1] - xr[j, k + 1]
    qadd = np.zeros((N, m)); mag = np.zeros((N, m))
    if useR:
        for k in range(N):
            for a in range(m):
                sr = 0.0; sa = 0.0
                for c in range(m):
                    t = Rs[c, a] * (ubar[c, k] - ur[c, k])
                    sr += t; sa += abs(t)
                qadd[k, a] += 2.0 * sr; mag[k, a] += 2.0 * sa
    if useS:
        for k in range(N - 1):
            for a in range(m):
                sd = 0.0; sa = 0.0
                for c in range(m):
                    t = Ss[c, a] * (ubar[c, k] - ubar[c, k + 1])
                    sd += t; sa += abs(t)
                qadd[k, a] += 2.0 * sd; qadd[k + 1, a] -= 2.0 * sd
                mag[k, a] += 2.0 * sa; mag[k + 1, a] += 2.0 * sa
    return dict(ebar=ebar, qadd=qadd, eqt=xr[:, N].copy(), mag=mag)
