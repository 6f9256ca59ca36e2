"""Shared definitions of the continuous-to-discrete tests (tests/test_c2d_host.py, tests/test_gpu_c2d.py).

c2d_ref      numpy restatement, line by line, of hm::c2d (csrc/almpc_host_math.h) -- and so of k_c2d (csrc/almpc_c2d.hip.h)
zoh_scipy    the truth: scipy.linalg.expm of the augmented matrix [A B; 0 0] Ts
models       the fixed generator of continuous-time test models
c2d_error    max|X - X_ref| / max(1, max|X_ref|), the larger of the values for A_d and B_d
TOL          1e-10: a numpy prototype of the algorithm measured at most 5.4e-13 against scipy on these inputs; the bound leaves about
             200 x for FMA contraction and scipy's own error"""
import numpy as np
import scipy.linalg as sla

K_TERMS, MAX_HALVINGS = 16, 60
TOL = 1e-10
SHAPES = [(1, 1), (2, 1), (4, 2), (12, 4), (16, 16), (17, 3), (32, 8), (33, 3), (64, 16)]
SAMPLE_TIMES = [0.05, 1.0, 5.0]
BATCH = 67


def c2d_ref(A, B, Ts):
    """(A_d, B_d, s), or None where hm::c2d returns status 1."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n = A.shape[0]
    cs = Ts * np.abs(A).sum(axis=0)
    if not np.all(np.isfinite(cs)):
        return None
    nrm = cs.max()
    s, h = 0, Ts
    while nrm > 0.5:
        s += 1
        if s > MAX_HALVINGS:
            return None
        nrm *= 0.5
        h *= 0.5
    X = h * A
    G = np.eye(n)
    for k in range(K_TERMS, 0, -1):
        G = np.eye(n) + (1.0 / (k + 1)) * (X @ G)
    Bd = h * (G @ B)
    Ad = np.eye(n) + X @ G
    for _ in range(s):
        Bd = Bd + Ad @ Bd
        Ad = Ad @ Ad
    if not (np.all(np.isfinite(Ad)) and np.all(np.isfinite(Bd))):
        return None
    return Ad, Bd, s


def zoh_scipy(A, B, Ts):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n, m = B.shape
    M = np.zeros((n + m, n + m))
    M[:n, :n] = A
    M[:n, n:] = B
    E = sla.expm(M * Ts)
    return E[:n, :n].copy(), E[:n, n:].copy()


def models(n, m, b=BATCH):
    rng = np.random.default_rng(2000 + n)
    A = rng.standard_normal((b, n, n)) / np.sqrt(n) * rng.uniform(0.3, 3.0, (b, 1, 1)) - rng.uniform(0.0, 2.0, (b, 1, 1)) * np.eye(n)
    B = rng.standard_normal((b, n, m))
    return A, B


def c2d_error(Ad, Bd, Ad_ref, Bd_ref):
    ea = np.abs(Ad - Ad_ref).max() / max(1.0, np.abs(Ad_ref).max())
    eb = np.abs(Bd - Bd_ref).max() / max(1.0, np.abs(Bd_ref).max())
    return max(ea, eb)


_truth = {}


def truth(n, m, Ts):
    """zoh_scipy of every model of models(n, m), computed once and shared (read-only)."""
    key = (n, m, Ts)
    if key not in _truth:
        A, B = models(n, m)
        out = [zoh_scipy(A[i], B[i], Ts) for i in range(A.shape[0])]
        Ad, Bd = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        Ad.setflags(write=False)
        Bd.setflags(write=False)
        _truth[key] = (Ad, Bd)
    return _truth[key]
