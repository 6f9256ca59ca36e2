"""The cases of the per-instance-weight design (almpc_design_batched_weighted): one table for tests/test_weighted_design_cases.py (CPU:
the table's conditions against the oracle, the table against the source) and tests/test_gpu_weighted_design.py (GPU).

Shapes are rows of tests/instance_step_cases.py (imported, not edited): one per build of k_design_instance_t, one whose scaling is
k_design_scale's own launch (a design LDS below 128 doubles; and a second handle under ALMPC_DBG_SPLIT_SCALE where the table asks), one
on the dense route (k_design_blocks + k_design_gamma + k_design_hessian).  Models, references, the input box and the given terminal
weight are that table's; the weights are this one's:

    Q_i = diag(10^U(0, 3)) + a symmetric off-diagonal part whose absolute row sums stay below a tenth of the smallest diagonal entry
          (diagonally dominant with a positive diagonal: positive definite),
    R_i = diag(10^U(-2, 0)),   S_i = diag(10^U(-2, 0)) or absent -- the same choice for every instance of a case,

from a generator seeded by the shape.  Amplitudes of x0 were chosen on the CPU so that the exact solution of every instance has few
rows on a bound (MAX_ACTIVE) -- the stage-wise redo does not cover these designs, the condensed step has to solve every instance on
its own -- and, in the sensitivity cases, no input within (1e-9, 1e-5) of its width from a bound (the rule of
tests/sens_face_cases.py).  The CPU test asserts all of it.
"""
import copy
import functools

import numpy as np

import instance_step_cases as ic
import mpc_oracle as mo

BATCH = ic.BATCH
MAX_ACTIVE = 16                    # rows on a bound in the exact solution of any instance: half of the finish's first tier
SPLIT_SCALE = {"ALMPC_DBG_SPLIT_SCALE": "1"}
NEAR_BOUND = (1e-9, 1e-5)          # of the box's width: no input of a sensitivity case may lie in between


class WCase:
    """A row of instance_step_cases (base), with or without S_i, the amplitude of x0, and what the row is for."""

    def __init__(self, base, with_s, amp, envs=(), tags=()):
        self.base = ic.CASE_BY_ID[base]
        self.with_s, self.amp = with_s, amp
        self.envs = tuple(dict(e) for e in envs)
        self.tags = frozenset(tags)
        self.n, self.m, self.N = self.base.shape
        self.batch = self.base.batch
        self.id = base + ("-s" if with_s else "")

    shape = property(lambda s: (s.n, s.m, s.N))

    def __repr__(self):
        return self.id


CASES = (
    WCase("12-4-12", True, 2.0, tags=("sens",)),            # k_design_instance_t<12, 4>, the scaling in its tail
    WCase("4-2-16", False, 3.0, tags=("sens", "null_p")),   # <4, 2>
    WCase("2-1-17", True, 3.0, tags=("null_p",)),           # <2, 1>
    WCase("3-2-6", True, 2.0, envs=(SPLIT_SCALE,), tags=("sens", "fd", "null_p")),   # <0, 0>; the scaling split off by the switch
    WCase("1-1-1", False, 2.0),                             # <0, 0>, 12 doubles of design LDS: the scaling by k_design_scale
    WCase("16-1-59", False, 1.0),                           # the dense route
)
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES) and all(24 <= c.batch <= 48 for c in CASES)


def tagged(tag):
    return tuple(c for c in CASES if tag in c.tags)


def reached():
    """what the table reaches of the design's launcher: the k_design_instance_t builds, the routes, the homes of the scaling"""
    out = dict(design=set(), design_route=set(), scale_in_tail=set())
    for c in CASES:
        out["design_route"].add(ic.design_route(*c.shape))
        if ic.design_route(*c.shape) == "lds":
            out["design"].add(ic.design_build(c.n, c.m))
        for env in ({},) + c.envs:
            out["scale_in_tail"].add(ic.scale_in_tail(*c.shape, env))
    return out


def _weights(seed, batch, n, m, with_s):
    rng = np.random.default_rng(seed)
    Q = np.zeros((batch, n, n)); R = np.zeros((batch, m, m)); S = np.zeros((batch, m, m))
    for i in range(batch):
        dq = 10.0 ** rng.uniform(0.0, 3.0, n)
        off = rng.uniform(-1.0, 1.0, (n, n))
        off = 0.5 * (off + off.T)
        np.fill_diagonal(off, 0.0)
        Q[i] = np.diag(dq) + off * (0.1 * dq.min() / max(1, n - 1))
        R[i] = np.diag(10.0 ** rng.uniform(-2.0, 0.0, m))
        s = 10.0 ** rng.uniform(-2.0, 0.0, m)
        if with_s:
            S[i] = np.diag(s)
    for M in (Q, R, S):
        M.setflags(write=False)
    return Q, R, (S if with_s else None)


@functools.lru_cache(maxsize=None)
def weights(c):
    """(Q (batch, n, n), R (batch, m, m), S (batch, m, m) or None), read-only"""
    return _weights(77000 + 900 * c.n + 10 * c.m + c.N, c.batch, c.n, c.m, c.with_s)


@functools.lru_cache(maxsize=None)
def terminal(c):
    """the terminal weight given to the design: the base table's one matrix (n, n); in the sensitivity cases (batch, n, n), every
    instance's own P_i = DARE(A_i, B_i, Q_i, R_i) -- the problem a design with P = NULL has, so that almpc_sensitivity_params_vjp_dare
    is tested on a problem the CPU test has held to the table's conditions"""
    if "sens" not in c.tags:
        return ic.template(c.base).P
    Q, R, _ = weights(c)
    A, B = ic.models(c.base)
    P = np.stack([mo.dare(A[i], B[i], Q[i], R[i]) for i in range(c.batch)])
    P.setflags(write=False)
    return P


def problem_with(c, i, Q, R, S, P=None):
    """instance i's problem of the base table with the given weights (S None: zeros); P None: the table's terminal weight"""
    p = copy.copy(ic.problem(c.base, i))
    p.Q, p.R = np.array(Q), np.array(R)
    p.S = np.zeros((c.m, c.m)) if S is None else np.array(S)
    T = terminal(c)
    p.P = np.array(P if P is not None else T if T.ndim == 2 else T[i])
    return p


def problem(c, i):
    Q, R, S = weights(c)
    return problem_with(c, i, Q[i], R[i], None if S is None else S[i])


def x0(c):
    return ic.x0(c.base, c.amp)


@functools.lru_cache(maxsize=None)
def condensed(c):
    """[(H_i, F_i)] of every instance's own problem (mo.condense)"""
    return [mo.condense(problem(c, i))[2:4] for i in range(c.batch)]


def exact_of(p, x):
    H, f, lo, hi = mo.condensed_qp(p, x)
    return mo.rollout(p, x, mo.solve_box_qp_exact(H, f, lo, hi))


@functools.lru_cache(maxsize=None)
def reference(c):
    """dict(X0, exact: [rollout dict of the exact solution of instance i's own problem]) of EVERY instance, once per process"""
    X0 = x0(c)
    return dict(X0=X0, exact=[exact_of(problem(c, i), X0[i]) for i in range(c.batch)])


def bound_gaps(p, u):
    """distance of every input to its nearer bound over the box's width, (m, N)"""
    w = (p.u_max - p.u_min)[:, None]
    return np.minimum(u - p.u_min[:, None], p.u_max[:, None] - u) / w


def active_rows(p, u, tol=1e-9):
    return int((bound_gaps(p, u) <= tol).sum())


# ---------------------------------------------------------------------------- the parameter gradients
# worst gap of the G form (what the device computes) to the direct form of tests/sens_params_ref.py on the oracle's solutions of a
# sensitivity case, every group's error per instance over max(1, max|group|): the figures one run of
# tests/test_weighted_design_cases.py printed, which holds every later run to them within GAP_SLACK (the rule and the factor of
# tests/sens_params_cases.py).  The tolerance on the device is ten times the gap, for the device's own rounded G.
GAP_SLACK = 4.0
MEASURED_GAP = {"12-4-12-s": 1.3e-13, "4-2-16": 7.7e-14, "3-2-6-s": 3.4e-14}


def gpu_tol(cid):
    return 10.0 * MEASURED_GAP[cid]


def loss(c, seed=41):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(c.batch, c.m, c.N)), rng.normal(size=(c.batch, c.n, c.N + 1))


# ---------------------------------------------------------------------------- state rows
ROWS_BATCH, ROWS_N = 48, 10
ROWS_XMIN, ROWS_XMAX = np.array([-10.0, -0.8]), np.array([10.0, 0.8])
ROWS_CASES = ("box", "eq")


@functools.lru_cache(maxsize=None)
def rows_family():
    """the double-integrator family of tests/test_gpu_state_rows_instances.py (one sampling time per instance), weights of this table
    with S_i, and states from which every instance is feasible under the velocity box and under the terminal equality"""
    Ts = 0.5 + 0.02 * np.arange(ROWS_BATCH)
    A = np.stack([np.array([[1.0, t], [0.0, 1.0]]) for t in Ts])
    B = np.stack([np.array([[0.5 * t * t], [t]]) for t in Ts])
    Q, R, S = _weights(77123, ROWS_BATCH, 2, 1, True)
    X0 = mo.splitmix_normal(0x5EED0011, 0, ROWS_BATCH, 2) * np.array([1.0, 0.5])[None]
    X0[:, 1] = np.clip(X0[:, 1], -0.75, 0.75)
    return A, B, Q, R, S, X0


def rows_problem(case, i):
    A, B, Q, R, S, _ = rows_family()
    box = case == "box"
    p = mo.make_problem(A[i], B[i], ROWS_N, [-1.0], [1.0], x_min=ROWS_XMIN if box else None, x_max=ROWS_XMAX if box else None,
                        terminal="none" if box else "equality", P=np.eye(2))
    p.Q, p.R, p.S = np.array(Q[i]), np.array(R[i]), np.array(S[i])
    p.P = mo.dare(A[i], B[i], p.Q, p.R)     # (the design's P = NULL)
    return p


@functools.lru_cache(maxsize=None)
def rows_reference(case):
    """[exact solution with info] of every instance; raises where one is infeasible (the CPU test says none is)"""
    X0 = rows_family()[5]
    return [mo.solve_mpc_exact(rows_problem(case, i), X0[i], return_info=True) for i in range(ROWS_BATCH)]
