"""The cases of the structured-handle sensitivity tests with an input-rate weight S (tests/test_sens_face_rate_restatement.py on the
oracle, tests/test_gpu_sens_face_rate.py on the device): input box, S != 0.

  table   the twelve `-S-ubox` cases of tests/stagewise_shape_cases.CASES (s = 0.5; one per build of k_sdual that a stage state
          [e_k; v_(k-1)] reaches): 16-16-5 has nt^2 = 1024 exactly, 30-7-6 has nt = 37 (nt^2 = 1369 > 1024), 32-16-4 is the largest
          stage (nt = 48, m nt = 768 > 512), 1-1-5 the smallest; problem and X0 from stagewise_shape_cases.inputs, batch 37
  edge    30-2-63-S-ubox of EDGE_CASES: the horizon edge of the (32, 16) build, four instances
  quad    the quadrotor with s = 0.05 at N = 30 (48 instances, amplitude 3: a condensed handle exists beside the structured one) and
          at N = 50 (16 instances, amplitude 10: m N = 200, no condensed handle exists)
  inst    one model per instance: the family of sens_face_cases' inst-5-3-12 with s = 0.5, batch 24 (n + m = 8: a build of k_sdual
          that the suite runs with per-instance models already)

GAP[case] is the worst gap of the restatement (tests/sens_face_rate_ref.py) to the direct form (tests/sens_ref.py jac_direct /
vjp_direct on the unscaled condensed H, F, which carry D'SD) on the exact oracle's solutions of every instance, Jacobians over
max(1, max|J_i|) and VJPs over sens_ref.vjp_scale: the figures one run of tests/test_sens_face_rate_restatement.py printed, which
holds every later run to them within GAP_SLACK.  The GPU tolerance of a case is ten times its gap and not below TOL_FLOOR, as in
tests/sens_face_cases.py.  It is not tuned against the device.  LEFT_OUT[case]: instances whose oracle solution has an input inside
the band (BAND) where the active-set rule would depend on the tolerance; none was found.
"""
import functools

import numpy as np

import mpc_oracle as mo
import stagewise_shape_cases as sc
from sens_face_cases import BAND, FD_H, FD_TOL, GAP_SLACK, TOL_FLOOR   # noqa: F401

_TABLE = ("1-1-5-S", "2-1-7-S", "4-1-7-S", "4-2-9-S", "5-3-9-S", "4-4-6-S", "8-4-8-S", "12-4-8-S", "8-8-6-S", "16-16-5-S", "30-7-6-S",
          "32-16-4-S")
_EDGE = {"30-2-63-S": next(c for c in sc.EDGE_CASES if c.id == "30-2-63-S-ubox")}
QUAD_S, INST_S = 0.05, 0.5
NAMES = _TABLE + tuple(_EDGE) + ("quad-30-S", "quad-50-S", "inst-5-3-12-S")

GAP = {"1-1-5-S": 1.8e-15, "2-1-7-S": 8.9e-16, "4-1-7-S": 1.3e-15, "4-2-9-S": 4.0e-15, "5-3-9-S": 4.0e-15, "4-4-6-S": 5.2e-15,
       "8-4-8-S": 7.9e-15, "12-4-8-S": 3.8e-15, "8-8-6-S": 1.2e-14, "16-16-5-S": 9.9e-15, "30-7-6-S": 3.6e-15, "32-16-4-S": 2.3e-15,
       "30-2-63-S": 3.1e-15, "quad-30-S": 6.0e-11, "quad-50-S": 9.2e-10, "inst-5-3-12-S": 1.2e-13}
LEFT_OUT = {}


def gpu_tol(name):
    return max(10.0 * GAP[name], TOL_FLOOR)


def _table_case(name):
    if name in _EDGE:
        return _EDGE[name]
    c = sc.CASE_BY_ID[name + "-ubox"]
    assert c.S
    return c


def _quadrotor(N):
    box = mo.quadrotor(N=N)
    return mo.make_problem(*mo.quadrotor_model(), N, box.u_min, box.u_max, s=QUAD_S)


@functools.lru_cache(maxsize=None)
def case(name):
    """(problems, X0, shared): one problem for the whole batch (shared) or one per instance."""
    if name == "quad-30-S":
        return _quadrotor(30), mo.quadrotor_x0_batch(48, 3.0), True
    if name == "quad-50-S":
        return _quadrotor(50), mo.quadrotor_x0_batch(16, 10.0), True
    if name == "inst-5-3-12-S":
        rng = np.random.default_rng(5)
        b, n, m, N = 24, 5, 3, 12
        As, Bs = [], []
        for _ in range(b):
            A = rng.standard_normal((n, n)); A *= (0.7 + 0.6 * rng.random()) / np.max(np.abs(np.linalg.eigvals(A)))
            As.append(A); Bs.append(rng.standard_normal((n, m)))
        X0 = 2.0 * rng.standard_normal((b, n))
        x_ref = 0.2 * np.ones((n, N + 1)); u_ref = np.tile(np.linspace(-0.2, 0.2, N), (m, 1))
        return tuple(mo.make_problem(As[i], Bs[i], N, -np.ones(m), np.ones(m), x_ref=x_ref, u_ref=u_ref, s=INST_S) for i in range(b)), X0, False
    p, X0 = sc.inputs(_table_case(name))
    return p, X0, True


def problem_of(name, i):
    ps, _, shared = case(name)
    return ps if shared else ps[i]


def instances(name):
    """the instances of a case that take part (all but LEFT_OUT's)"""
    return [i for i in range(case(name)[1].shape[0]) if i not in LEFT_OUT.get(name, ())]


@functools.lru_cache(maxsize=None)
def condensed(name, i=0):
    """(H, F) of the (instance's) problem, unscaled: what sens_ref.jac_direct / vjp_direct read"""
    _, _, H, F = mo.condense(problem_of(name, i))
    return H, F


def condensed_of(name, i):
    return condensed(name, 0 if case(name)[2] else i)


@functools.lru_cache(maxsize=None)
def exact_inputs(name):
    """u (m, N) of the exact oracle for every instance of a case: computed once per process, read-only"""
    _, X0, _ = case(name)
    out = []
    for i in range(X0.shape[0]):
        u = mo.solve_mpc_exact(problem_of(name, i), X0[i])["u"]
        u.setflags(write=False)
        out.append(u)
    return tuple(out)


def loss(name, seed=11):
    """loss gradients g_u (b, m, N), g_x (b, n, N+1) of a case: unit normal"""
    ps, X0, shared = case(name)
    p = ps if shared else ps[0]
    rng = np.random.default_rng(seed)
    return rng.normal(size=(X0.shape[0], p.m, p.N)), rng.normal(size=(X0.shape[0], p.n, p.N + 1))
