"""The cases of the structured-handle sensitivity tests (tests/test_sens_face_restatement.py on the oracle, tests/test_gpu_sens_face.py
on the device): input box, S = 0.

  table   the `ubox` cases of tests/stagewise_shape_cases.py without S (one per build of k_sdual and beyond), the first two tier cases
          (amplitude 10: working sets beyond 32 rows) and the two long horizons 17-1-63 and 13-5-127 (m N = 635); problem and X0 from
          stagewise_shape_cases.inputs, batch 37
  quad    the quadrotor at N = 30 (48 instances, amplitude 3: a condensed handle exists beside the structured one) and at N = 50
          (16 instances, amplitude 10: m N = 200, no condensed handle exists)
  inst    one model per instance: the family of test_structured_handle_with_per_instance_models_and_references, (5, 3, 12), batch 24

GAP[case] is the worst gap of the restatement (tests/sens_face_ref.py) to the direct form (tests/sens_ref.py jac_direct / vjp_direct)
on the exact oracle's solutions of every instance, Jacobians over max(1, max|J_i|) and VJPs over sens_ref.vjp_scale: the figures one
run of tests/test_sens_face_restatement.py printed, which holds every later run to them within GAP_SLACK (they are sums of roundings
and move with the BLAS underneath numpy).  The GPU tolerance of a case is ten times its gap and not below TOL_FLOOR: a recorded gap
of one rounding (1-1-1: 1.4e-16) must not make a tolerance that no other order of summation meets, and the floor covers the
reordering of a few hundred FP64 roundings.  It is not tuned against the device.  LEFT_OUT[case]: instances whose oracle solution has an input inside the band (BAND) where the
active-set rule would depend on the tolerance; none was found.
"""
import functools

import numpy as np

import mpc_oracle as mo
import stagewise_shape_cases as sc

GAP_SLACK = 4.0
TOL_FLOOR = 1e-13
BAND = (1e-9, 1e-5)     # no returned input may lie between these fractions of its box's width from a bound
FD_H, FD_TOL = 1e-6, 1e-5

_TABLE = ("1-1-1", "2-2-9", "4-1-11", "6-1-10", "7-3-10", "9-3-12", "9-4-12", "13-3-9", "16-4-8", "11-5-8", "16-8-6", "17-3-8", "20-9-6",
          "32-16-5")
_TIER = {"32-16-5-amp10": sc.TIER_CASES[0][0], "16-8-12-amp10": sc.TIER_CASES[1][0]}
_EDGE = {c.id[:-len("-ubox")]: c for c in sc.EDGE_CASES if c.id in ("17-1-63-ubox", "13-5-127-ubox")}
TIER_NAMES = tuple(_TIER)
NAMES = _TABLE + TIER_NAMES + tuple(_EDGE) + ("quad-30", "quad-50", "inst-5-3-12")

GAP = {"1-1-1": 1.4e-16, "2-2-9": 1.8e-14, "4-1-11": 2.4e-15, "6-1-10": 2.0e-15, "7-3-10": 1.3e-14, "9-3-12": 1.2e-14, "9-4-12": 7.6e-15,
       "13-3-9": 3.4e-15, "16-4-8": 7.5e-15, "11-5-8": 1.2e-14, "16-8-6": 3.7e-15, "17-3-8": 1.6e-15, "20-9-6": 3.8e-15,
       "32-16-5": 4.5e-15, "32-16-5-amp10": 1.6e-15, "16-8-12-amp10": 6.5e-15, "17-1-63": 1.5e-15, "13-5-127": 3.0e-14,
       "quad-30": 6.2e-11, "quad-50": 1.2e-9, "inst-5-3-12": 1.3e-13}
LEFT_OUT = {}


def gpu_tol(name):
    return max(10.0 * GAP[name], TOL_FLOOR)


def _table_case(name):
    if name in _TIER:
        return _TIER[name]
    if name in _EDGE:
        return _EDGE[name]
    c = sc.CASE_BY_ID[name + "-ubox"]
    assert not c.S
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """(problems, X0, shared): one problem for the whole batch (shared) or one per instance."""
    if name == "quad-30":
        return mo.quadrotor(N=30), mo.quadrotor_x0_batch(48, 3.0), True
    if name == "quad-50":
        return mo.quadrotor(N=50), mo.quadrotor_x0_batch(16, 10.0), True
    if name == "inst-5-3-12":
        rng = np.random.default_rng(5)
        b, n, m, N = 24, 5, 3, 12
        As, Bs = [], []
        for _ in range(b):
            A = rng.standard_normal((n, n)); A *= (0.7 + 0.6 * rng.random()) / np.max(np.abs(np.linalg.eigvals(A)))
            As.append(A); Bs.append(rng.standard_normal((n, m)))
        X0 = 2.0 * rng.standard_normal((b, n))
        x_ref = 0.2 * np.ones((n, N + 1)); u_ref = np.tile(np.linspace(-0.2, 0.2, N), (m, 1))
        return tuple(mo.make_problem(As[i], Bs[i], N, -np.ones(m), np.ones(m), x_ref=x_ref, u_ref=u_ref) for i in range(b)), X0, False
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
