"""The cases of the rows-form sensitivity tests (tests/test_sens_rows_restatement.py on the oracle, tests/test_gpu_sensitivity_rows.py on
the device): the smallest shapes that reach each code path of k_sens<.., .., true>.

  di_box / di_eq / di_both   (2,1,10): Rs = 128, a partial last workgroup (batch 19), projection with ne = n
  r637_box / r637_both       (6,3,7):  nz = 21 <= 32, no second-tier launch; ne = 6
  r3233_box / r3233_both     (3,2,33): R = 165 -> Rs = 256, nz > 32
  quad_box / quad_both       quadrotor N = 30: Rs = 512, working sets beyond 32 rows (second tier); with the equality once projected
                             and once under ALMPC_NO_EQ_PROJECTION

MEASURED_GAP[case] is the worst gap of the G form and the projected G form to the direct KKT form on the oracle's solutions, Jacobians
over max(1, max|J|) and VJPs over max(1, max|g_x0|): the figures one run of tests/test_sens_rows_restatement.py printed, which holds
every later run to them (within GAP_SLACK: they are sums of roundings and move with the BLAS underneath numpy).  The GPU tolerance of
a case is that gap times ten, the factor being for the device's own G and Ghat; it is not tuned against the device.
"""
import dataclasses

import numpy as np

QUAD_BOX = 3.0 * np.array([1, 1, 1, .5, .5, .5, .1, .1, .1, .1, .1, .1])

MEASURED_GAP = {"di_box": 4.6e-13, "di_eq": 4.8e-13, "di_both": 4.8e-13, "r637_box": 8.5e-15, "r637_both": 8.1e-15,
                "r3233_box": 5.7e-15, "r3233_both": 6.4e-15, "quad_box": 3.5e-11, "quad_both": 3.9e-11}
GAP_SLACK = 4.0   # what a later CPU run may exceed the recorded gap by


def gpu_tol(name):
    return 10.0 * MEASURED_GAP[name]


def random_stable(mo, n, m, N, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    A *= 0.9 / np.max(np.abs(np.linalg.eigvals(A)))
    return mo.make_problem(A, rng.standard_normal((n, m)), N, -np.ones(m), np.ones(m))


def _inside_x0(n):
    # inside the box +-0.5 at stage 1 (a state outside it is infeasible at once), wide enough that some instances meet the box later
    return np.clip(0.6 * np.random.default_rng(n).normal(size=(24, n)), -0.49, 0.49)


def _with(p, box=None, eq=False):
    lo, hi = (None, None) if box is None else (np.asarray(box[0], float), np.asarray(box[1], float))
    return dataclasses.replace(p, x_min=lo, x_max=hi, terminal="equality" if eq else "none")


def case(mo, name):
    """(problem, X0) of a case."""
    kind, variant = name.split("_")
    box_on, eq_on = variant in ("box", "both"), variant in ("eq", "both")
    if kind == "di":
        p = mo.double_integrator(N=10)
        X0 = 3.0 * np.random.default_rng(7).normal(size=(19, 2))
        X0[:, 1] = np.clip(X0[:, 1], -0.75, 0.75)
        if eq_on:
            X0 = 0.5 * X0
        box = ([-10.0, -0.8], [10.0, 0.8])
    elif kind in ("r637", "r3233"):
        n, m, N = (6, 3, 7) if kind == "r637" else (3, 2, 33)
        p = random_stable(mo, n, m, N, 100 + n)
        X0 = _inside_x0(n)
        box = (-0.5 * np.ones(n), 0.5 * np.ones(n))
    elif kind == "quad":
        p = mo.quadrotor(N=30)
        X0 = np.clip(mo.quadrotor_x0_batch(32, 1.0, first_instance=900), -0.99 * QUAD_BOX, 0.99 * QUAD_BOX)
        box = (-QUAD_BOX, QUAD_BOX)
    else:
        raise KeyError(name)
    return _with(p, box if box_on else None, eq_on), X0


DI_CASES = ("di_box", "di_eq", "di_both")
GPU_CASES = DI_CASES + ("r637_box", "r637_both", "r3233_box", "r3233_both", "quad_box", "quad_both")
