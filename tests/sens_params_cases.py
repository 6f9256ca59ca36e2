"""The cases of the parameter-gradient tests (tests/test_sens_params_restatement.py on the oracle, tests/test_gpu_sensitivity_params.py
on the device).

  di        the double integrator, N = 10, batch 32: working sets of 0 .. 10 rows, 50 lower and 66 upper in total
  r326      a random stable (3, 2, 6) model, non-zero x_ref and u_ref, an asymmetric box, S = 0
  r326_s    the same with S != 0
  quad      the quadrotor at N = 30, quadrotor_x0_batch(16, amplitude 3): 2 .. 15 rows
  quad_big  the quadrotor at amplitude 10 (the large-working-set input of tests/test_gpu_sensitivity.py): instances beyond 32 rows
  r326_refs r326_s with one reference per instance (batch 19 on the device: a partial first-tier workgroup)
  quadfam   eight quadrotors with their own mass and inertia (test_gpu_batched_models.quad_family) at N = 10, each with its own DARE
            terminal weight: almpc_design_batched on the device

MEASURED_GAP[case] is the worst gap of the G form to the direct form on the oracle's solutions, over every output group and instance,
each group's error per instance over max(1, max|group|): the figures one run of tests/test_sens_params_restatement.py printed, which
holds every later run to them (within GAP_SLACK: they are sums of roundings and move with the BLAS underneath numpy).  The GPU
tolerance of a case is that gap times ten, the factor being for the device's own rounded G (the precedent of
tests/sens_rows_cases.py); it is not tuned against the device.
"""
import dataclasses

import numpy as np

GAP_SLACK = 4.0

R326_SEED = 11
R326_UMIN, R326_UMAX = np.array([-0.6, -1.0]), np.array([1.0, 0.4])

MEASURED_GAP = {"di": 4.9e-12, "r326": 1.7e-14, "r326_s": 7.7e-15, "quad": 1.2e-9, "quad_big": 3.0e-9, "r326_refs": 2.4e-14,
                "quadfam": 5.9e-13}


def gpu_tol(name):
    return 10.0 * MEASURED_GAP[name]


def r326(mo, s):
    rng = np.random.default_rng(R326_SEED)
    A = rng.standard_normal((3, 3))
    A *= 0.9 / np.max(np.abs(np.linalg.eigvals(A)))
    B = rng.standard_normal((3, 2))
    x_ref = 0.2 * rng.standard_normal(3)
    u_ref = np.array([0.1, -0.15])
    p = mo.make_problem(A, B, 6, R326_UMIN, R326_UMAX, x_ref=x_ref, u_ref=u_ref, s=s)
    X0 = np.logspace(-1.3, 0.8, 19)[(7 * np.arange(19)) % 19][:, None] * rng.standard_normal((19, 3))
    return p, X0


def r326_instance_refs(b=19):
    """Per-instance references of the r326_s device case: x_ref (b, 3, 7), u_ref (b, 2, 6), constant over the horizon."""
    rng = np.random.default_rng(R326_SEED + 1)
    xr = 0.2 * rng.standard_normal((b, 3, 1)) * np.ones((b, 3, 7))
    ur = 0.15 * rng.uniform(-1, 1, size=(b, 2, 1)) * np.ones((b, 2, 6))
    return xr, ur


def case(mo, name):
    """(problem, X0) of a case."""
    if name == "di":
        return mo.double_integrator(N=10), 3.0 * np.random.default_rng(7).normal(size=(32, 2))
    if name == "r326":
        return r326(mo, 0.0)
    if name == "r326_s":
        return r326(mo, 0.5)
    if name == "quad":
        return mo.quadrotor(N=30), mo.quadrotor_x0_batch(16, amplitude=3.0)
    if name == "quad_big":
        return mo.quadrotor(N=30), mo.quadrotor_x0_batch(16, amplitude=10.0)
    raise KeyError(name)


QUAD_UMIN, QUAD_UMAX = [-2.0, -0.05, -0.05, -0.02], [3.0, 0.05, 0.05, 0.02]


def quadfam(mo, b=8, N=10):
    """(A_i, B_i) of the family and the states: the inputs of tests/test_gpu_sensitivity.py::test_per_instance_models at batch 8."""
    from test_gpu_batched_models import quad_family
    As, Bs = quad_family(mo, b)
    return As, Bs, mo.quadrotor_x0_batch(b, 2.0, first_instance=5000)


def problems(mo, name):
    """(one problem per instance, X0): the shared problem of case() b times, or the per-instance ones."""
    if name == "r326_refs":
        p, X0 = r326(mo, 0.5)
        xr, ur = r326_instance_refs(len(X0))
        return [dataclasses.replace(p, x_ref=xr[i], u_ref=ur[i]) for i in range(len(X0))], X0
    if name == "quadfam":
        As, Bs, X0 = quadfam(mo)
        return [mo.make_problem(As[i], Bs[i], 10, QUAD_UMIN, QUAD_UMAX) for i in range(len(X0))], X0
    p, X0 = case(mo, name)
    return [p] * len(X0), X0


FD_CASES = ("di", "r326", "r326_s")
G_CASES = FD_CASES + ("quad", "quad_big", "r326_refs", "quadfam")


def loss(rng, p):
    return rng.normal(size=(p.m, p.N)), rng.normal(size=(p.n, p.N + 1))
