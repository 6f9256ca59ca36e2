"""The cases of the sensitivities of a time-varying design (k_sens_ltv), one table for tests/test_sens_ltv_restatement.py (CPU) and
tests/test_gpu_sens_ltv.py (GPU), batch 4 throughout:

  the twenty cases of tests/cert_ltv_cases.py as they stand (N = 1, 2, 3, m N = 128, 16-3-4, 16-1-59 with footprint 1020 of 1024,
  R[0,0] = 0, one P per instance, the <12, 4> builds at N = 1, 2, 3), and each of them again with S = None (suffix -s0), so that both
  RATE builds of the kernel see every shape.  (4-3-N7-b4-plain has no S and 4-2-3-r0 drops it with R: their -s0 twins run the same
  build on the same data.)

Checked on the CPU (tests/test_sens_ltv_restatement.py) on the exact optima of the design's QP (mo.ltv_qp, mo.solve_box_qp_exact): no
free row lies inside sens_face_cases.BAND = (1e-9, 1e-5) of the box width from a bound -- the nearest is 1.59e-4 (4-4-N32-b4) for the
twenty as they stand and 2.1e-4 (5-3-N42-b4-s0) for the variants --, so the active-set rule does not depend on its tolerance.  An
instance in the band would be listed in LEFT_OUT with the reason, at most one per case and four in all (LEFT_OUT_CAP); beyond that
the variant's seed changes (SEED), not the cap.  None was found.  Every case but 2-1-N1 and 2-1-N2 (and their twins) has both free
and held rows; those two, and single instances of 2-1-N3 (0, 2), 4-2-3-r0 (1, 3) and 4-2-3-uref (3), hold every row.  They stay in:
their du/dp is zero and their dx/dp is the free response A_{k-1} ... A_0.

TI_NAMES: six time-invariant twins for the test that is independent of the recursion -- (4, 3, 7), (12, 4, 3) and (6, 1, 5) with one P
per instance, with and without S: instance i of the base case with A_k = A_i,0, B_k = B_i,0, xbar = x0_i repeated, ubar = 0, the defects
of that trajectory c_k = (A_i - I) x0_i and no references.  Then x_k = x0_i + dx_k obeys x_{k+1} = A_i x_k + B_i u_k: the
time-invariant problem (A_i, B_i) from x0_i, which almpc_design_batched solves on a structured handle (structured_twin), and the two
handles hold the same face.  (With c = 0 and references they would not: a time-invariant design propagates the deviation
e_{k+1} = A e_k + B v from e_0 = x0 - x_ref_0 and tracks no state reference as a trajectory, so its QP is that of an LTV design only
where the trajectory's defects are given and the references vanish.)  The twins pass the same band check and have gaps of their own.

GAP[case] is the worst gap of the restatement (tests/sens_ltv_ref.py: the recursion) to the direct form (jac_direct) on the oracle's
solutions of every instance, Jacobians over max(1, max|J_i|) and VJPs over sens_ref.vjp_scale: the figures one run of
tests/test_sens_ltv_restatement.py printed, which holds every later run to them within GAP_SLACK.  The GPU tolerance of a case is
max(10 GAP, 1e-13), the rule of sens_face_cases.py; it is not tuned against the device.
"""
import dataclasses
import functools

import numpy as np

import cert_ltv_cases as lc
import mpc_oracle as mo
import nlp_shape_cases as nc
import sens_ltv_ref as tr
from sens_face_cases import BAND, FD_H, FD_TOL, GAP_SLACK, TOL_FLOOR   # noqa: F401

BATCH = 4
S0 = "-s0"
NAMES = lc.NAMES + tuple(name + S0 for name in lc.NAMES)
assert len(NAMES) == 40
TI_BASES = ("4-3-N7-b4", "12-4-N3-b4", "6-1-N5-b4-pinst")
TI_NAMES = tuple("ti-" + b for b in TI_BASES) + tuple("ti-" + b + S0 for b in TI_BASES)
ALL_NAMES = NAMES + TI_NAMES

SEED = {}            # {variant: seed of nlp_shape_cases.Case} where the base case's own seed left an instance in the band
LEFT_OUT = {}        # {case: (instance, ...)} with the reason beside it
LEFT_OUT_CAP = (1, 4)   # per case, in all

GAP = {
    "2-1-N1-b4": 1.1e-16, "2-1-N2-b4": 1.8e-16, "2-1-N3-b4": 3.3e-16, "2-4-N32-b4": 1.0e-14,
    "4-2-N3-b4": 1.6e-16, "4-4-N32-b4": 6.4e-14, "4-3-N7-b4": 2.9e-15, "6-8-N16-b4": 4.4e-14,
    "6-1-N5-b4": 3.2e-16, "12-4-N1-b4": 3.5e-16, "12-4-N2-b4": 4.8e-16, "12-4-N3-b4": 3.5e-16,
    "5-3-N42-b4": 1.3e-14, "7-2-N64-b4": 4.1e-15, "4-3-N7-b4-plain": 3.1e-15, "6-1-N5-b4-pinst": 4.0e-16,
    "16-3-4": 5.5e-16, "16-1-59": 3.5e-15, "4-2-3-r0": 4.0e-16, "4-2-3-uref": 3.9e-16,
    "2-1-N1-b4-s0": 1.1e-16, "2-1-N2-b4-s0": 1.8e-16, "2-1-N3-b4-s0": 3.3e-16, "2-4-N32-b4-s0": 1.6e-14,
    "4-2-N3-b4-s0": 3.3e-16, "4-4-N32-b4-s0": 4.1e-14, "4-3-N7-b4-s0": 3.1e-15, "6-8-N16-b4-s0": 5.9e-14,
    "6-1-N5-b4-s0": 4.8e-16, "12-4-N1-b4-s0": 3.5e-16, "12-4-N2-b4-s0": 2.9e-16, "12-4-N3-b4-s0": 6.2e-16,
    "5-3-N42-b4-s0": 9.8e-15, "7-2-N64-b4-s0": 3.7e-15, "4-3-N7-b4-plain-s0": 3.1e-15, "6-1-N5-b4-pinst-s0": 4.5e-16,
    "16-3-4-s0": 6.7e-16, "16-1-59-s0": 2.1e-15, "4-2-3-r0-s0": 4.0e-16, "4-2-3-uref-s0": 4.4e-16,
    "ti-4-3-N7-b4": 2.2e-15, "ti-12-4-N3-b4": 1.1e-15, "ti-6-1-N5-b4-pinst": 5.1e-16,
    "ti-4-3-N7-b4-s0": 2.7e-15, "ti-12-4-N3-b4-s0": 1.1e-15, "ti-6-1-N5-b4-pinst-s0": 5.0e-16,
}


def gpu_tol(name):
    return max(10.0 * GAP[name], TOL_FLOOR)


def base(name):
    """the case of tests/cert_ltv_cases.py a case is made from"""
    name = name[len("ti-"):] if name.startswith("ti-") else name
    return name[:-len(S0)] if name.endswith(S0) else name


def shape(name):
    return lc.shape(base(name))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict of design_ltv's arguments, read-only: cert_ltv_cases.inputs, for a -s0 variant with S = None (and the seed of SEED)"""
    if name.startswith("ti-"):
        a = dict(inputs(name[len("ti-"):]))
        b, N = a["A_all"].shape[:2]
        a["A_all"] = np.repeat(a["A_all"][:, :1], N, axis=1)
        a["B_all"] = np.repeat(a["B_all"][:, :1], N, axis=1)
        x0 = a["xbar"][:, :, 0]
        a["c_all"] = np.repeat((np.einsum("bij,bj->bi", a["A_all"][:, 0], x0) - x0)[:, None, :], N, axis=1)
        a["xbar"] = np.repeat(x0[:, :, None], N + 1, axis=2)
        a["ubar"] = np.zeros_like(a["ubar"])
        a["x_ref"] = a["u_ref"] = None
        return a
    if not name.endswith(S0):
        return lc.inputs(name)
    if name in SEED:
        b = base(name)
        assert b in lc._BASE, "a seed of its own is for a case made by ltv_inputs alone"
        a = dict(nc.ltv_inputs(dataclasses.replace(lc._BASE[b], seed=SEED[name])))
    else:
        a = dict(lc.inputs(base(name)))
    a["S"] = None
    return a


def instance(name, i):
    """dict(A, B, Q, R, S, P, umin, umax) of instance i -- what tests/sens_ltv_ref.py reads -- and the whole argument set"""
    a = inputs(name)
    P = a["P"][i] if a["P"].ndim == 3 else a["P"]
    return dict(A=a["A_all"][i], B=a["B_all"][i], Q=a["Q"], R=a["R"], S=a["S"], P=P), a


@functools.lru_cache(maxsize=None)
def qp(name, i):
    """dict(H, q, lo, hi, Gam, g, v, u) of instance i: mo.ltv_qp with the prediction, its exact optimum v* and u* = ubar + v* (m, N)"""
    if name in lc.NAMES:
        p = dict(lc.qp(name, i))
    else:
        k, a = instance(name, i)
        m = a["ubar"].shape[1]
        c = None if a["c_all"] is None else a["c_all"][i]
        H, q, lo, hi, Gam, g = mo.ltv_qp(k["A"], k["B"], c, a["xbar"][i], a["ubar"][i], a["x_ref"], a["u_ref"], k["Q"], k["R"], np.zeros((m, m)) if k["S"] is None else k["S"],
                                         k["P"], a["umin"], a["umax"], return_prediction=True)
        p = dict(H=H, q=q, lo=lo, hi=hi, Gam=Gam, g=g, v=mo.solve_box_qp_exact(H, q, lo, hi))
    ubar = inputs(name)["ubar"][i]
    m, N = ubar.shape
    p["u"] = ubar + p["v"].reshape(N, m).T
    return p


def instances(name):
    """the instances of a case that take part (all but LEFT_OUT's)"""
    return [i for i in range(BATCH) if i not in LEFT_OUT.get(name, ())]


def in_band(u, umin, umax):
    """the distances (in box widths) of the inputs u (m, N) that lie inside BAND"""
    dist = tr.distance_to_bounds(u, umin, umax)
    return dist[(dist > BAND[0]) & (dist < BAND[1])]


def loss(name, seed=11):
    """loss gradients g_u (b, m, N), g_x (b, n, N+1) of a case: unit normal"""
    n, m, N = shape(name)
    rng = np.random.default_rng(seed)
    return rng.normal(size=(BATCH, m, N)), rng.normal(size=(BATCH, n, N + 1))


def direct(name, i, act):
    """(J, dX) of the direct form of instance i on the face `act`"""
    k, _ = instance(name, i)
    p = qp(name, i)
    return tr.jac_direct(k["A"], k["B"], k["Q"], k["P"], p["H"], p["Gam"], act)


def structured_twin(name):
    """the arguments of a "ti-" case as a per-instance time-invariant design of a structured handle takes them:
    dict(A (b, n, n), B (b, n, m), Q, R, S, P, umin, umax, X0 (b, n)); the references are zero"""
    assert name.startswith("ti-")
    a = inputs(name)
    return dict(A=a["A_all"][:, 0], B=a["B_all"][:, 0], Q=a["Q"], R=a["R"], S=a["S"], P=a["P"], umin=a["umin"], umax=a["umax"],
                X0=np.ascontiguousarray(a["xbar"][:, :, 0]))
