"""The restatement of the sensitivities of a time-varying design (tests/sens_ltv_ref.py: the Riccati recursion on the face with the stage
models) against the direct form on the design's own QP (mo.ltv_qp: dv_f/dp = -H_ff^-1 F_f, F = 2 Gam' Qbar Phi), on the CPU, on the
exact oracle's solution of every instance of every case of tests/sens_ltv_cases.py, within GAP_SLACK of the recorded gaps; the VJP
against the Jacobians; time-invariant stages against tests/sens_face_ref.py and tests/sens_face_rate_ref.py; and the premises the GPU
test leans on: no oracle solution has an input inside the band where the active-set rule would depend on its tolerance, the table holds
free and held rows, and the finite-difference test's instances keep their active set at +-h.  Also: the header declares the entry
points and the Python binding and the Julia shim have them."""
import os
import re

import numpy as np
import pytest

import mpc_oracle as mo
import sens_face_rate_ref as rr
import sens_face_ref as fr
import sens_ltv_cases as tc
import sens_ltv_ref as tr
import sens_ref as sr
from conftest import ROOT

SYMBOLS = ("almpc_sensitivity_ltv", "almpc_sensitivity_ltv_vjp")
ALL_HELD = {"2-1-N1-b4", "2-1-N2-b4"}               # (and their -s0 twins) the cases without a free row
FD_CASES = ("4-3-N7-b4", "12-4-N3-b4")              # tests/test_gpu_sens_ltv.py::test_finite_differences_of_the_device_solution


def _act(name, i):
    a = tc.inputs(name)
    return tr.active_rows(tc.qp(name, i)["u"], a["umin"], a["umax"])


def test_table_and_left_out_stay_within_their_caps():
    assert set(tc.GAP) == set(tc.ALL_NAMES)
    assert all(len(v) <= tc.LEFT_OUT_CAP[0] for v in tc.LEFT_OUT.values()) and sum(len(v) for v in tc.LEFT_OUT.values()) <= tc.LEFT_OUT_CAP[1]
    assert set(tc.LEFT_OUT) <= set(tc.NAMES) and set(tc.SEED) <= {n for n in tc.NAMES if n.endswith(tc.S0)}
    for name in tc.ALL_NAMES:
        useR, useS = tr.branch(tc.inputs(name)["R"], tc.inputs(name)["S"])
        if name.endswith(tc.S0):
            assert not useS, name
    assert sum(tr.branch(tc.inputs(n)["R"], tc.inputs(n)["S"])[1] for n in tc.NAMES) == 18   # (20 less -plain and -r0)


@pytest.mark.parametrize("name", tc.ALL_NAMES)
def test_no_oracle_solution_is_in_the_band(name):
    """... and the batch holds free and held rows (the all-held instances apart)"""
    a = tc.inputs(name)
    nearest, held, free = np.inf, 0, 0
    for i in range(tc.BATCH):
        u = tc.qp(name, i)["u"]
        band = tc.in_band(u, a["umin"], a["umax"])
        if i in tc.LEFT_OUT.get(name, ()):
            assert band.size, (name, i, "listed in LEFT_OUT without a reason")
            continue
        assert not band.size, (name, i, band)
        dist = tr.distance_to_bounds(u, a["umin"], a["umax"])
        act = _act(name, i)
        if (~act).any():
            nearest = min(nearest, float(dist.T.reshape(-1)[~act].min()))
        held += int(act.sum()); free += int((~act).sum())
    print(f"{name}: held {held}, free {free}, nearest free row {nearest:.2e} of the box width")
    assert held > 0 and (free > 0 or tc.base(name) in ALL_HELD)
    assert nearest >= 1.5e-4   # (1.59e-4 at 4-4-N32-b4: fifteen times the band's upper edge)


@pytest.mark.parametrize("name", tc.ALL_NAMES)
def test_recursion_equals_the_direct_form(name):
    n, m, N = tc.shape(name)
    g_u, g_x = tc.loss(name)
    gap = 0.0
    for i in tc.instances(name):
        k, _ = tc.instance(name, i)
        act = _act(name, i)
        J, dX = tr.jacobians(act=act, **k)
        Jd, dXd = tc.direct(name, i, act)
        sj, sx = max(1.0, np.abs(Jd).max()), max(1.0, np.abs(dXd).max())
        gap = max(gap, np.abs(J - Jd).max() / sj, np.abs(dX - dXd).max() / sx)
        assert np.array_equal(dX[:, 0, :], np.eye(n)) and not J[act].any()
        if act.all():
            assert not J.any()   # (dX is then the free response A_{k-1} ... A_0)
        # the VJP: against the direct Jacobians and against its own
        K0d, dUd = sr.shaped(Jd, m, N)
        ref = sr.vjp_from_jacobians(dUd, dXd, g_u[i], g_x[i])
        got = tr.vjp(act=act, g_u=g_u[i], g_x=g_x[i], **k)
        own = sr.vjp_from_jacobians(sr.shaped(J, m, N)[1], dX, g_u[i], g_x[i])
        scale = sr.vjp_scale(ref)
        gap = max(gap, np.abs(got - ref).max() / scale)
        assert np.abs(got - own).max() / scale <= max(tc.GAP_SLACK * tc.GAP[name], tc.TOL_FLOOR), (name, i)
    print(f"{name}: gap {gap:.1e} (recorded {tc.GAP[name]:.1e})")
    assert gap <= tc.GAP_SLACK * tc.GAP[name], (name, gap, tc.GAP[name])


@pytest.mark.parametrize("name", tc.NAMES)
def test_time_invariant_stages_give_the_recursions_of_the_structured_handles(name):
    """A_k = A, B_k = B: sens_face_ref without the rate term, sens_face_rate_ref with it -- the same operations in the same order."""
    n, m, N = tc.shape(name)
    g_u, g_x = tc.loss(name)
    for i in range(tc.BATCH):
        k, _ = tc.instance(name, i)
        act = _act(name, i)
        A, B = k["A"][N // 2], k["B"][N // 2]
        kk = dict(k, A=np.broadcast_to(A, (N, n, n)), B=np.broadcast_to(B, (N, n, m)))
        J, dX = tr.jacobians(act=act, **kk)
        g = tr.vjp(act=act, g_u=g_u[i], g_x=g_x[i], **kk)
        if tr.branch(k["R"], k["S"])[1]:
            Jr, dXr = rr.jacobians(A, B, k["Q"], k["R"], k["S"], k["P"], act, N)
            gr = rr.vjp(A, B, k["Q"], k["R"], k["S"], k["P"], act, g_u[i], g_x[i])
        else:
            Jr, dXr = fr.jacobians(A, B, k["Q"], k["R"], k["P"], act, N)
            gr = fr.vjp(A, B, k["Q"], k["R"], k["P"], act, g_u[i], g_x[i])
        assert np.array_equal(J, Jr) and np.array_equal(dX, dXr) and np.array_equal(g, gr), (name, i)


@pytest.mark.parametrize("name", FD_CASES)
def test_the_finite_difference_instances_keep_their_active_set(name):
    """dx_0 = p is the same QP as c_0 <- c_0 + A_0 p: at p = +-FD_H e_j the oracle's active set of every instance is the one at p = 0,
    and the central difference of its optimum is the restatement's column j."""
    n, m, N = tc.shape(name)
    a = tc.inputs(name)
    worst = 0.0
    for i in range(tc.BATCH):
        k, _ = tc.instance(name, i)
        act = _act(name, i)
        J, _ = tr.jacobians(act=act, **k)
        for j in range(n):
            us = []
            for sgn in (1.0, -1.0):
                c = a["c_all"][i].copy()
                c[0] += sgn * tc.FD_H * k["A"][0][:, j]
                H, q, lo, hi = mo.ltv_qp(k["A"], k["B"], c, a["xbar"][i], a["ubar"][i], a["x_ref"], a["u_ref"], k["Q"], k["R"],
                                         np.zeros((m, m)) if k["S"] is None else k["S"], k["P"], a["umin"], a["umax"])
                u = a["ubar"][i] + mo.solve_box_qp_exact(H, q, lo, hi).reshape(N, m).T
                assert np.array_equal(tr.active_rows(u, a["umin"], a["umax"]), act), (name, i, j, sgn)
                us.append(u.T.reshape(-1))
            fd = (us[0] - us[1]) / (2.0 * tc.FD_H)
            worst = max(worst, np.abs(fd - J[:, j]).max() / max(1.0, np.abs(J).max()))
    print(f"{name}: central differences of the oracle against the restatement {worst:.2e} (FD_TOL {tc.FD_TOL:g})")
    assert worst <= tc.FD_TOL


def test_header_declares_the_entry_points_and_the_bindings_have_them(pkg):
    with open(os.path.join(ROOT, "include", "almpc.h")) as f:
        header = f.read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert not re.search(r"\bint %s\(" % s.replace("almpc_", "almpc_group_"), header), s   # (almpc_design_ltv has no group form)
    capi = pkg._capi
    with open(os.path.join(ROOT, "julia", "AlmpcHIP.jl")) as f:
        shim = f.read()
    for s in SYMBOLS:
        assert s in capi.prototypes(), s
        assert "(:%s, libalmpc)" % s in shim, s
    for nm in ("sensitivity_ltv", "sensitivity_ltv_vjp"):
        assert callable(getattr(capi.Solver, nm)), nm
        assert not hasattr(capi.Group, nm), nm
        assert nm in shim
