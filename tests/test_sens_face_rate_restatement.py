"""CPU: the restatement of the sensitivities on structured handles with an input-rate weight S (tests/sens_face_rate_ref.py: the
Riccati recursion on the face in the stage state [dx_k; du_(k-1)]) on the exact oracle's solutions of every instance of every case of
tests/sens_face_rate_cases.py.

  gap record            against the direct form (sens_ref.jac_direct / vjp_direct on the unscaled condensed H, F, which carry D'SD):
                        the worst gap of a case, Jacobians over max(1, max|J_i|) and VJPs over sens_ref.vjp_scale, must stay within
                        GAP_SLACK of the figure recorded in sens_face_rate_cases.GAP; ten times that figure is the case's tolerance
                        on the device.  dX is held against sens_ref.dx_from_du of the direct form's Jacobian in the same record
  central differences   du/dx0 against central differences of solve_mpc_exact's u (h = 1e-6) on two instances per case (the first and
                        the middle one), 1e-5 of max(1, max|J_i|)
  band condition        no input of the oracle's solutions lies between 1e-9 and 1e-5 of its box's width from a bound, so the active
                        set does not depend on the tolerance of the rule (1e-7)
  coverage              every case holds an instance with a clamped and a free row
  S = 0                 the restatement with S = 0 is that of tests/sens_face_ref.py to rounding
  surface               the header declares the four new symbols, the Julia shim and _capi bind them, Solver and Group carry the methods
"""
import os
import re

import numpy as np
import pytest

import mpc_oracle as mo
import sens_face_cases as fc0
import sens_face_rate_cases as fc
import sens_face_rate_ref as fr
import sens_face_ref as fr0
import sens_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("almpc_sensitivity_stagewise_rate", "almpc_sensitivity_stagewise_rate_vjp", "almpc_group_sensitivity_stagewise_rate",
           "almpc_group_sensitivity_stagewise_rate_vjp")


def _ops(p):
    return p.A, p.B, p.Q, p.R, p.S, p.P


@pytest.mark.parametrize("name", fc.NAMES)
def test_restatement_against_the_direct_form(name):
    U = fc.exact_inputs(name)
    g_u, g_x = fc.loss(name)
    gap_j = gap_v = 0.0
    rows = []
    for i in fc.instances(name):
        p = fc.problem_of(name, i)
        assert p.S[0, 0] != 0.0 and p.R[0, 0] != 0.0
        H, F = fc.condensed_of(name, i)
        act = fr.active_rows(U[i], p.u_min, p.u_max)
        rows.append(int(act.sum()))
        Jd = sr.jac_direct(H, F, act)
        J, dX = fr.jacobians(*_ops(p), act, p.N)
        gap_j = max(gap_j, np.abs(J - Jd).max() / max(1.0, np.abs(Jd).max()))
        dXd = sr.dx_from_du(p.A, p.B, Jd, p.N)
        gap_j = max(gap_j, np.abs(dX - dXd).max() / max(1.0, np.abs(dXd).max()))
        vd = sr.vjp_direct(H, F, act, p.A, p.B, g_u[i], g_x[i])
        v = fr.vjp(*_ops(p), act, g_u[i], g_x[i])
        gap_v = max(gap_v, np.abs(v - vd).max() / sr.vjp_scale(vd))
    print(f"{name}: rows {min(rows)} .. {max(rows)}; gap to the direct form: J {gap_j:.3e}, VJP {gap_v:.3e} "
          f"(recorded {fc.GAP[name]:g}, tolerance on the device {fc.gpu_tol(name):g})")
    assert max(gap_j, gap_v) <= fc.GAP_SLACK * fc.GAP[name]


@pytest.mark.parametrize("name", fc.NAMES)
def test_restatement_against_central_differences_of_the_oracle(name):
    _, X0, _ = fc.case(name)
    U = fc.exact_inputs(name)
    inst = fc.instances(name)
    worst = 0.0
    for i in (inst[0], inst[len(inst) // 2]):
        p = fc.problem_of(name, i)
        act = fr.active_rows(U[i], p.u_min, p.u_max)
        J, _ = fr.jacobians(*_ops(p), act, p.N)
        Jf = np.zeros_like(J)
        for c in range(p.n):
            e = np.zeros(p.n); e[c] = fc.FD_H
            hi, lo = mo.solve_mpc_exact(p, X0[i] + e), mo.solve_mpc_exact(p, X0[i] - e)
            Jf[:, c] = (hi["u"] - lo["u"]).T.reshape(-1) / (2 * fc.FD_H)
        worst = max(worst, np.abs(J - Jf).max() / max(1.0, np.abs(J).max()))
    print(f"{name}: worst gap to central differences {worst:.3e}")
    assert worst <= fc.FD_TOL


def test_band_condition_and_coverage():
    for name in fc.NAMES:
        _, X0, _ = fc.case(name)
        U = fc.exact_inputs(name)
        left = fc.LEFT_OUT.get(name, ())
        assert len(left) <= (2 if X0.shape[0] >= 19 else 0)
        nearest_free, most, clamped, free = np.inf, 0, False, False
        for i in fc.instances(name):
            p = fc.problem_of(name, i)
            dist = fr.distance_to_bounds(U[i], p.u_min, p.u_max)
            assert not np.any((dist > fc.BAND[0]) & (dist < fc.BAND[1])), (name, i, dist[(dist > fc.BAND[0]) & (dist < fc.BAND[1])])
            act = fr.active_rows(U[i], p.u_min, p.u_max)
            assert np.array_equal(act, (dist <= fc.BAND[0]).T.reshape(-1))
            nearest_free = min(nearest_free, dist[dist > fc.BAND[0]].min(initial=np.inf))
            clamped, free = clamped or bool(act.any()), free or not act.all()
            most = max(most, int(act.sum()))
        print(f"{name}: nearest free input at {nearest_free:.1e} of its width, working sets up to {most} rows")
        assert clamped and free, name


def test_the_case_table_is_the_one_the_tests_are_written_for():
    assert len(fc.NAMES) == 16 and set(fc.GAP) == set(fc.NAMES)
    dims = {name: (fc.problem_of(name, 0).n, fc.problem_of(name, 0).m) for name in fc.NAMES}
    nt = {k: n + m for k, (n, m) in dims.items()}
    assert nt["16-16-5-S"] ** 2 == 1024 and nt["30-7-6-S"] ** 2 > 1024 and nt["32-16-4-S"] == 48 and 16 * nt["32-16-4-S"] > 512
    assert dims["quad-50-S"] == (12, 4) and fc.problem_of("quad-50-S", 0).N == 50 and fc.problem_of("quad-50-S", 0).S[0, 0] == 0.05
    assert not fc.case("inst-5-3-12-S")[2] and nt["inst-5-3-12-S"] <= 16


def test_with_a_zero_rate_weight_the_restatement_is_the_old_one():
    name = "9-4-12"
    p = fc0.problem_of(name, 0)
    g_u, g_x = fc0.loss(name)
    U = fc0.exact_inputs(name)
    Z = np.zeros_like(p.S)
    worst = 0.0
    for i in (0, 7, 18):
        act = fr0.active_rows(U[i], p.u_min, p.u_max)
        J0, dX0 = fr0.jacobians(p.A, p.B, p.Q, p.R, p.P, act, p.N)
        J, dX = fr.jacobians(p.A, p.B, p.Q, p.R, Z, p.P, act, p.N)
        v0 = fr0.vjp(p.A, p.B, p.Q, p.R, p.P, act, g_u[i], g_x[i])
        v = fr.vjp(p.A, p.B, p.Q, p.R, Z, p.P, act, g_u[i], g_x[i])
        worst = max(worst, np.abs(J - J0).max() / max(1.0, np.abs(J0).max()), np.abs(dX - dX0).max() / max(1.0, np.abs(dX0).max()),
                    np.abs(v - v0).max() / sr.vjp_scale(v0))
    print(f"S = 0 on {name}: worst gap to sens_face_ref {worst:.3e}")
    assert worst <= fc0.GAP_SLACK * fc0.GAP[name]   # (both are the same recursion: they differ by less than either from the direct form)


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_capi_and_shim_carry_the_new_symbols(pkg):
    hdr = _read(ROOT, "include", "almpc.h")
    shim = _read(ROOT, "julia", "AlmpcHIP.jl")
    for s in SYMBOLS:
        assert re.search(r"^int %s\(" % s, hdr, re.M), s
        assert "(:%s, libalmpc)" % s in shim, s
        assert s in pkg._capi.prototypes(), s
    for cls in (pkg._capi.Solver, pkg._capi.Group):
        for nm in ("sensitivity_stagewise_rate", "sensitivity_stagewise_rate_vjp"):
            assert callable(getattr(cls, nm, None)), (cls.__name__, nm)
    for nm in ("sensitivity_stagewise_rate", "sensitivity_stagewise_rate_vjp", "group_sensitivity_stagewise_rate",
               "group_sensitivity_stagewise_rate_vjp"):
        assert re.search(r"^function %s\(" % nm, shim, re.M), nm
        assert re.search(r"\b%s\b" % nm, shim[shim.index("export"):shim.index("\n\n", shim.index("export"))]), nm
