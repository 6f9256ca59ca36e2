"""CPU: the restatement of the sensitivities on structured handles (tests/sens_face_ref.py: the Riccati recursion on the face) on
the exact oracle's solutions of every instance of every case of tests/sens_face_cases.py.

  gap record            against the direct form (sens_ref.jac_direct / vjp_direct on the unscaled condensed H, F): the worst gap of a
                        case, Jacobians over max(1, max|J_i|) and VJPs over sens_ref.vjp_scale, must stay within GAP_SLACK of the
                        figure recorded in sens_face_cases.GAP; ten times that figure is the case's tolerance on the device
  central differences   du/dx0 against central differences of solve_mpc_exact's u (h = 1e-6) on two instances per case (the first and
                        the middle one), 1e-5 of max(1, max|J_i|); worst seen 1.7e-6, on the quadrotor at N = 50, where the oracle's
                        own u carries 1e-12.  (Differences of the oracle's x are no reference for dX there: x is u rolled out
                        through an open-loop unstable model, and they miss dX by 4.5e-5; dX is held against the rollout of the
                        direct form's Jacobian in the gap record.)
  band condition        no input of the oracle's solutions lies between 1e-9 and 1e-5 of its box's width from a bound, so the active
                        set does not depend on the tolerance of the rule (1e-7)
  coverage              every case holds an instance with a clamped and a free row; the tier cases one beyond 32 clamped rows
"""
import numpy as np
import pytest

import mpc_oracle as mo
import sens_face_cases as fc
import sens_face_ref as fr
import sens_ref as sr


def _ops(p):
    return p.A, p.B, p.Q, p.R, p.P


@pytest.mark.parametrize("name", fc.NAMES)
def test_restatement_against_the_direct_form(name):
    _, X0, _ = fc.case(name)
    U = fc.exact_inputs(name)
    g_u, g_x = fc.loss(name)
    gap_j = gap_v = 0.0
    rows = []
    for i in fc.instances(name):
        p = fc.problem_of(name, i)
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
        nearest_free, mixed, most, clamped, free = np.inf, False, 0, False, False
        for i in fc.instances(name):
            p = fc.problem_of(name, i)
            dist = fr.distance_to_bounds(U[i], p.u_min, p.u_max)
            assert not np.any((dist > fc.BAND[0]) & (dist < fc.BAND[1])), (name, i, dist[(dist > fc.BAND[0]) & (dist < fc.BAND[1])])
            act = fr.active_rows(U[i], p.u_min, p.u_max)
            assert np.array_equal(act, (dist <= fc.BAND[0]).T.reshape(-1))
            nearest_free = min(nearest_free, dist[dist > fc.BAND[0]].min(initial=np.inf))
            mixed = mixed or (0 < act.sum() < act.size) or act.size == 1   # (1-1-1 has one row: clamped and free instances, below)
            clamped, free = clamped or bool(act.any()), free or not act.all()
            most = max(most, int(act.sum()))
        print(f"{name}: nearest free input at {nearest_free:.1e} of its width, working sets up to {most} rows")
        assert mixed and clamped and free, name
        if name in fc.TIER_NAMES:
            assert most > 32, (name, most)
