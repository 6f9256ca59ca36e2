"""CPU checks of the rows-form sensitivity formulas (tests/sens_rows_ref.py) on the oracle's solutions, and of the new surface.

(a) The direct KKT form against central differences of mpc_oracle.solve_mpc_exact, h = 1e-6 per state, on the double integrator with
    the state box, with the terminal equality and with both, 12 instances each: bound 1e-5 of max(1, max|J|) (measured 6.1e-7 for J,
    1.1e-6 for dX; on a fixed face the solution is affine in x0, so what is left is the oracle's own certified solve divided by 2h).
    Only instances whose active set is the same at x0 +- h e_c take part.
(b), (c) The G form the device computes and its projected variant against (a) on every case of the GPU test
    (tests/sens_rows_cases.py), Jacobians over max(1, max|J|) and VJPs over max(1, max|g_x0|).  The worst gap of a case is recorded in
    sens_rows_cases.MEASURED_GAP (4.6e-13 ... 4.8e-13 on the double integrator, 5.7e-15 ... 8.5e-15 on the two random models, 3.5e-11
    and 3.9e-11 on the quadrotor without and with the equality); ten times it is the case's tolerance on the device.  A run must stay
    within GAP_SLACK = 4 of the record: the gaps are sums of roundings and move with the BLAS underneath numpy.

The same test asserts what keeps the GPU cases honest, on the oracle's solutions: in every case with a box some solved instance has
active state-box rows and some has none (the equality-only case has its n equality rows in every instance and instances with and
without active input rows); no solved instance has cond(Ghat_WW) > 1e10; no state row lies between 1e-9 and 1e-5 of max(1, |bound|)
from its bound.
"""
import os
import re

import numpy as np
import pytest

import sens_ref as sr
import sens_rows_cases as sc
import sens_rows_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_H = 1e-6
FD_RTOL = 1e-5


def _design(mo, p):
    _, _, H, F = mo.condense(p)
    d = mo.jacobi_scaling(H)
    st, ix, eq = rr.state_rows(p.n, p.N, p.x_min is not None, p.terminal == "equality")
    Gam, Phi = rr.row_tables(p.A, p.B, p.N, st, ix)
    return dict(H=H, F=F, d=d, st=st, ix=ix, eq=eq, Gam=Gam, Phi=Phi)


def _solve(mo, p, D, x0):
    """The oracle's solution with its active rows, or None where the instance is infeasible."""
    try:
        e = mo.solve_mpc_exact(p, x0)
    except ValueError:
        return None
    e["act_u"] = sr.active_rows(e["u"], p.u_min, p.u_max, D["d"])
    e["act_x"] = rr.active_state_rows(e["x"], p.x_min, p.x_max, D["st"], D["ix"], D["eq"])
    return e


@pytest.fixture(scope="module")
def solved(mo):
    """Per case: the problem, its design data and the oracle's solutions (None: infeasible), computed once."""
    out = {}
    for name in sc.GPU_CASES:
        p, X0 = sc.case(mo, name)
        D = _design(mo, p)
        out[name] = dict(p=p, X0=X0, D=D, sol=[_solve(mo, p, D, x0) for x0 in X0])
    return out


def test_row_tables_are_the_oracles_condensation(mo, solved):
    for name in ("di_both", "r637_box", "quad_both"):
        p, D = solved[name]["p"], solved[name]["D"]
        cr = mo.constraint_rows(p)
        assert np.array_equal(cr["stage"] + 1, D["st"]) and np.array_equal(cr["state"], D["ix"]) and np.array_equal(cr["eq"], D["eq"])
        assert np.abs(cr["C"] - D["Gam"]).max() <= 1e-12 * max(1.0, np.abs(cr["C"]).max())
        assert np.abs(cr["Phi"] - D["Phi"]).max() <= 1e-12 * max(1.0, np.abs(cr["Phi"]).max())


def test_direct_form_matches_finite_differences_of_the_exact_oracle(mo, solved):
    for name in sc.DI_CASES:
        c = solved[name]
        p, D = c["p"], c["D"]
        worst_j = worst_x = 0.0
        used = with_state = 0
        for x0, e in list(zip(c["X0"], c["sol"]))[:12]:
            assert e is not None
            Jfd, Xfd, same = np.zeros((p.nz, p.n)), np.zeros((p.n, p.N + 1, p.n)), True
            for col in range(p.n):
                h = np.zeros(p.n); h[col] = FD_H
                ep, em = _solve(mo, p, D, x0 + h), _solve(mo, p, D, x0 - h)
                same = same and all(q is not None and np.array_equal(q["act_u"], e["act_u"]) and np.array_equal(q["act_x"], e["act_x"])
                                    for q in (ep, em))
                if not same:
                    break
                Jfd[:, col] = (ep["u"] - em["u"]).T.reshape(-1) / (2 * FD_H)
                Xfd[:, :, col] = (ep["x"] - em["x"]) / (2 * FD_H)
            if not same:
                continue
            used += 1
            with_state += int((e["act_x"] & ~D["eq"]).any())
            J = rr.jac_direct(D["H"], D["F"], D["Gam"], D["Phi"], e["act_u"], e["act_x"])
            dX = sr.dx_from_du(p.A, p.B, J, p.N)
            worst_j = max(worst_j, np.abs(J - Jfd).max() / max(1.0, np.abs(J).max()))
            worst_x = max(worst_x, np.abs(dX - Xfd).max() / max(1.0, np.abs(dX).max()))
            if D["eq"].any():   # the terminal state does not move with x0
                assert np.abs(dX[:, p.N, :]).max() <= 1e-9
        print(f"{name}: {used} of 12 instances keep their active set within +-h ({with_state} with active box rows); "
              f"worst relative error against central differences: J {worst_j:.3e}, dX {worst_x:.3e}")
        assert used >= 6 and worst_j <= FD_RTOL and worst_x <= FD_RTOL
        assert with_state >= 1 or p.x_min is None


def test_g_forms_equal_the_direct_form_on_every_gpu_case(solved):
    for name in sc.GPU_CASES:
        c = solved[name]
        p, D = c["p"], c["D"]
        ops = rr.rows_operands(D["H"], D["F"], D["d"], D["Gam"], D["Phi"])
        E = p.nz + np.nonzero(D["eq"])[0]
        ops_p = rr.project(*ops, E) if E.size else None
        rng = np.random.default_rng(11)
        gap_j = gap_v = worst_cond = 0.0
        n_state, n_in, n_all = [], [], []
        for e in c["sol"]:
            if e is None:
                continue
            au, ax = e["act_u"], e["act_x"]
            gaps = rr.bound_gaps(e["x"], p.x_min, p.x_max, D["st"], D["ix"], D["eq"])
            assert not np.any((gaps > 1e-9) & (gaps < 1e-5)), (name, gaps[(gaps > 1e-9) & (gaps < 1e-5)])
            worst_cond = max(worst_cond, rr.cond_S(ops, au, ax))
            Jd = rr.jac_direct(D["H"], D["F"], D["Gam"], D["Phi"], au, ax)
            g_u, g_x = rng.normal(size=(p.m, p.N)), rng.normal(size=(p.n, p.N + 1))
            vd = rr.vjp_direct(D["H"], D["F"], D["Gam"], D["Phi"], au, ax, p.A, p.B, g_u, g_x)
            forms = [(rr.jac_gform(ops, D["d"], au, ax), rr.vjp_gform(ops, D["d"], au, ax, p.A, p.B, g_u, g_x))]
            if E.size:
                forms.append((rr.jac_projected(ops_p, D["d"], au, ax, D["eq"]),
                              rr.vjp_projected(ops_p, D["d"], au, ax, D["eq"], p.A, p.B, g_u, g_x)))
            for Jg, vg in forms:
                gap_j = max(gap_j, np.abs(Jg - Jd).max() / max(1.0, np.abs(Jd).max()))
                gap_v = max(gap_v, np.abs(vg - vd).max() / sr.vjp_scale(vd))
            # the VJP restatement is the transpose of the Jacobians
            _, dU = sr.shaped(Jd, p.m, p.N)
            own = sr.vjp_from_jacobians(dU, sr.dx_from_du(p.A, p.B, Jd, p.N), g_u, g_x)
            assert np.abs(own - vd).max() <= 1e-9 * sr.vjp_scale(vd)
            n_state.append(int((ax & ~D["eq"]).sum())); n_in.append(int(au.sum())); n_all.append(int(au.sum() + ax.sum()))
        infeasible = sum(e is None for e in c["sol"])
        print(f"{name}: {infeasible} of {len(c['sol'])} infeasible; rows (input, state box) up to ({max(n_in)}, {max(n_state)}), |W| "
              f"{min(n_all)} .. {max(n_all)}, {sum(r > 32 for r in n_all)} beyond 32; worst cond(Ghat_WW) {worst_cond:.2e}; gap to the direct form: "
              f"J {gap_j:.3e}, VJP {gap_v:.3e} (recorded {sc.MEASURED_GAP[name]:g}, tolerance on the device {sc.gpu_tol(name):g})")
        assert max(gap_j, gap_v) <= sc.GAP_SLACK * sc.MEASURED_GAP[name]
        assert worst_cond <= 1e10
        if p.x_min is not None:
            assert max(n_state) > 0 and min(n_state) == 0, n_state
        else:
            assert max(n_in) > 0 and min(n_in) == 0 and all(r - i == p.n for r, i in zip(n_all, n_in))
    # the paths the shapes are there for
    q = solved["quad_box"]
    assert sum(e is not None and e["act_u"].sum() + e["act_x"].sum() > 32 for e in q["sol"]) >= 1
    assert sum(e is None for e in solved["quad_both"]["sol"]) >= 1 and sum(e is None for e in solved["r637_box"]["sol"]) >= 1


def test_state_row_rule_ignores_bounds_that_are_none():
    st, ix, eq = rr.state_rows(2, 3, True, True)
    assert st.tolist() == [1, 1, 2, 2, 3, 3] and eq.tolist() == [False] * 4 + [True] * 2
    x = np.array([[0.0, 1.0, 1.0 - 5e-8, 7.0], [0.0, -1e300, 2.0, 3.0]])
    act = rr.active_state_rows(x, np.array([-1.0, -1e300]), np.array([1.0, np.inf]), st, ix, eq)
    assert act.tolist() == [True, False, True, False, True, True]
    assert rr.state_rows(2, 3, False, True)[0].tolist() == [3, 3]


ROWS_NAMES = ("almpc_sensitivity_rows", "almpc_sensitivity_rows_vjp", "almpc_group_sensitivity_rows", "almpc_group_sensitivity_rows_vjp")


def test_header_and_bindings_carry_the_rows_form(pkg):
    header = open(os.path.join(ROOT, "include", "almpc.h")).read()
    declared = set(re.findall(r"\b(almpc_[a-z0-9_]+)\s*\(", header))
    assert not [n for n in ROWS_NAMES if n not in declared]
    capi = pkg._capi
    for cls in (capi.Solver, capi.Group):
        assert callable(getattr(cls, "sensitivity_rows")) and callable(getattr(cls, "sensitivity_rows_vjp"))
    assert not [n for n in ROWS_NAMES if n not in capi.prototypes()]
    shim = open(os.path.join(ROOT, "julia", "AlmpcHIP.jl")).read()
    assert not [n for n in ROWS_NAMES if ("(:" + n + ", libalmpc)") not in shim]
