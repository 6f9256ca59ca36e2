"""CPU checks of the sensitivity formulas (tests/sens_ref.py) against finite differences of the exact oracle, of the G-based form the
device computes against the direct H_FF solve, and of the new surface (header, bindings).

Bounds.  Finite differences: central, h = 1e-6 per state, relative error <= 1e-5 of max(1, max|J|) (measured 1.2e-7 for J, 1.6e-6 for dX; the truncation
term is zero on a fixed face -- the solution is affine there -- so what is left is the oracle's own 1e-9-certified solve divided by
2h).  No instance is left out: on these inputs no active set changes within +-h (smallest scaled multiplier 5e-5, smallest scaled gap
0.44).  G form against direct form: 1e-9 (J: of max(1, max|J|); VJP: of max(1, max|g_x0|), sens_ref.vjp_scale; measured figures are printed
by the test and recorded in DESIGN.md).
"""
import os
import re

import numpy as np
import pytest

import sens_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_H = 1e-6
FD_RTOL = 1e-5
FORM_TOL = 1e-9


def _cases(mo):
    pd = mo.double_integrator(N=10)
    pq = mo.quadrotor(N=30)
    return [("double_integrator", pd, 3.0 * np.random.default_rng(7).normal(size=(32, 2))),
            ("quadrotor", pq, mo.quadrotor_x0_batch(16, amplitude=1.0))]


def _solve(mo, p, H, F, lo, hi, fS, x0):
    return mo.solve_box_qp_exact(H, F @ (x0 - p.x_ref[:, 0]) + fS, lo, hi)


@pytest.fixture(scope="module")
def solved(mo):
    """Per case: the problem, its condensed data and, per instance, the exact solution with its Jacobian by central differences."""
    out = []
    for name, p, X0 in _cases(mo):
        _, _, H, F = mo.condense(p)
        _, _, lo, hi = mo.condensed_qp(p, X0[0])
        fS = mo.s_rate_gradient(p)
        d = mo.jacobi_scaling(H)
        inst = []
        for x0 in X0:
            v = _solve(mo, p, H, F, lo, hi, fS, x0)
            Jfd = np.zeros((p.nz, p.n))
            Xfd = np.zeros((p.n, p.N + 1, p.n))
            for c in range(p.n):
                e = np.zeros(p.n); e[c] = FD_H
                vp, vm = _solve(mo, p, H, F, lo, hi, fS, x0 + e), _solve(mo, p, H, F, lo, hi, fS, x0 - e)
                Jfd[:, c] = (vp - vm) / (2 * FD_H)
                Xfd[:, :, c] = (mo.rollout(p, x0 + e, vp)["x"] - mo.rollout(p, x0 - e, vm)["x"]) / (2 * FD_H)
            u = mo.rollout(p, x0, v)["u"]
            inst.append(dict(x0=x0, u=u, act=sr.active_rows(u, p.u_min, p.u_max, d), Jfd=Jfd, Xfd=Xfd))
        out.append(dict(name=name, p=p, H=H, F=F, d=d, inst=inst))
    return out


def test_restatement_matches_finite_differences_of_the_exact_oracle(solved):
    for case in solved:
        rows = [int(q["act"].sum()) for q in case["inst"]]
        worst = 0.0
        for q in case["inst"]:
            J = sr.jac_direct(case["H"], case["F"], q["act"])
            worst = max(worst, np.abs(J - q["Jfd"]).max() / max(1.0, np.abs(J).max()))
        print(f"{case['name']}: |W| {min(rows)} .. {max(rows)}, worst relative error against central differences {worst:.3e}")
        assert worst <= FD_RTOL
        if case["name"] == "double_integrator":
            assert min(rows) == 0 and max(rows) == case["p"].nz, rows
        else:
            assert max(rows) > 0


def test_g_form_equals_the_direct_form(mo, solved):
    rng = np.random.default_rng(11)
    batches = [(c["p"], c["H"], c["F"], c["d"], [q["act"] for q in c["inst"]]) for c in solved]
    pq = mo.quadrotor(N=30)
    _, _, H, F = mo.condense(pq)
    _, _, lo, hi = mo.condensed_qp(pq, np.zeros(pq.n))
    d = mo.jacobi_scaling(H)
    for a in (0.3, 3.0):
        acts = []
        for x0 in mo.quadrotor_x0_batch(48, a):
            u = mo.rollout(pq, x0, _solve(mo, pq, H, F, lo, hi, mo.s_rate_gradient(pq), x0))["u"]
            acts.append(sr.active_rows(u, pq.u_min, pq.u_max, d))
        batches.append((pq, H, F, d, acts))
    worst_j = worst_v = 0.0
    for p, H, F, d, acts in batches:
        for act in acts:
            Jd, Jg = sr.jac_direct(H, F, act), sr.jac_gform(H, F, d, act)
            worst_j = max(worst_j, np.abs(Jd - Jg).max() / max(1.0, np.abs(Jd).max()))
            g_u, g_x = rng.normal(size=(p.m, p.N)), rng.normal(size=(p.n, p.N + 1))
            vd = sr.vjp_direct(H, F, act, p.A, p.B, g_u, g_x)
            vg = sr.vjp_gform(H, F, d, act, p.A, p.B, g_u, g_x)
            worst_v = max(worst_v, np.abs(vd - vg).max() / sr.vjp_scale(vd))
    print(f"G form against direct form: J {worst_j:.3e}, VJP {worst_v:.3e}")
    assert worst_j <= FORM_TOL and worst_v <= FORM_TOL


def test_dx_matches_finite_differences_of_the_rollout(solved):
    for case in solved:
        p = case["p"]
        worst = 0.0
        for q in case["inst"]:
            dX = sr.dx_from_du(p.A, p.B, sr.jac_direct(case["H"], case["F"], q["act"]), p.N)
            assert np.array_equal(dX[:, 0, :], np.eye(p.n))
            worst = max(worst, np.abs(dX - q["Xfd"]).max() / max(1.0, np.abs(dX).max()))
            # and the VJP restatement is the transpose of these Jacobians
            g_u, g_x = np.cos(np.arange(p.m * p.N)).reshape(p.m, p.N), np.sin(np.arange(p.n * (p.N + 1))).reshape(p.n, p.N + 1)
            _, dU = sr.shaped(sr.jac_direct(case["H"], case["F"], q["act"]), p.m, p.N)
            ref = sr.vjp_from_jacobians(dU, dX, g_u, g_x)
            got = sr.vjp_direct(case["H"], case["F"], q["act"], p.A, p.B, g_u, g_x)
            assert np.abs(ref - got).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        print(f"{case['name']}: dX worst relative error against central differences {worst:.3e}")
        assert worst <= FD_RTOL


SENS_NAMES = ("almpc_sensitivity", "almpc_get_sensitivity", "almpc_device_sensitivity", "almpc_sensitivity_vjp",
              "almpc_group_sensitivity", "almpc_group_get_sensitivity", "almpc_group_sensitivity_vjp")


def test_header_and_bindings_carry_the_new_surface(pkg):
    """The entry points of the issue's ABI block and its three group forms, the three ALMPC_SENS_* bits with the same values in
    the Python binding, and the methods above the ABI."""
    header = open(os.path.join(ROOT, "include", "almpc.h")).read()
    declared = set(re.findall(r"\b(almpc_[a-z0-9_]+)\s*\(", header))
    assert not [n for n in SENS_NAMES if n not in declared]
    bits = dict(re.findall(r"#define ALMPC_SENS_(K0|DU|DX) (0x[0-9a-f]+)u", header))
    assert {k: int(v, 16) for k, v in bits.items()} == {"K0": 1, "DU": 2, "DX": 4}
    capi = pkg._capi
    assert capi.SENS == {"K0": 1, "dU": 2, "dX": 4}
    for cls in (capi.Solver, capi.Group):
        assert callable(getattr(cls, "sensitivity")) and callable(getattr(cls, "sensitivity_vjp"))
    assert not [n for n in SENS_NAMES if n not in capi.prototypes()]
    assert callable(getattr(__import__("importlib").import_module(pkg.__name__ + ".controller"), "sensitivity"))
