"""CPU checks of the parameter-gradient formulas (tests/sens_params_ref.py) on the oracle's solutions, and of the new surface.

1  The direct form against central differences of mpc_oracle.solve_box_qp_exact with the design rebuilt (dataclasses.replace on the
   MPCProblem, P given so that it stays fixed): a linear loss sum g_u.u + sum g_x.x, three random directions per parameter group
   (symmetric for Q, P, R, S), h = 1e-6, bound FD_RTOL = 1e-5 of max(1, |value|) (seen: <= 2e-7).  Every instance of every case
   takes part; a guard on the exact solutions keeps a change of face from hiding: the smallest multiplier on W is >= 1e-3 and the
   smallest distance of a free row to its bounds is >= 1e-4.
2  The G form the device computes against the direct form, per case and group over max(1, max|group|) per instance; the worst gap of
   a case is recorded in sens_params_cases.MEASURED_GAP and a run must stay within GAP_SLACK = 4 of the record.
3  dL/dx0 of the restatement equals sens_ref.vjp_direct, and mu_1 equals it to 1e-12 of max(1, max|g_x0|) on the three cases of (1).
   (On the quadrotor, whose H has a condition number of 1e10, two evaluations of the same H_FF solve already differ by 5e-11: the
   figure is printed there, not asserted.)
4  The two symbols are in the header and in _capi's argtypes, the struct's fields are in the header's order, the Julia shim names both.
"""
import dataclasses
import os
import re

import numpy as np
import pytest

import sens_params_cases as pc
import sens_params_ref as pr
import sens_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_H = 1e-6
FD_RTOL = 1e-5
MIN_MULT, MIN_GAP = 1e-3, 1e-4


def _solve(mo, p, x0):
    H, f, lo, hi = mo.condensed_qp(p, x0)
    v = mo.solve_box_qp_exact(H, f, lo, hi)
    return mo.rollout(p, x0, v), (H, f, lo, hi, v)


@pytest.fixture(scope="module")
def solved(mo):
    """Per case: the problem, its design data and the oracle's solutions with their working sets, computed once."""
    out = {}
    for name in pc.G_CASES:
        ps, X0 = pc.problems(mo, name)
        designs = {}   # (H, F, d, G-form operands) per distinct model
        sol = []
        for p, x0 in zip(ps, X0):
            if id(p.A) not in designs:
                _, _, H, F = mo.condense(p)
                d = mo.jacobi_scaling(H)
                designs[id(p.A)] = (H, F, d, sr.g_operands(H, F, d))
            H, F, d, ops = designs[id(p.A)]
            res, (Hq, f, lo, hi, v) = _solve(mo, p, x0)
            act, lower = pr.sides(res["u"], p.u_min, p.u_max, d)
            g = Hq @ v + f
            sol.append(dict(p=p, H=H, F=F, d=d, ops=ops, res=res, act=act, lower=lower, mult=np.where(lower, g, -g)[act],
                            gap=np.minimum(v - lo, hi - v)[~act]))
        out[name] = dict(p=ps[0], X0=X0, H=sol[0]["H"], F=sol[0]["F"], sol=sol)
    return out


def _sym(M):
    return 0.5 * (M + M.T)


def _directions(rng, p):
    """Three directions per parameter group: (group, field of the problem or 'x0', direction)."""
    n, m, N = p.n, p.m, p.N
    out = []
    for _ in range(3):
        out += [("x0", rng.normal(size=n)), ("u_ref", rng.normal(size=(m, N))), ("u_min", rng.normal(size=m)), ("u_max", rng.normal(size=m)),
                ("Q", _sym(rng.normal(size=(n, n)))), ("P", _sym(rng.normal(size=(n, n)))), ("R", _sym(rng.normal(size=(m, m)))),
                ("S", _sym(rng.normal(size=(m, m)))), ("A", rng.normal(size=(n, n))), ("B", rng.normal(size=(n, m)))]
    return out


def _perturbed(p, x0, group, D, h):
    if group == "x0":
        return p, x0 + h * D
    if group == "S" and p.S[0, 0] == 0.0:
        return p, x0   # (the design drops S: the cost does not depend on it, the gradient is zero)
    return dataclasses.replace(p, **{group: getattr(p, group) + h * D}), x0


def test_direct_form_matches_finite_differences_with_the_design_rebuilt(mo, solved):
    for name in pc.FD_CASES:
        c = solved[name]
        p = c["p"]
        rows = [int(s["act"].sum()) for s in c["sol"]]
        n_lo = sum(int((s["act"] & s["lower"]).sum()) for s in c["sol"])
        n_hi = sum(int((s["act"] & ~s["lower"]).sum()) for s in c["sol"])
        min_mult = min((s["mult"].min() for s in c["sol"] if s["mult"].size), default=np.inf)
        min_gap = min((s["gap"].min() for s in c["sol"] if s["gap"].size), default=np.inf)
        assert min_mult >= MIN_MULT and min_gap >= MIN_GAP, (name, min_mult, min_gap)
        assert min(rows) == 0 and n_lo > 0 and n_hi > 0, (name, rows, n_lo, n_hi)
        if name == "di":
            assert (min(rows), max(rows), n_lo, n_hi) == (0, 10, 50, 66)
        rng = np.random.default_rng(23)
        worst = {}
        for x0, s in zip(c["X0"], c["sol"]):
            g_u, g_x = pc.loss(rng, p)
            got = pr.params_direct(pr.prob_of(p), c["H"], c["F"], s["act"], s["lower"], s["res"], g_u, g_x)
            for group, D in _directions(rng, p):
                L = []
                for sgn in (1.0, -1.0):
                    pp, xx = _perturbed(p, x0, group, D, sgn * FD_H)
                    r, _ = _solve(mo, pp, xx)
                    L.append(float((g_u * r["u"]).sum() + (g_x * r["x"]).sum()))
                fd = (L[0] - L[1]) / (2 * FD_H)
                val = float((got[group] * D).sum())
                err = abs(val - fd) / max(1.0, abs(val))
                worst[group] = max(worst.get(group, 0.0), err)
        print(f"{name}: rows {min(rows)} .. {max(rows)}, {n_lo} lower, {n_hi} upper, smallest multiplier {min_mult:.3g}, smallest gap "
              f"{min_gap:.3g}; worst error against central differences per group: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
        assert max(worst.values()) <= FD_RTOL, worst


def test_g_form_equals_the_direct_form_on_every_case(solved):
    for name in pc.G_CASES:
        c = solved[name]
        rng = np.random.default_rng(29)
        worst = dict.fromkeys(pr.GROUPS, 0.0)
        for s in c["sol"]:
            p = s["p"]
            g_u, g_x = pc.loss(rng, p)
            a = pr.params_direct(pr.prob_of(p), s["H"], s["F"], s["act"], s["lower"], s["res"], g_u, g_x)
            b = pr.params_gform(pr.prob_of(p), s["ops"], s["d"], s["act"], s["lower"], s["res"], g_u, g_x)
            for k, e in pr.worst_gaps(b, a).items():
                worst[k] = max(worst[k], e)
        rows = [int(s["act"].sum()) for s in c["sol"]]
        print(f"{name}: rows {min(rows)} .. {max(rows)}, {sum(r > 32 for r in rows)} beyond 32; gap to the direct form per group: "
              + ", ".join(f"{k} {v:.1e}" for k, v in worst.items())
              + f"; worst {max(worst.values()):.3e} (recorded {pc.MEASURED_GAP[name]:g}, tolerance on the device {pc.gpu_tol(name):g})")
        assert max(worst.values()) <= pc.GAP_SLACK * pc.MEASURED_GAP[name]
    rows = [int(s["act"].sum()) for s in solved["quad"]["sol"]]
    assert (min(rows), max(rows)) == (2, 15), rows
    assert sum(int(s["act"].sum()) > 32 for s in solved["quad_big"]["sol"]) >= 1
    assert min(s["mult"].min() for s in solved["quad"]["sol"]) >= MIN_MULT


def test_x0_gradient_is_the_vjp_of_the_existing_restatement(solved):
    for name in pc.G_CASES:
        c = solved[name]
        rng = np.random.default_rng(31)
        w_x0 = w_mu = 0.0
        for s in c["sol"]:
            p = s["p"]
            g_u, g_x = pc.loss(rng, p)
            a = pr.params_direct(pr.prob_of(p), s["H"], s["F"], s["act"], s["lower"], s["res"], g_u, g_x)
            vd = sr.vjp_direct(s["H"], s["F"], s["act"], p.A, p.B, g_u, g_x)
            w_x0 = max(w_x0, np.abs(a["x0"] - vd).max() / sr.vjp_scale(vd))
            w_mu = max(w_mu, np.abs(a["mu1"] - vd).max() / sr.vjp_scale(vd))
        print(f"{name}: lam_1 + F'z against vjp_direct {w_x0:.3e}, mu_1 against it {w_mu:.3e}")
        if name in pc.FD_CASES:
            assert w_x0 <= 1e-12 and w_mu <= 1e-12


NAMES = ("almpc_sensitivity_params_vjp", "almpc_group_sensitivity_params_vjp")


def test_header_and_bindings_carry_the_parameter_gradients(pkg):
    header = open(os.path.join(ROOT, "include", "almpc.h")).read()
    declared = set(re.findall(r"\b(almpc_[a-z0-9_]+)\s*\(", header))
    assert not [n for n in NAMES if n not in declared]
    capi = pkg._capi
    for cls in (capi.Solver, capi.Group):
        assert callable(getattr(cls, "sensitivity_params_vjp"))
    assert not [n for n in NAMES if n not in capi.prototypes()]
    body = re.search(r"typedef struct almpc_param_grads \{(.*?)\} almpc_param_grads;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in capi.almpc_param_grads._fields_], (fields, capi.almpc_param_grads._fields_)
    assert fields == ["x0", "f", "u_ref", "u_min", "u_max", "Q", "P", "A", "R", "S", "B", "rows"]
    shim = open(os.path.join(ROOT, "julia", "AlmpcHIP.jl")).read()
    assert not [n for n in NAMES if ("(:" + n + ", libalmpc)") not in shim]
    assert "sensitivity_params" in __import__("importlib").import_module(pkg.__name__ + ".controller").__all__
