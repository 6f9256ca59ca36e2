"""The certificate's restatement (tests/cert_ref.py) against the condensed oracle (oracle/mpc_oracle.py), on the CPU, on every case of
tests/cert_cases.py and every instance: the recursion equals the condensed QP's gradient, cost and KKT residual within the rounding
bounds of both sides (cert_ref's docstring, cert_ref.condensed_bound), the residual vanishes at the exact optimum, and the first costate
is the derivative of the optimal cost in x0.  Also: the header declares the entry points and the Python binding has them."""
import functools
import os
import re

import numpy as np
import pytest

import cert_cases as cc
import cert_ref as cr
import mpc_oracle as mo
from conftest import ROOT

SYMBOLS = ("almpc_certificate", "almpc_get_certificate", "almpc_device_certificate", "almpc_group_certificate", "almpc_group_get_certificate")
FD_H, FD_TOL = 1e-6, 1e-6


@functools.lru_cache(maxsize=None)
def _condensed(name, i):
    c = cc.case(name)
    p = c.problems[i]
    if i > 0 and p is c.problems[0]:
        return _condensed(name, 0)
    return mo.condense(p)


def _qp(name, i, x0):
    p = cc.case(name).problems[i]
    Phi, Gam, H, F = _condensed(name, i)
    lo, hi = cc.flat_bounds(p)
    return p, H, F @ (np.asarray(x0) - p.x_ref[:, 0]) + mo.s_rate_gradient(p), lo, hi


def _cert(p, x0, v):
    r = mo.rollout(p, x0, v)
    return cr.certificate(p.A, p.B, p.Q, p.R, p.S, p.P, p.u_min, p.u_max, r["e_x"], r["e_u"], r["u"]), r


def _j0(p, Phi, e0, absval):
    """the cost of v = 0 from the condensed prediction E = Phi e0 (absval: on absolute values, Phi those of cert_ref.condensed_bound)"""
    a = np.abs if absval else (lambda x: x)
    n, N = p.n, p.N
    useR, useS = cr.branch(p.R, p.S)
    E = (Phi @ a(e0)).reshape(N, n)
    Q, P = a(cr.sym(p.Q)), a(cr.sym(p.P))
    j = float(a(e0) @ Q @ a(e0)) + sum(float(E[k] @ Q @ E[k]) for k in range(N - 1)) + float(E[N - 1] @ P @ E[N - 1])
    if useS:
        ur = a(p.u_ref)
        d = ur[:, :-1] + ur[:, 1:] if absval else ur[:, :-1] - ur[:, 1:]
        j += float(np.sum(d * (a(cr.sym(p.S)) @ d)))
    return j


@pytest.mark.parametrize("name", cc.NAMES)
def test_recursion_equals_the_condensed_qp_at_random_feasible_inputs(name):
    c = cc.case(name)
    rng = np.random.default_rng(len(name) + c.n)
    for i in range(c.batch):
        p, H, f, lo, hi = _qp(name, i, c.X0[i])
        v = lo + rng.random(lo.size) * (hi - lo)
        k, r = _cert(p, c.X0[i], v)
        useR, useS = cr.branch(p.R, p.S)
        e0 = c.X0[i] - p.x_ref[:, 0]
        cb = cr.condensed_bound(p.A, p.B, p.Q, p.R, p.S, p.P, p.N, e0, v, p.u_ref, useR, useS)
        g = (H @ v + f).reshape(p.N, p.m).T
        tol_g = 0.5 * k["tol_grad"] + cr.gamma(cb["ops"]) * cb["mag_grad"]   # (one side each)
        assert np.all(np.abs(k["grad"] - g) <= tol_g), (name, i, float(np.max(np.abs(k["grad"] - g) / tol_g)))
        # cost = 1/2 v'Hv + f'v + J(0)
        Phi = _condensed(name, i)[0]
        cost = 0.5 * float(v @ H @ v) + float(f @ v) + _j0(p, Phi, e0, False)
        mag_c = float(np.abs(v) @ (cb["H"] @ np.abs(v))) + float(cb["f"] @ np.abs(v)) + _j0(p, cb["Phi"], e0, True)
        tol_c = 0.5 * k["tol_cost"] + cr.gamma(cb["ops"] + p.n * p.N + p.m * p.N + 4) * mag_c
        assert abs(k["cost"] - cost) <= tol_c, (name, i, abs(k["cost"] - cost) / tol_c)
        # res = kkt_residual, which works in v = u - u_ref: three more roundings of numbers no larger than |u| + |u_ref| + |g|
        res = mo.kkt_residual(H, f, lo, hi, v)
        tol_r = float(np.max(tol_g)) + 2.0 ** -52 * float(np.max(np.abs(r["u"]) + np.abs(g))) \
            + 3 * 2.0 ** -53 * float(np.max(np.abs(r["u"]) + np.abs(p.u_ref) + np.abs(g)))
        assert abs(k["res"] - res) <= tol_r, (name, i, abs(k["res"] - res) / tol_r)


@pytest.mark.parametrize("name", cc.NAMES)
def test_residual_vanishes_at_the_exact_optimum(name):
    c = cc.case(name)
    for i in range(c.batch):
        k, _ = _cert(c.problems[i], c.X0[i], cc.exact(name, i))
        assert k["res"] <= 1e-9 * max(1.0, float(np.max(np.abs(k["grad"])))), (name, i, k["res"])


def test_quadrotor_case_has_free_and_clamped_inputs_and_a_decidable_residual():
    c = cc.case("quad-12-4-5")
    p = c.problems[0]
    lo, hi = cc.flat_bounds(p)
    at_bound = lambda v: (v - lo <= 1e-12 * (hi - lo)) | (hi - v <= 1e-12 * (hi - lo))
    clamped = np.array([np.sum(at_bound(cc.exact(c.name, i))) for i in range(c.batch)])
    assert clamped.min() == 0 and clamped.max() > 0 and np.any((clamped > 0) & (clamped < lo.size)), clamped
    # (cert_cases.QUAD_AMPLITUDES) the rounding bound of g stays a small share of the threshold of the solved-batch check
    for i in range(c.batch):
        k, _ = _cert(p, c.X0[i], cc.exact(c.name, i))
        assert np.max(k["tol_grad"]) <= cc.QUAD_NOISE_SHARE * 1e-9 * max(1.0, float(np.max(np.abs(k["grad"])))), (i, float(np.max(k["tol_grad"])))
        # (cert_cases.QUAD_MULTIPLIER_MARGIN) no input sits weakly at a bound: every clamped input's multiplier is far from zero
        v, g = cc.exact(c.name, i), k["grad"].T.reshape(-1)
        at_hi, at_lo = hi - v <= 1e-12 * (hi - lo), v - lo <= 1e-12 * (hi - lo)
        mu = np.where(at_hi, -g, np.where(at_lo, g, np.inf))
        assert np.all(mu >= cc.QUAD_MULTIPLIER_MARGIN * 1e-9 * max(1.0, float(np.max(np.abs(g))))), (i, float(mu.min()))


@pytest.mark.parametrize("name", cc.NAMES)
def test_first_costate_is_the_derivative_of_the_optimal_cost(name):
    c = cc.case(name)
    for i in range(c.batch):
        p = c.problems[i]
        lam0 = _cert(p, c.X0[i], cc.exact(name, i))[0]["costate"][:, 0]
        fd = np.zeros(p.n)
        for j in range(p.n):
            J, act = [], []
            for sgn in (1.0, -1.0):
                x0 = c.X0[i].copy(); x0[j] += sgn * FD_H
                _, H, f, lo, hi = _qp(name, i, x0)
                v = mo.solve_box_qp_exact(H, f, lo, hi)
                J.append(_cert(p, x0, v)[0]["cost"]); act.append(((v == lo), (v == hi)))
            assert np.array_equal(act[0][0], act[1][0]) and np.array_equal(act[0][1], act[1][1]), (name, i, j, "the active set changes inside the step")
            fd[j] = (J[0] - J[1]) / (2.0 * FD_H)
        assert np.max(np.abs(fd - lam0)) <= FD_TOL * max(1.0, float(np.max(np.abs(lam0)))), (name, i, float(np.max(np.abs(fd - lam0))))


def test_nonfinite_trajectory_gives_nonfinite_outputs():
    c = cc.case("2-1-2-S")
    p = c.problems[0]
    r = mo.rollout(p, c.X0[0], np.zeros(p.m * p.N))
    r["e_x"][0, 1] = np.nan
    k = cr.certificate(p.A, p.B, p.Q, p.R, p.S, p.P, p.u_min, p.u_max, r["e_x"], r["e_u"], r["u"])
    assert np.isnan(k["cost"]) and np.isnan(k["res"]) and np.isnan(k["costate"][:, 0]).all()


def test_header_declares_the_entry_points_and_the_binding_has_them(pkg):
    with open(os.path.join(ROOT, "include", "almpc.h")) as f:
        header = f.read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
    for bit, val in (("COST", 1), ("RES", 2), ("GRAD", 4), ("COSTATE", 8)):
        assert re.search(r"#define ALMPC_CERT_%s %du\b" % (bit, val), header), bit
    capi = pkg._capi
    for s in SYMBOLS:
        assert s in capi.prototypes(), s
    assert capi.CERT == {"cost": 1, "res": 2, "grad": 4, "costate": 8}
    for cls, names in ((capi.Solver, ("certificate", "device_certificate")), (capi.Group, ("certificate",))):
        for nm in names:
            assert callable(getattr(cls, nm)), (cls, nm)
    assert callable(pkg.controller.certificate)
    # the mask: -grad at the inputs at a bound, positive at umax
    g = np.array([[[1.0, -2.0, 3.0]]]); u = np.array([[[-1.0, 1.0, 0.2]]])
    mu = capi.multipliers(g, u, [-1.0], [1.0], 1e-9)
    assert np.array_equal(mu, np.array([[[-1.0, 2.0, 0.0]]]))
