"""The restatement of the certificate of a time-varying design (tests/cert_ltv_ref.py) against the design's QP (oracle/mpc_oracle.py::
ltv_qp), on the CPU, on every case of tests/cert_ltv_cases.py and every instance, at the exact optimum v* and at a random feasible v:
the stacked gradient is H v + q, the cost is the QP's objective up to J(0), the predicted states are xbar + Gam v + g, each within the
rounding bounds of both sides; with time-invariant stages every value is cert_ref.certificate's; lam_{k+1} is the derivative of J in
c_k; the residual vanishes at v*.  Also: the header declares the entry points and the Python binding and the Julia shim have them."""
import os
import re

import numpy as np
import pytest

import cert_ltv_cases as lc
import cert_ltv_ref as lr
import cert_ref as cr
import mpc_oracle as mo
from conftest import ROOT

SYMBOLS = ("almpc_set_keep_stage_models", "almpc_certificate_ltv", "almpc_get_certificate_ltv", "almpc_device_certificate_ltv",
           "almpc_relin_fnn_certificate", "almpc_group_relin_fnn_certificate")


def _points(name, i):
    """(v*, a random feasible v) of instance i, flat [N][m]"""
    p = lc.qp(name, i)
    rng = np.random.default_rng(1000 * len(name) + i)
    return p["v"], p["lo"] + rng.random(p["lo"].size) * (p["hi"] - p["lo"])


def _cert(name, i, vflat):
    k, ubar = lc.instance(name, i)
    m, N = ubar.shape
    v = vflat.reshape(N, m).T
    return lr.certificate_ltv(v=v, u=ubar + v, **k)


@pytest.mark.parametrize("name", lc.NAMES)
def test_recursion_equals_the_designs_qp(name):
    n, m, N = lc.shape(name)
    for i in range(4):
        k, ubar = lc.instance(name, i)
        p = lc.qp(name, i)
        useR, useS = cr.branch(k["R"], k["S"])
        qb = lr.qp_bound(mo, k["A"], k["B"], k["c"], k["xbar"], ubar, k["xref"], k["uref"], k["Q"], k["R"], k["S"], k["P"], k["umin"], k["umax"],
                         useR, useS)
        j0 = _cert(name, i, np.zeros(m * N))
        for v in _points(name, i):
            r = _cert(name, i, v)
            av = np.abs(v)
            # grad = H v + q
            g = (p["H"] @ v + p["q"]).reshape(N, m).T
            tol_g = 0.5 * r["tol_grad"] + cr.gamma(qb["ops"]) * (qb["H"] @ av + qb["q"]).reshape(N, m).T   # (one side each)
            assert np.all(np.abs(r["grad"] - g) <= tol_g), (name, i, float(np.max(np.abs(r["grad"] - g) / tol_g)))
            # J(v) - J(0) = 1/2 v'Hv + q'v
            dj = 0.5 * float(v @ p["H"] @ v) + float(p["q"] @ v)
            tol_j = 0.5 * (r["tol_cost"] + j0["tol_cost"]) + 2.0 ** -52 * (r["mag_cost"] + j0["mag_cost"]) \
                + cr.gamma(qb["ops"] + m * N + 2) * (0.5 * float(av @ qb["H"] @ av) + float(qb["q"] @ av))
            assert abs((r["cost"] - j0["cost"]) - dj) <= tol_j, (name, i, abs((r["cost"] - j0["cost"]) - dj) / tol_j)
            # x - xbar = Gam v + g (the difference x - xbar rounds once more, a number no larger than |x| + |xbar|)
            dx = (p["Gam"] @ v + p["g"]).reshape(N, n).T
            tol_x = 0.5 * r["tol_x"][:, 1:] + 2.0 ** -53 * (r["mag_x"][:, 1:] + np.abs(k["xbar"][:, 1:])) \
                + cr.gamma(qb["ops"]) * (qb["Gam"] @ av + qb["g"]).reshape(N, n).T
            err = np.abs((r["x"] - k["xbar"])[:, 1:] - dx)
            assert np.all(err <= tol_x), (name, i, float(np.max(err / np.maximum(tol_x, 1e-300))))
            assert np.array_equal(r["x"][:, 0], k["xbar"][:, 0])
            assert np.array_equal(r["e_x"], r["x"] - (0.0 if k["xref"] is None else k["xref"]))


@pytest.mark.parametrize("name", lc.NAMES)
def test_time_invariant_stages_give_the_certificate_of_the_lti_design(name):
    """A_k = A, B_k = B, c = 0, xbar the linear rollout of ubar: the backward sweep is cert_ref.certificate's at the same trajectories
    (its e_u is u - uref), and x is the rollout of u from xbar_0."""
    n, m, N = lc.shape(name)
    for i in range(4):
        k, ubar = lc.instance(name, i)
        A, B = k["A"][0], k["B"][0]
        xbar = np.zeros((n, N + 1)); xbar[:, 0] = k["xbar"][:, 0]
        for s in range(N):
            xbar[:, s + 1] = A @ xbar[:, s] + B @ ubar[:, s]
        kk = dict(k, A=np.broadcast_to(A, (N, n, n)), B=np.broadcast_to(B, (N, n, m)), c=None, xbar=xbar)
        for vflat in _points(name, i):
            v = vflat.reshape(N, m).T
            u = ubar + v
            r = lr.certificate_ltv(v=v, u=u, **kk)
            uref = np.zeros((m, N)) if k["uref"] is None else k["uref"]
            t = cr.certificate(A, B, k["Q"], k["R"], k["S"], k["P"], k["umin"], k["umax"], r["e_x"], u - uref, u)
            for key in ("grad", "costate"):
                tol = 0.5 * (r["tol_" + key] + t["tol_" + key])
                assert np.all(np.abs(r[key] - t[key]) <= tol), (name, i, key)
            assert abs(r["cost"] - t["cost"]) <= 0.5 * (r["tol_cost"] + t["tol_cost"]), (name, i)
            assert abs(r["res"] - t["res"]) <= 0.5 * (r["tol_res"] + t["tol_res"]), (name, i)
            # the rollout of u: x_{s+1} = A x_s + B u_s, at most ops_x roundings on the same magnitudes plus those of xbar's own rollout
            x = np.zeros((n, N + 1)); x[:, 0] = xbar[:, 0]
            mx = np.abs(x)
            for s in range(N):
                x[:, s + 1] = A @ x[:, s] + B @ u[:, s]
                mx[:, s + 1] = np.abs(A) @ mx[:, s] + np.abs(B) @ np.abs(u[:, s])
            tol = 0.5 * r["tol_x"] + 3.0 * lr.tol_of(r["ops_x"], mx + r["mag_x"])
            assert np.all(np.abs(r["x"] - x) <= tol), (name, i, float(np.max(np.abs(r["x"] - x) / np.maximum(tol, 1e-300))))


@pytest.mark.parametrize("name", lc.NAMES)
def test_costates_are_the_derivative_of_the_cost_in_the_defects(name):
    """lam_{k+1} = dJ/dc_k at fixed v: J is quadratic in c, so the central difference (any step: 1 here) is exact up to rounding."""
    n, m, N = lc.shape(name)
    i = len(name) % 4
    k, ubar = lc.instance(name, i)
    c0 = np.zeros((N, n)) if k["c"] is None else k["c"]
    for vflat in _points(name, i):
        v = vflat.reshape(N, m).T
        r = lr.certificate_ltv(v=v, u=ubar + v, **k)
        for s in range(N):
            for j in range(n):
                J = []
                for sgn in (1.0, -1.0):
                    c = c0.copy(); c[s, j] += sgn
                    J.append(lr.certificate_ltv(v=v, u=ubar + v, **dict(k, c=c)))
                fd = (J[0]["cost"] - J[1]["cost"]) / 2.0
                tol = 0.25 * (J[0]["tol_cost"] + J[1]["tol_cost"]) + 2.0 ** -53 * (J[0]["mag_cost"] + J[1]["mag_cost"]) + 0.5 * r["tol_costate"][j, s + 1]
                assert abs(fd - r["costate"][j, s + 1]) <= tol, (name, s, j, abs(fd - r["costate"][j, s + 1]) / tol)


@pytest.mark.parametrize("name", lc.NAMES)
def test_residual_vanishes_at_the_exact_optimum(name):
    for i in range(4):
        p = lc.qp(name, i)
        assert np.linalg.eigvalsh(p["H"]).min() > 0.0, (name, i)
        r = _cert(name, i, p["v"])
        assert r["res"] <= lc.QUAD_NOISE_SHARE * 1e-9 * max(1.0, float(np.max(np.abs(r["grad"])))), (name, i, r["res"])


def test_nonfinite_input_gives_nonfinite_outputs():
    k, ubar = lc.instance("4-2-N3-b4", 0)
    v = np.zeros_like(ubar); v[0, 0] = np.nan
    r = lr.certificate_ltv(v=v, u=ubar + v, **k)
    assert np.isnan(r["cost"]) and np.isnan(r["res"]) and np.isnan(r["costate"][:, 0]).all() and np.isnan(r["x"][:, 1:]).all()


def test_header_declares_the_entry_points_and_the_bindings_have_them(pkg):
    with open(os.path.join(ROOT, "include", "almpc.h")) as f:
        header = f.read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
    assert re.search(r"#define ALMPC_CERT_STATES 16u\b", header)
    capi = pkg._capi
    with open(os.path.join(ROOT, "julia", "AlmpcHIP.jl")) as f:
        shim = f.read()
    for s in SYMBOLS:
        assert s in capi.prototypes(), s
        assert "(:%s, libalmpc)" % s in shim, s
    assert capi.CERT_LTV == {"cost": 1, "res": 2, "grad": 4, "costate": 8, "x": 16, "e_x": 16}
    for cls, names in ((capi.Solver, ("set_keep_stage_models", "certificate_ltv", "device_certificate_ltv", "relin_fnn_certificate")),
                       (capi.Group, ("relin_fnn_certificate",))):
        for nm in names:
            assert callable(getattr(cls, nm)), (cls, nm)
