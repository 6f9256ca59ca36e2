"""GPU tests of k_sens_face (csrc/almpc_sens.hip.h): almpc_sensitivity_stagewise, almpc_sensitivity_stagewise_vjp and their group forms
on ALMPC_FLAG_STRUCTURED handles.

Reference per instance: tests/sens_face_ref.py (the Riccati recursion on the face, numpy FP64) evaluated at the handle's OWN returned u
under the contract's active-set rule, so both sides differentiate the same face.  Tolerance per case: ten times the gap of that
restatement to the direct form on the CPU (sens_face_cases.GAP, tests/test_sens_face_restatement.py), not below 1e-13, of
max(1, max|J_i|) for K0, dU, dX and of sens_ref.vjp_scale for the VJP.  The designs are given the oracle's terminal weight P, so that
the device and the restatement start the recursion from the same matrix.  Every case prints its worst figure.
"""
import functools

import numpy as np
import pytest

import sens_face_cases as fc
import sens_face_gpu as fg
import sens_face_ref as fr
import sens_ref as sr
from sens_face_gpu import ERR_INVALID, ERR_UNSUPPORTED, K_SENS_RTOL, flat

pytestmark = pytest.mark.gpu

solve = functools.partial(fg.solve, cases=fc, batched_S=False)
_refused = functools.partial(fg.refused, jac="sensitivity_stagewise", vjp="sensitivity_stagewise_vjp")


@functools.lru_cache(maxsize=None)
def device(capi, name):
    """One solve of a case on a structured handle and every sensitivity call on it, shared by the tests below (read-only)."""
    s = solve(capi, name)
    res = s.get_results()
    sens = s.sensitivity_stagewise()
    g_u, g_x = fc.loss(name)
    g_x0, vrows = s.sensitivity_stagewise_vjp(g_u, g_x)
    a0 = s.sensitivity_stagewise_vjp(g_u, None)
    a1 = s.sensitivity_stagewise_vjp(g_u, np.zeros_like(g_x))
    s.close()
    return dict(res=res, sens=sens, g_u=g_u, g_x=g_x, g_x0=g_x0, vrows=vrows, null=a0, zeros=a1)


@pytest.mark.parametrize("name", fc.NAMES)
def test_jacobians_of_every_case(capi, name):
    d = device(capi, name)
    res, sens = d["res"], d["sens"]
    assert np.all(res["status"] == 0), np.bincount(res["status"])
    tol = fc.gpu_tol(name)
    worst, rows = 0.0, []
    for i in fc.instances(name):
        p = fc.problem_of(name, i)
        u = res["u"][i]
        dist = fr.distance_to_bounds(u, p.u_min, p.u_max)
        assert not np.any((dist > fc.BAND[0]) & (dist < fc.BAND[1])), (i, dist[(dist > fc.BAND[0]) & (dist < fc.BAND[1])])
        act = fr.active_rows(u, p.u_min, p.u_max)
        rows.append(int(act.sum()))
        assert sens["rows"][i] == act.sum(), (i, sens["rows"][i], act.sum())
        J, dX = fr.jacobians(p.A, p.B, p.Q, p.R, p.P, act, p.N)
        K0, dU = sr.shaped(J, p.m, p.N)
        sj, sx = max(1.0, np.abs(J).max()), max(1.0, np.abs(dX).max())
        roll = sr.dx_from_du(p.A, p.B, flat(sens["dU"][i]), p.N)
        for got, ref, scale in ((sens["K0"][i], K0, sj), (sens["dU"][i], dU, sj), (sens["dX"][i], dX, sx), (sens["dX"][i], roll, sx)):
            err = np.abs(got - ref).max() / scale
            worst = max(worst, err)
            assert err <= tol, (i, err, tol)
        assert np.ascontiguousarray(sens["K0"][i]).tobytes() == np.ascontiguousarray(sens["dU"][i][:, 0, :]).tobytes(), i
        assert np.array_equal(sens["dX"][i][:, 0, :], np.eye(p.n))
    print(f"{name}: rows {min(rows)} .. {max(rows)}, worst error / scale {worst:.3e} (tolerance {tol:g})")
    assert 0 < sum(rows) < len(rows) * res["u"][0].size, "the batch must hold free and clamped rows"
    if name in fc.TIER_NAMES:
        assert max(rows) > 32


@pytest.mark.parametrize("name", fc.NAMES)
def test_vjp_of_every_case(capi, name):
    d = device(capi, name)
    res, sens, tol = d["res"], d["sens"], fc.gpu_tol(name)
    assert np.array_equal(d["vrows"], sens["rows"])
    worst = 0.0
    for i in fc.instances(name):
        p = fc.problem_of(name, i)
        act = fr.active_rows(res["u"][i], p.u_min, p.u_max)
        ref = fr.vjp(p.A, p.B, p.Q, p.R, p.P, act, d["g_u"][i], d["g_x"][i])
        own = sr.vjp_from_jacobians(sens["dU"][i], sens["dX"][i], d["g_u"][i], d["g_x"][i])
        scale = sr.vjp_scale(ref)
        for other in (ref, own):
            err = np.abs(d["g_x0"][i] - other).max() / scale
            worst = max(worst, err)
            assert err <= tol, (i, err, tol)
    print(f"{name}: VJP worst error / scale {worst:.3e} (tolerance {tol:g})")
    (a0, r0), (a1, r1) = d["null"], d["zeros"]
    assert a0.tobytes() == a1.tobytes() and np.array_equal(r0, r1)
    assert np.abs(a0).max() > 0


def test_two_independent_kernels_on_the_quadrotor(capi):
    """k_sens_face on the structured handle against k_sens on a condensed handle: same problem, same x0, nothing shared but the data."""
    name = "quad-30"
    d = device(capi, name)
    s = solve(capi, name, structured=False)
    res = s.get_results()
    assert np.all(res["status"] == 0)
    sens = s.sensitivity()
    g_x0, vrows = s.sensitivity_vjp(d["g_u"], d["g_x"])
    s.close()
    tol = K_SENS_RTOL + fc.gpu_tol(name)
    assert np.array_equal(sens["rows"], d["sens"]["rows"]) and np.array_equal(vrows, d["vrows"])
    worst = 0.0
    for i in range(res["u"].shape[0]):
        sj, sx = max(1.0, np.abs(sens["dU"][i]).max()), max(1.0, np.abs(sens["dX"][i]).max())
        for k, scale in (("K0", sj), ("dU", sj), ("dX", sx)):
            worst = max(worst, np.abs(sens[k][i] - d["sens"][k][i]).max() / scale)
        worst = max(worst, np.abs(g_x0[i] - d["g_x0"][i]).max() / sr.vjp_scale(g_x0[i]))
    print(f"k_sens_face against k_sens on the quadrotor at N = 30: worst difference / scale {worst:.3e} (tolerance {tol:g})")
    assert worst <= tol


@pytest.mark.parametrize("name, picked", [("2-2-9", None), ("quad-50", (0, 9))])
def test_first_move_gain_against_differences_of_the_device_solution(capi, name, picked):
    ps, X0, _ = fc.case(name)
    s = solve(capi, name)
    K0 = s.sensitivity_stagewise(("K0",))["K0"]
    h = 1e-6
    fd = np.zeros_like(K0)
    for c in range(ps.n):
        e = np.zeros(ps.n); e[c] = h
        u = []
        for sgn in (1.0, -1.0):
            s.update_initialization(X0 + sgn * e)
            s.calculate()
            assert np.all(s.get_results()["status"] == 0)
            u.append(s.get_first_input())
        fd[:, :, c] = (u[0] - u[1]) / (2 * h)
    s.close()
    idx = list(range(X0.shape[0])) if picked is None else list(picked)
    err = max(np.abs(K0[i] - fd[i]).max() / max(1.0, np.abs(K0[i]).max()) for i in idx)
    print(f"{name}: K0 against central differences of the device's own u[:,1]: {err:.3e}")
    assert err <= 1e-6
    assert np.any(K0[idx] != 0.0)


def test_unsolved_instances_get_minus_one_and_zeros(capi, monkeypatch):
    """k_sdual hands what its cap leaves undecided to k_riccati, which has its own: on such a handle no polish_max_iter produces an
    unsolved instance.  Under ALMPC_STRUCTURED_PRIMAL k_riccati is the only solver and the cap is its own: at 8 working-set changes
    it leaves part of the quadrotor batch unsolved.

    The zeros and rows = -1 are written by sens_face_unsolved (csrc/almpc_sens.hip.h), the one epilogue of k_sens_face and
    k_sens_face_rate, so this test is also the test of the rate kernel's failure path.  It has no twin on a design with S: under
    ALMPC_STRUCTURED_PRIMAL the design of a structured handle refuses an input-rate weight ("state rows / input-rate weight need
    the stage-wise dual solve": setup_structured_solvers, csrc/almpc_api.hip), so these means leave no unsolved instance there."""
    name = "quad-30"
    monkeypatch.setenv("ALMPC_STRUCTURED_PRIMAL", "1")
    full = solve(capi, name)
    capped = solve(capi, name, capi.default_opts(polish_max_iter=8))
    monkeypatch.delenv("ALMPC_STRUCTURED_PRIMAL", raising=False)
    g_u, g_x = fc.loss(name)
    out = []
    for s in (full, capped):
        r = s.get_results()
        sens = s.sensitivity_stagewise()
        sens["g_x0"], sens["vrows"] = s.sensitivity_stagewise_vjp(g_u, g_x)
        sens["status"] = r["status"]
        s.close()
        out.append(sens)
    a, b = out
    assert np.all(a["status"] == 0)
    bad, good = np.nonzero(b["status"] != 0)[0], np.nonzero(b["status"] == 0)[0]
    assert bad.size >= 1 and good.size >= 1, np.bincount(b["status"])
    for i in bad:
        assert b["rows"][i] == -1 and b["vrows"][i] == -1
        assert not b["K0"][i].any() and not b["dU"][i].any() and not b["dX"][i].any() and not b["g_x0"][i].any()
    for i in good:
        for k in ("K0", "dU", "dX", "g_x0", "rows", "vrows"):
            assert np.ascontiguousarray(a[k][i]).tobytes() == np.ascontiguousarray(b[k][i]).tobytes(), (i, k)
    print(f"{bad.size} unsolved of {b['status'].size}")


def test_refusals(capi, mo):
    p = mo.double_integrator(N=10)
    X0 = 0.5 * np.random.default_rng(1).normal(size=(4, 2))
    gu, gx0 = np.zeros((4, 10, 1)), np.zeros((4, 2))
    ptr = lambda a: a.ctypes.data_as(capi._dp)
    # a condensed handle: almpc_sensitivity serves it
    s = capi.Solver(2, 1, 10, 4)
    s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    s.update_initialization(X0); s.calculate()
    _refused(capi, s)
    assert b"almpc_sensitivity" in s.L.almpc_last_error(s.h)
    s.close()
    # S != 0, a state box, the terminal equality
    for kw in (dict(S=0.5 * np.eye(1)), dict(xmin=[-50.0, -50.0], xmax=[50.0, 50.0]), dict(terminal="equality")):
        s = capi.Solver(2, 1, 10, 4, structured=True)
        s.design_shared(p.A, p.B, p.Q, p.R, kw.pop("S", None), None, p.u_min, p.u_max, **kw)
        s.update_initialization(0.1 * X0); s.calculate()
        _refused(capi, s)
        s.close()
    s = capi.Solver(2, 1, 10, 4, structured=True)
    s.design_shared(p.A, p.B, p.Q, p.R, None, None, p.u_min, p.u_max)
    _refused(capi, s, ERR_INVALID)   # before the first step
    s.update_initialization(X0); s.calculate()
    # bad want, NULL pointers
    assert s.L.almpc_sensitivity_stagewise(s.h, 0, 0.0) == ERR_INVALID and s.L.almpc_sensitivity_stagewise(s.h, 8, 0.0) == ERR_INVALID
    assert s.L.almpc_sensitivity_stagewise_vjp(s.h, None, None, 0.0, ptr(gx0), None) == ERR_INVALID
    assert s.L.almpc_sensitivity_stagewise_vjp(s.h, ptr(gu), None, 0.0, None, None) == ERR_INVALID
    assert s.L.almpc_get_sensitivity(s.h, None, None, None, None) == ERR_INVALID   # nothing computed yet
    # the calls of condensed handles still refuse a structured one
    for call in (lambda: s.sensitivity(("K0",)), lambda: s.sensitivity_vjp(np.zeros((4, 1, 10))), lambda: s.sensitivity_rows(("K0",)),
                 lambda: s.sensitivity_params_vjp(np.zeros((4, 1, 10)), want=("x0",))):
        with pytest.raises(capi.AlmpcError) as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED, e.value
    s.sensitivity_stagewise(("K0",))
    s.design_shared(p.A, p.B, p.Q, p.R, None, None, p.u_min, p.u_max)   # a new design: no step of it yet
    _refused(capi, s, ERR_INVALID)
    s.close()


def test_a_call_disturbs_nothing_and_a_group_equals_one_handle(capi):
    name = "9-4-12"
    ps, X0, _ = fc.case(name)
    g_u, g_x = fc.loss(name)
    twins = [solve(capi, name) for _ in range(2)]
    before = twins[0].get_results()
    sens = twins[0].sensitivity_stagewise()
    again = twins[0].L.almpc_get_sensitivity   # (what the call returned is what almpc_get_sensitivity hands out afterwards)
    got = capi._sens_read(again, twins[0].h, twins[0]._check, ("K0", "dU", "dX"), twins[0].batch, ps.n, ps.m, ps.N)
    for k in ("K0", "dU", "dX", "rows"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(sens[k]).tobytes(), k
    k0_only = twins[0].sensitivity_stagewise(("K0",))
    assert np.ascontiguousarray(k0_only["K0"]).tobytes() == np.ascontiguousarray(sens["K0"]).tobytes()
    sens["g_x0"], sens["vrows"] = twins[0].sensitivity_stagewise_vjp(g_u, g_x)
    after = twins[0].get_results()
    for k in ("x", "e_x", "u", "e_u", "status"):
        assert before[k].tobytes() == after[k].tobytes(), k
    out = []
    for s in twins:
        s.update_initialization(X0 + 0.01)
        s.calculate(capi.default_opts(warm_start=1))
        out.append(s.get_results())
        s.close()
    for k in ("x", "e_x", "u", "e_u", "status", "iters", "polish_iters"):
        assert out[0][k].tobytes() == out[1][k].tobytes(), k
    g = solve(capi, name, make=lambda: capi.Group(ps.n, ps.m, ps.N, X0.shape[0], devices=[0, 0], structured=True))
    gs = g.sensitivity_stagewise()
    gs["g_x0"], gs["vrows"] = g.sensitivity_stagewise_vjp(g_u, g_x)
    g.close()
    assert sens["rows"].max() > 0
    for k in ("K0", "dU", "dX", "g_x0", "rows", "vrows"):
        assert np.ascontiguousarray(sens[k]).tobytes() == np.ascontiguousarray(gs[k]).tobytes(), k
