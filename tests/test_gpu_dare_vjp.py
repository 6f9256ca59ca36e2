"""GPU tests of k_dare_vjp (csrc/almpc_dare_vjp.hip.h): the batched entry point almpc_dare_vjp_batched against the scipy-Lyapunov form of
tests/dare_vjp_ref.py, and almpc_sensitivity_params_vjp_dare (terminal="dare") on shared and per-instance designs.

Tolerances.  The kernel against the Lyapunov form on the same inputs: 1e-9 of max(1, max|group|) per instance and group, the relative
bound the project holds k_dare to (the doubling restatement's measured gap on these inputs is <= 1.1e-13: tests/test_dare_vjp_host.py).
The handle path: "dare" = "data" + the Lyapunov form applied to the library's own A_i, B_i, P_i and returned P group, per group within
sens_params_cases.gpu_tol(case) + 1e-9 of the group's scale; everything the DARE does not reach has the bits of "data".  The whole
stack: central differences of the device's own designs (P = NULL: every perturbed design takes its own DARE) and steps, h = 1e-6,
1e-5 of max(1, |value|), as tests/test_gpu_sensitivity_params.py.
"""
import ctypes
import dataclasses
import importlib

import numpy as np
import pytest
import scipy.linalg as sla

import dare_vjp_ref as dv
import sens_params_cases as pc
import sens_params_ref as pr
from test_gpu_dare import bad_model, random_models

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_NUMERIC = -1, -4, -6
FD_H, FD_RTOL = 1e-6, 1e-5
SHAPES = [(1, 1), (2, 1), (4, 2), (12, 4), (16, 16), (17, 3), (32, 8), (33, 3), (48, 16)]
SENTINEL = -12345.678
SQRT5 = np.sqrt(5.0)
CHAINED = ("Q", "R", "A", "B")


def _gp(seed, b, n):
    g = np.random.default_rng(seed).standard_normal((b, n, n))
    return 0.5 * (g + g.transpose(0, 2, 1))


def check_against_lyapunov(label, got, st, A, B, Q, R, P, gP):
    assert np.all(st == 0), np.nonzero(st)[0]
    worst, where = 0.0, ""
    for i in range(A.shape[0]):
        gap, k = dv.worst_gap({k: got[k][i] for k in dv.GROUPS}, dv.dare_vjp_lyap(A[i], B[i], Q, R, P[i], gP[i]))
        if gap > worst:
            worst, where = gap, f"{k} of instance {i}"
    print(f"{label}: worst gap to the Lyapunov form {worst:.3e} ({where})")
    assert worst <= dv.RTOL
    for k in ("Q", "R"):
        assert np.array_equal(got[k], got[k].transpose(0, 2, 1)), k   # symmetric bit for bit


@pytest.mark.parametrize("n,m", SHAPES)
def test_batched_entry_point_matches_the_lyapunov_form(capi, n, m):
    A, B, Q, R = random_models(n, m, 67)
    P, stp = capi.dare_batched(A, B, Q, R)
    assert np.all(stp == 0)
    gP = _gp(4000 + n, 67, n)
    got, st = capi.dare_vjp_batched(A, B, Q, R, P, gP)
    check_against_lyapunov(f"n {n} m {m}", got, st, A, B, Q, R, P, gP)


def test_slow_closed_loops(capi):
    models = [dv.slow_mode_model(lam) for lam in (0.999, 0.9999)]
    A, B = np.stack([mdl[0] for mdl in models]), np.stack([mdl[1] for mdl in models])
    Q, R = models[0][2], models[0][3]
    P, stp = capi.dare_batched(A, B, Q, R)
    assert np.all(stp == 0)
    gP = _gp(5, 2, 4)
    got, st = capi.dare_vjp_batched(A, B, Q, R, P, gP)
    check_against_lyapunov("slow modes 0.999, 0.9999", got, st, A, B, Q, R, P, gP)


def test_status_cases_and_limits(capi):
    one = np.ones((1, 1, 1))
    # the anti-stabilising root of a = 2, b = q = r = 1 solves the equation; its closed loop is 2.618
    for root, want in ((2.0 - SQRT5, 2), (2.0 + SQRT5, 0)):
        got, st = capi.dare_vjp_batched(2.0 * one, one, one[0], one[0], root * one, one)
        assert st[0] == want, (root, st)
        assert np.isnan(got["Q"][0, 0, 0]) == (want != 0)
    # a P that does not solve the equation
    A, B, Q, R = random_models(4, 2, 5)
    P, _ = capi.dare_batched(A, B, Q, R)
    P2 = P.copy()
    P2[2] *= 1.001
    got, st = capi.dare_vjp_batched(A, B, Q, R, P2, _gp(1, 5, 4))
    assert st.tolist() == [0, 0, 3, 0, 0] and np.all(np.isnan(got["A"][2])) and not np.isnan(got["A"][[0, 1, 3, 4]]).any()
    # singular R, the limits
    with pytest.raises(capi.AlmpcError) as e:
        capi.dare_vjp_batched(A, B, Q, np.array([[1.0, 2.0], [2.0, 4.0]]), P, _gp(1, 5, 4))
    assert e.value.code == ERR_NUMERIC
    for n, m in ((49, 2), (4, 17)):
        A, B, Q, R = random_models(n, m, 3)
        with pytest.raises(capi.AlmpcError) as e:
            capi.dare_vjp_batched(A, B, Q, R, np.tile(np.eye(n), (3, 1, 1)), _gp(1, 3, n))
        assert e.value.code == ERR_UNSUPPORTED


def test_failing_instances_are_reported_and_leave_the_others_alone(capi):
    A, B, Q, R = random_models(4, 2, 40)
    P, _ = capi.dare_batched(A, B, Q, R)
    gP = _gp(2, 40, 4)
    A2, B2, P2 = A.copy(), B.copy(), P.copy()
    A2[3], B2[3] = bad_model()          # no solution at all: any P is refused
    P2[17] = 1.001 * P[17]              # not the solution of this model
    init = {"A": np.full((40, 4, 4), SENTINEL), "B": np.full((40, 4, 2), SENTINEL), "Q": np.full((40, 4, 4), SENTINEL),
            "R": np.full((40, 2, 2), SENTINEL)}
    good, stg = capi.dare_vjp_batched(A, B, Q, R, P, gP, init=init)
    got, st = capi.dare_vjp_batched(A2, B2, Q, R, P2, gP, init=init)
    assert np.all(stg == 0)
    assert sorted(np.nonzero(st)[0].tolist()) == [3, 17]
    keep = np.ones(40, dtype=bool)
    keep[[3, 17]] = False
    for k in dv.GROUPS:
        assert np.all(got[k][~keep] == SENTINEL), k          # a refused instance's slots are not written
        assert np.array_equal(got[k][keep], good[k][keep]), k  # bit-identical: no instance depends on its neighbours


# ---- almpc_sensitivity_params_vjp_dare ------------------------------------------------------------------------------------------------

def _loss(seed, b, p):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(b, p.m, p.N)), rng.normal(size=(b, p.n, p.N + 1))


def solve_shared(capi, p, X0, P=None, opts=None, **kw):
    sv = capi.Solver(p.n, p.m, p.N, X0.shape[0], **kw)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, P, p.u_min, p.u_max)
    sv.set_reference(p.x_ref, p.u_ref)
    sv.update_initialization(X0)
    sv.calculate(opts)
    return sv


def _same_bits(a, b, keys):
    for k in keys:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k


def check_chain(name, sv, data, dare, Q, R):
    """dare = data + the Lyapunov form of the library's own A_i, B_i, P_i and returned P group, on Q, R, A, B; the rest has data's bits."""
    assert np.all(dare["dare_status"] == 0), dare["dare_status"]
    _same_bits(data, dare, [k for k in pr.GROUPS if k not in CHAINED] + ["rows"])
    tol = pc.gpu_tol(name) + dv.RTOL
    worst = dict.fromkeys(CHAINED, 0.0)
    moved = 0.0
    for i in range(sv.batch):
        A, B = sv.model_instance(i)
        ref = dv.dare_vjp_lyap(A, B, Q, R, sv.terminal_weight_instance(i), data["P"][i])
        for k in CHAINED:
            want = data[k][i] + ref[k]
            worst[k] = max(worst[k], float(np.abs(dare[k][i] - want).max()) / pr.group_scale(want))
        moved = max(moved, float(np.abs(ref["Q"]).max()))
    print(f"{name}: worst error of the chained groups: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items())
          + f"; tolerance {tol:g}; largest DARE term in dL/dQ {moved:.3g}")
    assert max(worst.values()) <= tol, worst
    assert moved > 0.0


def test_shared_design_with_its_own_dare(capi, mo):
    p, X0 = pc.case(mo, "di")
    sv = solve_shared(capi, p, X0)   # P = NULL: the design's own DARE
    assert np.all(sv.get_results()["status"] == 0)
    g_u, g_x = _loss(41, len(X0), p)
    data = sv.sensitivity_params_vjp(g_u, g_x)
    dare = sv.sensitivity_params_vjp(g_u, g_x, terminal="dare")
    check_chain("di", sv, data, dare, p.Q, p.R)
    # without out->P the library makes the P group itself: the same bits; only what is asked for comes back
    part = sv.sensitivity_params_vjp(g_u, g_x, want=("Q", "B", "u_max"), terminal="dare")
    assert sorted(part) == ["B", "Q", "dare_status", "rows", "u_max"]
    _same_bits(part, dare, ("Q", "B", "u_max"))
    sv.close()


def test_per_instance_models_with_device_dares(capi, mo):
    ps, X0 = pc.problems(mo, "quadfam")
    b = len(X0)
    sv = capi.Solver(12, 4, 10, b)
    sv.set_terminal_weight("dare_device")
    sv.design_batched(np.stack([p.A for p in ps]), np.stack([p.B for p in ps]), ps[0].Q, ps[0].R, None, None, pc.QUAD_UMIN, pc.QUAD_UMAX)
    sv.update_initialization(X0)
    sv.calculate()
    assert np.all(sv.get_results()["status"] == 0)
    g_u, g_x = _loss(43, b, ps[0])
    data = sv.sensitivity_params_vjp(g_u, g_x)
    dare = sv.sensitivity_params_vjp(g_u, g_x, terminal="dare")
    check_chain("quadfam", sv, data, dare, ps[0].Q, ps[0].R)
    sv.close()


def test_whole_stack_against_differences_of_the_devices_own_designs(capi, mo):
    """dL/dQ, dL/dR, dL/dA with the DARE followed, each contracted with one direction, against central differences of the device's
    own designs (P = NULL: every perturbed design recomputes its DARE) and steps; h = 1e-6, bound 1e-5 of max(1, |value|)."""
    p, X0 = pc.case(mo, "di")
    g_u, g_x = _loss(47, len(X0), p)
    sv = solve_shared(capi, p, X0)
    got = sv.sensitivity_params_vjp(g_u, g_x, want=("Q", "R", "A"), terminal="dare")
    data = sv.sensitivity_params_vjp(g_u, g_x, want=("Q", "R", "A"))
    sv.close()
    assert np.all(got["dare_status"] == 0)

    def total_loss(**change):
        s2 = solve_shared(capi, dataclasses.replace(p, **change), X0)
        r = s2.get_results()
        s2.close()
        assert np.all(r["status"] == 0)
        return float((g_u * r["u"]).sum() + (g_x * r["x"]).sum())

    rng = np.random.default_rng(53)
    sym = lambda M: 0.5 * (M + M.T)
    dirs = {"Q": sym(rng.normal(size=(2, 2))), "R": sym(rng.normal(size=(1, 1))), "A": rng.normal(size=(2, 2))}
    errs = {}
    for k, D in dirs.items():
        base = getattr(p, k)
        fd = (total_loss(**{k: base + FD_H * D}) - total_loss(**{k: base - FD_H * D})) / (2 * FD_H)
        val = float((got[k].sum(axis=0) * D).sum())   # (a shared design: the caller sums over the batch)
        as_data = float((data[k].sum(axis=0) * D).sum())
        errs[k] = abs(val - fd) / max(1.0, abs(val))
        print(f"dL/d{k} . direction: {val:.9g} (P as data: {as_data:.9g}), central differences of the device's designs and steps {fd:.9g}, "
              f"error {errs[k]:.2e}")
    assert max(errs.values()) <= FD_RTOL, errs


def test_a_given_weight_that_is_no_dare_solution_is_reported(capi, mo):
    p, X0 = pc.case(mo, "di")
    sv = solve_shared(capi, p, X0, P=2.0 * p.P)
    solved = sv.get_results()["status"] == 0
    assert solved.all()
    g_u, g_x = _loss(41, len(X0), p)
    data = sv.sensitivity_params_vjp(g_u, g_x)
    dare = sv.sensitivity_params_vjp(g_u, g_x, terminal="dare")
    assert np.all(dare["dare_status"][solved] != 0), dare["dare_status"]
    _same_bits(data, dare, pr.GROUPS + ("rows",))
    # without dare_status the call fails, names the lowest instance and copies nothing out
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    gu = np.ascontiguousarray(g_u.transpose(0, 2, 1))
    Qout = np.full((len(X0), 2, 2), SENTINEL)
    out = capi.almpc_param_grads(Q=dp(Qout))
    assert sv.L.almpc_sensitivity_params_vjp_dare(sv.h, dp(gu), None, 0.0, ctypes.byref(out), None) == ERR_NUMERIC
    assert "instance 0 " in sv.L.almpc_last_error(sv.h).decode()
    assert np.all(Qout == SENTINEL)
    # a given P that IS the DARE solution is followed: no flag records where P came from
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, sla.solve_discrete_are(p.A, p.B, p.Q, p.R), p.u_min, p.u_max)
    sv.update_initialization(X0)
    sv.calculate()
    assert np.all(sv.sensitivity_params_vjp(g_u, g_x, want=("Q",), terminal="dare")["dare_status"] == 0)
    sv.close()


def _refused(capi, sv, code=ERR_UNSUPPORTED):
    with pytest.raises(capi.AlmpcError) as e:
        sv.sensitivity_params_vjp(np.zeros((sv.batch, sv.m, sv.N)), terminal="dare")
    assert e.value.code == code, e.value
    assert (sv.L.almpc_last_error(sv.h) or b"").decode().strip()


def test_refusals(capi, mo):
    p = mo.double_integrator(N=10)
    X0 = 0.5 * np.random.default_rng(1).normal(size=(4, 2))
    # a design that dropped R has no DARE
    sv = capi.Solver(2, 1, 10, 4)
    sv.design_shared(p.A, p.B, p.Q, np.zeros((1, 1)), p.S, p.P, p.u_min, p.u_max)
    sv.update_initialization(X0); sv.calculate()
    assert sv.sensitivity_params_vjp(np.zeros((4, 1, 10)))["rows"].shape == (4,)   # (the plain call serves it)
    _refused(capi, sv)
    sv.close()
    # the refusals of the plain call: before a step, a state box, a structured handle
    sv = capi.Solver(2, 1, 10, 4)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    _refused(capi, sv, ERR_INVALID)
    sv.close()
    sv = capi.Solver(2, 1, 10, 4)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, xmin=[-50.0, -50.0], xmax=[50.0, 50.0])
    sv.update_initialization(0.1 * X0); sv.calculate()
    _refused(capi, sv)
    sv.close()
    sv = capi.Solver(2, 1, 10, 4, structured=True)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    sv.update_initialization(X0); sv.calculate()
    _refused(capi, sv)
    sv.close()


def test_unsolved_instances_get_minus_one_and_zeros(capi, mo):
    p = mo.quadrotor(N=30)
    b = 48
    X0 = mo.quadrotor_x0_batch(b, amplitude=3.0)
    sv = solve_shared(capi, p, X0, P=p.P, opts=capi.default_opts(polish_max_iter=1), structured_fallback=False)
    res = sv.get_results()
    bad, good = np.nonzero(res["status"] != 0)[0], np.nonzero(res["status"] == 0)[0]
    assert bad.size >= 1 and good.size >= 1, np.bincount(res["status"])
    g_u, g_x = _loss(59, b, p)
    data = sv.sensitivity_params_vjp(g_u, g_x)
    dare = sv.sensitivity_params_vjp(g_u, g_x, terminal="dare")
    sv.close()
    assert np.all(dare["dare_status"] == 0)
    for i in bad:
        assert dare["rows"][i] == -1
        assert not any(dare[k][i].any() for k in pr.GROUPS)
    _same_bits(data, dare, [k for k in pr.GROUPS if k not in CHAINED] + ["rows"])
    assert all(np.any(dare["Q"][i] != data["Q"][i]) for i in good)


def test_group_equals_one_handle(capi, mo):
    p, X0 = pc.case(mo, "quad_big")
    X0 = X0[:13]
    g_u, g_x = _loss(67, 13, p)
    got = []
    for make in (lambda: capi.Solver(12, 4, 30, 13), lambda: capi.Group(12, 4, 30, 13, devices=[0, 0])):
        s = make()
        s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
        s.set_reference(p.x_ref, p.u_ref)
        s.update_initialization(X0)
        s.calculate()
        got.append(s.sensitivity_params_vjp(g_u, g_x, terminal="dare"))
        s.close()
    assert np.all(got[0]["dare_status"] == 0)
    _same_bits(got[0], got[1], pr.GROUPS + ("rows", "dare_status"))


def test_a_call_disturbs_nothing(capi, mo):
    p, X0 = pc.case(mo, "quad")
    g_u, g_x = _loss(61, len(X0), p)
    twins = [solve_shared(capi, p, X0) for _ in range(2)]
    v0 = twins[0].sensitivity_vjp(g_u, g_x)
    twins[0].sensitivity_params_vjp(g_u, g_x, terminal="dare")
    v1 = twins[0].sensitivity_vjp(g_u, g_x)
    assert v0[0].tobytes() == v1[0].tobytes() and np.array_equal(v0[1], v1[1])
    first = [sv.get_results() for sv in twins]
    out = []
    for sv in twins:
        sv.update_initialization(X0 + 0.01)
        sv.calculate(capi.default_opts(warm_start=1))
        out.append(sv.get_results())
        sv.close()
    for pair in (first, out):
        _same_bits(pair[0], pair[1], ("x", "e_x", "u", "e_u", "status", "iters", "polish_iters"))


def test_controller_mirror(pkg, capi, mo):
    """sensitivity_params(C, terminal="dare") of the Python mirror is Solver.sensitivity_params_vjp(terminal="dare") of its handle."""
    p = mo.double_integrator(N=10)
    X, U = pkg.Hyperrectangle([-100.0] * 2, [100.0] * 2), pkg.Hyperrectangle(p.u_min, p.u_max)
    sys_ = pkg.ConstrainedLinearControlDiscreteSystem(p.A, p.B, X, U)
    X0 = 3.0 * np.random.default_rng(7).normal(size=(8, 2))
    g_u, g_x = _loss(71, 8, p)
    for b in (8, 1):
        C = pkg.proceed_controller(sys_, "model_predictive_control", 10, 1, [0.0, 0.0], [0.0], mpc_batch=b)
        pkg._model_predictive_control_computation(C, X0[:b])
        gu, gx = (g_u, g_x) if b > 1 else (g_u[0], g_x[0])
        got = pkg.sensitivity_params(C, gu, gx, want=("x0", "Q", "B"), terminal="dare")
        sv = C.tuning.modeler.solver
        own = sv.sensitivity_params_vjp(g_u[:b], g_x[:b], want=("x0", "Q", "B"), terminal="dare")
        data = sv.sensitivity_params_vjp(g_u[:b], g_x[:b], want=("Q",))
        assert sorted(got) == ["B", "Q", "dare_status", "rows", "x0"]
        for k, v in own.items():
            assert np.array_equal(got[k], v[0] if b == 1 else v), k
        assert np.all(own["dare_status"] == 0) and np.any(own["Q"] != data["Q"])
        sv.close()
    assert "sensitivity_params" in importlib.import_module(pkg.__name__ + ".controller").__all__
