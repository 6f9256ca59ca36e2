"""GPU tests of k_sens (csrc/almpc_sens.hip.h): almpc_sensitivity, almpc_sensitivity_vjp and their group forms.

Reference per instance: tests/sens_ref.py (the G-based form, numpy FP64) fed with H, F, d from almpc_get_design /
almpc_get_design_instance and with the handle's OWN returned u under the contract's active-set rule, so both sides differentiate the
same face.  Tolerance: 1e-8 of max(1, max|J_i|) for K0, dU, dX; 1e-8 of max(1, max|g_x0_i|) for the VJP (sens_ref.vjp_scale).  The
reference differs from the direct H_FF solve by at most 1e-9 on the CPU (tests/test_sens_restatement.py), which leaves a factor of
ten for the device's own G = H'^-1 and V = -G F'.  Every case prints its worst figure.
"""
import importlib

import numpy as np
import pytest

import sens_ref as sr
from test_gpu_batched_models import quad_family

pytestmark = pytest.mark.gpu

J_RTOL = 1e-8
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
QUAD_UMIN, QUAD_UMAX = [-2.0, -0.05, -0.05, -0.02], [3.0, 0.05, 0.05, 0.02]


def random_stable(mo, n, m, N, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    A *= 0.9 / np.max(np.abs(np.linalg.eigvals(A)))
    return mo.make_problem(A, rng.standard_normal((n, m)), N, -np.ones(m), np.ones(m))


def shared_case(mo, shape):
    """(problem, x0 for 48 instances) of the issue's shape table."""
    n, m, N = shape
    if shape == (1, 1, 1):
        return mo.make_problem([[0.9]], [[1.0]], 1, [-1.0], [1.0]), np.linspace(-3.0, 3.0, 48).reshape(48, 1)
    if shape == (2, 1, 10):
        return mo.double_integrator(N=10), 3.0 * np.random.default_rng(7).normal(size=(48, 2))
    if n == 12:
        return mo.quadrotor(N=N), np.concatenate([mo.quadrotor_x0_batch(16, a, first_instance=16 * i) for i, a in enumerate((3.0, 1.0, 0.3))])
    # amplitudes spread over more than two decades, interleaved: in any leading part of the batch some instances stay inside the
    # box and some saturate
    amp = np.logspace(-1.5, 1.2, 48)[(7 * np.arange(48)) % 48]
    return random_stable(mo, n, m, N, 100 + n), np.random.default_rng(n).normal(size=(48, n)) * amp[:, None]


def solve_shared(capi, p, X0, opts=None, **kw):
    sv = capi.Solver(p.n, p.m, p.N, X0.shape[0], **kw)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    sv.set_reference(p.x_ref, p.u_ref)
    sv.update_initialization(X0)
    sv.calculate(opts)
    return sv


def reference(u, design, model, umin, umax, ops=None):
    """(J, dX, act) of one instance from the handle's own u (m, N)."""
    H, F, d = design
    A, B = model
    act = sr.active_rows(u, umin, umax, d)
    J = sr.jac_gform(H, F, d, act, ops)
    return J, sr.dx_from_du(A, B, J, u.shape[1]), act


def check_jacobians(sv, res, sens, designs, models, umin, umax, skip=()):
    """Every instance's K0, dU, dX and rows against the reference; returns (worst relative error, the active masks)."""
    worst, acts = 0.0, []
    shared_ops = sr.g_operands(*designs) if isinstance(designs, tuple) else None
    for i in range(res["u"].shape[0]):
        des = designs if shared_ops is not None else designs[i]
        mdl = models if isinstance(models, tuple) else models[i]
        J, dX, act = reference(res["u"][i], des, mdl, umin, umax, shared_ops)
        acts.append(act)
        if i in skip:
            continue
        K0, dU = sr.shaped(J, sv.m, sv.N)
        tol = J_RTOL * max(1.0, np.abs(J).max())
        tolx = J_RTOL * max(1.0, np.abs(dX).max())
        assert sens["rows"][i] == act.sum(), (i, sens["rows"][i], act.sum())
        for got, ref, t in ((sens["K0"][i], K0, tol), (sens["dU"][i], dU, tol), (sens["dX"][i], dX, tolx)):
            err = np.abs(got - ref).max()
            worst = max(worst, err / (t / J_RTOL))
            assert err <= t, (i, err, t)
        assert np.array_equal(sens["dX"][i][:, 0, :], np.eye(sv.n))
    return worst, acts


def shared_design(sv):
    g = sv.get_design()
    return g["H"], g["F"], g["d"]


@pytest.mark.parametrize("batch", [19, 48])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 10), (6, 3, 7), (3, 2, 33), (12, 4, 30), (12, 4, 32)])
def test_shared_designs_at_every_tile_shape(capi, mo, shape, batch):
    p, X0 = shared_case(mo, shape)
    sv = solve_shared(capi, p, X0[:batch])
    res = sv.get_results()
    assert np.all(res["status"] == 0), np.bincount(res["status"])
    sens = sv.sensitivity()
    worst, acts = check_jacobians(sv, res, sens, shared_design(sv), (p.A, p.B), p.u_min, p.u_max)
    sv.close()
    nact = sum(int(a.sum()) for a in acts)
    print(f"shape {shape} batch {batch}: rows {min(int(a.sum()) for a in acts)} .. {max(int(a.sum()) for a in acts)}, worst error / scale {worst:.3e}")
    assert 0 < nact < batch * p.nz, "the batch must hold free and active rows"


def test_working_sets_beyond_32_rows_take_the_second_tier(capi, mo):
    p = mo.quadrotor(N=30)
    sv = solve_shared(capi, p, mo.quadrotor_x0_batch(16, amplitude=10.0))
    res = sv.get_results()
    assert np.all(res["status"] == 0), np.bincount(res["status"])
    sens = sv.sensitivity()
    worst, acts = check_jacobians(sv, res, sens, shared_design(sv), (p.A, p.B), p.u_min, p.u_max)
    rows = [int(a.sum()) for a in acts]
    g_u, g_x = _loss(np.random.default_rng(5), 16, p)
    g_x0, vrows = sv.sensitivity_vjp(g_u, g_x)
    wv = _check_vjp(sv, res, sens, g_x0, g_u, g_x, shared_design(sv), (p.A, p.B), acts)
    sv.close()
    print(f"amplitude 10: rows {min(rows)} .. {max(rows)}, {sum(r > 32 for r in rows)} beyond 32; worst J {worst:.3e}, VJP {wv:.3e}")
    assert (min(rows), max(rows), sum(r > 32 for r in rows)) == (13, 58, 9), rows   # (the oracle's figures for this input)
    assert np.array_equal(vrows, sens["rows"])


@pytest.mark.parametrize("N", [10, 30])
def test_per_instance_models(capi, mo, N):
    b = 16
    As, Bs = quad_family(mo, b)
    sv = capi.Solver(12, 4, N, b)
    sv.design_batched(As, Bs, 100 * np.eye(12), 0.1 * np.eye(4), None, None, QUAD_UMIN, QUAD_UMAX)
    sv.update_initialization(mo.quadrotor_x0_batch(b, 2.0, first_instance=5000))
    sv.calculate()
    res = sv.get_results()
    assert np.all(res["status"] == 0), np.bincount(res["status"])
    sens = sv.sensitivity()
    designs = [tuple(sv.get_design_instance(i)[k] for k in ("H", "F", "d")) for i in range(b)]
    models = [(As[i], Bs[i]) for i in range(b)]
    worst, acts = check_jacobians(sv, res, sens, designs, models, np.array(QUAD_UMIN), np.array(QUAD_UMAX))
    g_u, g_x = _loss(np.random.default_rng(6), b, sv)
    g_x0, _ = sv.sensitivity_vjp(g_u, g_x)
    wv = _check_vjp(sv, res, sens, g_x0, g_u, g_x, designs, models, acts)
    sv.close()
    nact = sum(int(a.sum()) for a in acts)
    print(f"per-instance quadrotors N {N}: {nact} active rows, worst J {worst:.3e}, VJP {wv:.3e}")
    assert 0 < nact < b * 4 * N


def test_per_instance_references_and_input_rate_weight(capi, mo):
    # shared model, one reference per instance
    p, X0 = shared_case(mo, (2, 1, 10))
    b = 19
    rng = np.random.default_rng(3)
    xr = np.zeros((b, 2, 11)); xr[:, 0, :] = rng.normal(size=(b, 1))   # a position set-point per instance (an equilibrium)
    ur = 0.3 * rng.uniform(-1, 1, size=(b, 1, 1)) * np.ones((b, 1, 10))
    sv = capi.Solver(2, 1, 10, b)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    sv.set_reference(xr, ur, per_instance=True)
    sv.update_initialization(X0[:b])
    sv.calculate()
    res = sv.get_results()
    assert np.all(res["status"] == 0)
    worst, acts = check_jacobians(sv, res, sv.sensitivity(), shared_design(sv), (p.A, p.B), p.u_min, p.u_max)
    sv.close()
    nact = sum(int(a.sum()) for a in acts)
    assert 0 < nact < b * 10
    # the double integrator with an input-rate weight: S enters H only
    ps = mo.make_problem(p.A, p.B, 10, [-1.0], [1.0], s=0.5)
    sv = solve_shared(capi, ps, X0[:b])
    res = sv.get_results()
    assert np.all(res["status"] == 0)
    H = shared_design(sv)[0]
    assert np.abs(H - mo.condense(ps)[2]).max() <= 1e-10 * np.abs(H).max() and np.abs(H - mo.condense(p)[2]).max() > 0.1
    worst_s, acts = check_jacobians(sv, res, sv.sensitivity(), shared_design(sv), (ps.A, ps.B), ps.u_min, ps.u_max)
    sv.close()
    nact = sum(int(a.sum()) for a in acts)
    print(f"per-instance references: worst {worst:.3e}; S != 0: worst {worst_s:.3e}")
    assert 0 < nact < b * 10


def _loss(rng, b, p):
    return rng.normal(size=(b, p.m, p.N)), rng.normal(size=(b, p.n, p.N + 1))


def _check_vjp(sv, res, sens, g_x0, g_u, g_x, designs, models, acts):
    worst = 0.0
    shared_ops = sr.g_operands(*designs) if isinstance(designs, tuple) else None
    for i in range(g_x0.shape[0]):
        H, F, d = designs if shared_ops is not None else designs[i]
        A, B = models if isinstance(models, tuple) else models[i]
        ref = sr.vjp_gform(H, F, d, acts[i], A, B, g_u[i], g_x[i], shared_ops)
        scale = sr.vjp_scale(ref)
        own = sr.vjp_from_jacobians(sens["dU"][i], sens["dX"][i], g_u[i], g_x[i])
        for other in (ref, own):
            err = np.abs(g_x0[i] - other).max() / scale
            worst = max(worst, err)
            assert err <= J_RTOL, (i, err)
    return worst


def test_vjp_equals_the_jacobians_and_the_reference(capi, mo):
    for shape, b in (((2, 1, 10), 32), ((12, 4, 30), 48), ((6, 3, 7), 19)):
        p, X0 = shared_case(mo, shape)
        sv = solve_shared(capi, p, X0[:b])
        res = sv.get_results()
        sens = sv.sensitivity()
        des = shared_design(sv)
        acts = [sr.active_rows(res["u"][i], p.u_min, p.u_max, des[2]) for i in range(b)]
        g_u, g_x = _loss(np.random.default_rng(17), b, p)
        g_x0, rows = sv.sensitivity_vjp(g_u, g_x)
        assert np.array_equal(rows, sens["rows"])
        worst = _check_vjp(sv, res, sens, g_x0, g_u, g_x, des, (p.A, p.B), acts)
        a0, r0 = sv.sensitivity_vjp(g_u, None)
        a1, r1 = sv.sensitivity_vjp(g_u, np.zeros_like(g_x))
        sv.close()
        print(f"VJP shape {shape}: worst error / scale {worst:.3e}")
        assert a0.tobytes() == a1.tobytes() and np.array_equal(r0, r1)
        assert np.abs(a0).max() > 0


def test_first_move_gain_against_differences_of_the_device_solution(capi, mo):
    p, X0 = shared_case(mo, (2, 1, 10))
    X0 = X0[:32]
    sv = solve_shared(capi, p, X0)
    K0 = sv.sensitivity(("K0",))["K0"]
    h = 1e-6
    fd = np.zeros_like(K0)
    for c in range(2):
        e = np.zeros(2); e[c] = h
        u = []
        for sgn in (1.0, -1.0):
            sv.update_initialization(X0 + sgn * e)
            sv.calculate()
            u.append(sv.get_first_input())
        fd[:, :, c] = (u[0] - u[1]) / (2 * h)
    sv.close()
    err = np.abs(K0 - fd).max() / max(1.0, np.abs(K0).max())
    print(f"K0 against central differences of the device's own u[:,1]: {err:.3e}")
    assert err <= 1e-5
    assert np.any(K0 == 0.0) and np.any(K0 != 0.0)


def test_unsolved_instances_get_minus_one_and_zeros(capi, mo):
    p = mo.quadrotor(N=30)
    b = 48
    sv = solve_shared(capi, p, mo.quadrotor_x0_batch(b, amplitude=3.0), capi.default_opts(polish_max_iter=1), structured_fallback=False)
    res = sv.get_results()
    bad = np.nonzero(res["status"] != 0)[0]
    good = np.nonzero(res["status"] == 0)[0]
    assert bad.size >= 1 and good.size >= 1 and np.all(res["status"][bad] == 1), np.bincount(res["status"])
    sens = sv.sensitivity()
    g_u, g_x = _loss(np.random.default_rng(2), b, p)
    g_x0, vrows = sv.sensitivity_vjp(g_u, g_x)
    for i in bad:
        assert sens["rows"][i] == -1 and vrows[i] == -1
        assert not sens["K0"][i].any() and not sens["dU"][i].any() and not sens["dX"][i].any() and not g_x0[i].any()
    worst, _ = check_jacobians(sv, res, sens, shared_design(sv), (p.A, p.B), p.u_min, p.u_max, skip=set(bad.tolist()))
    sv.close()
    print(f"{bad.size} unsolved of {b}; the others: worst error / scale {worst:.3e}")
    assert np.all(sens["rows"][good] >= 0)


def _refused(capi, sv):
    for call in (lambda: sv.sensitivity(("K0",)), lambda: sv.sensitivity_vjp(np.zeros((sv.batch, sv.m, sv.N)))):
        with pytest.raises(capi.AlmpcError) as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED, e.value
        assert (sv.L.almpc_last_error(sv.h) or b"").decode().strip()


def test_refusals(capi, mo):
    p = mo.double_integrator(N=10)
    X0 = 0.5 * np.random.default_rng(1).normal(size=(4, 2))
    # before any step
    sv = capi.Solver(2, 1, 10, 4)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    assert sv.L.almpc_sensitivity(sv.h, 1, 0.0) == ERR_INVALID
    sv.update_initialization(X0); sv.calculate()
    assert sv.L.almpc_sensitivity(sv.h, 0, 0.0) == ERR_INVALID and sv.L.almpc_sensitivity(sv.h, 8, 0.0) == ERR_INVALID
    assert sv.L.almpc_get_sensitivity(sv.h, None, None, None, None) == ERR_INVALID   # nothing computed yet
    sv.sensitivity(("K0",))
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)   # a new design: no step of it yet
    assert sv.L.almpc_sensitivity(sv.h, 1, 0.0) == ERR_INVALID
    sv.close()
    # state box, terminal equality
    for kw in (dict(xmin=[-50.0, -50.0], xmax=[50.0, 50.0]), dict(terminal="equality")):
        sv = capi.Solver(2, 1, 10, 4)
        sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, **kw)
        sv.update_initialization(0.1 * X0); sv.calculate()
        _refused(capi, sv)
        sv.close()
    # structured handle
    sv = capi.Solver(2, 1, 10, 4, structured=True)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    sv.update_initialization(X0); sv.calculate()
    _refused(capi, sv)
    sv.close()
    # time-varying design
    sv = capi.Solver(2, 1, 10, 4)
    A_all, B_all = np.tile(p.A, (4, 10, 1, 1)), np.tile(p.B, (4, 10, 1, 1))
    xbar = np.zeros((4, 2, 11)); xbar[:, :, 0] = X0
    for k in range(10):
        xbar[:, :, k + 1] = xbar[:, :, k] @ p.A.T
    sv.design_ltv(A_all, B_all, None, xbar, np.zeros((4, 1, 10)), None, None, p.Q, p.R, None, p.P, p.u_min, p.u_max)
    _refused(capi, sv)
    sv.close()


def test_a_sensitivity_call_disturbs_nothing(capi, mo):
    p, X0 = shared_case(mo, (12, 4, 30))
    twins = [solve_shared(capi, p, X0) for _ in range(2)]
    before = twins[0].get_results()
    twins[0].sensitivity()
    twins[0].sensitivity_vjp(*_loss(np.random.default_rng(4), 48, p))
    after = twins[0].get_results()
    for k in ("x", "e_x", "u", "e_u", "status"):
        assert before[k].tobytes() == after[k].tobytes(), k
    X1 = X0 + 0.01
    out = []
    for sv in twins:
        sv.update_initialization(X1)
        sv.calculate(capi.default_opts(warm_start=1))
        out.append(sv.get_results())
        sv.close()
    for k in ("x", "e_x", "u", "e_u", "status", "iters", "polish_iters"):
        assert out[0][k].tobytes() == out[1][k].tobytes(), k


def test_group_equals_one_handle(capi, mo):
    p, X0 = shared_case(mo, (12, 4, 30))
    X0 = X0[:37]
    g_u, g_x = _loss(np.random.default_rng(8), 37, p)
    got = []
    for make in (lambda: capi.Solver(12, 4, 30, 37), lambda: capi.Group(12, 4, 30, 37, devices=[0, 0])):
        s = make()
        s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
        s.set_reference(p.x_ref, p.u_ref)
        s.update_initialization(X0)
        s.calculate()
        sens = s.sensitivity()
        sens["g_x0"], sens["vrows"] = s.sensitivity_vjp(g_u, g_x)
        got.append(sens)
        s.close()
    assert got[0]["rows"].max() > 0
    for k in ("K0", "dU", "dX", "g_x0", "rows", "vrows"):
        assert np.ascontiguousarray(got[0][k]).tobytes() == np.ascontiguousarray(got[1][k]).tobytes(), k


def test_controller_mirror_sensitivity(pkg, capi, mo):
    """sensitivity(C) of the Python mirror is Solver.sensitivity of its handle: a batched controller, and one instance without the
    batch axis."""
    p = mo.double_integrator(N=10)
    X, U = pkg.Hyperrectangle([-100.0] * 2, [100.0] * 2), pkg.Hyperrectangle(p.u_min, p.u_max)
    sys_ = pkg.ConstrainedLinearControlDiscreteSystem(p.A, p.B, X, U)
    X0 = 3.0 * np.random.default_rng(7).normal(size=(8, 2))
    for b in (8, 1):
        C = pkg.proceed_controller(sys_, "model_predictive_control", 10, 1, [0.0, 0.0], [0.0], mpc_batch=b)
        pkg._model_predictive_control_computation(C, X0[:b])
        got = pkg.sensitivity(C, ("K0", "dU"))
        sv = C.tuning.modeler.solver
        res = sv.get_results()
        des = shared_design(sv)
        for i in range(b):
            J, _, act = reference(res["u"][i], des, (p.A, p.B), p.u_min, p.u_max)
            K0, dU = sr.shaped(J, 1, 10)
            gi = {k: (v if b == 1 else v[i]) for k, v in got.items()}
            assert gi["K0"].shape == (1, 2) and gi["dU"].shape == (1, 10, 2) and "dX" not in got
            assert gi["rows"] == act.sum()
            assert np.abs(gi["K0"] - K0).max() <= J_RTOL * max(1.0, np.abs(J).max())
            assert np.abs(gi["dU"] - dU).max() <= J_RTOL * max(1.0, np.abs(J).max())
        sv.close()
    assert "sensitivity" in importlib.import_module(pkg.__name__ + ".controller").__all__
