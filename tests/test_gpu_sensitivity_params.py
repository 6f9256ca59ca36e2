"""GPU tests of the parameter gradients (k_sens_pz, k_sens_params: csrc/almpc_sens.hip.h) through almpc_sensitivity_params_vjp and its
group form.

Reference per instance: the direct form of tests/sens_params_ref.py (H_FF solves, no inverse, no scaling) fed with H, F, d from
almpc_get_design / almpc_get_design_instance and with the handle's OWN returned u, e_u, e_x under the contract's active-set rule, so
both sides differentiate the same face.  Tolerance per case: ten times the gap the G form has to the direct form on the CPU
(sens_params_cases.MEASURED_GAP, recorded by tests/test_sens_params_restatement.py), every group's error per instance over
max(1, max|group|); the factor is for the device's own rounded G = H'^-1.  Every case prints its worst figure per group.
"""
import ctypes
import dataclasses
import importlib

import numpy as np
import pytest

import sens_params_cases as pc
import sens_params_ref as pr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
FD_H, FD_RTOL = 1e-6, 1e-5


def _loss(seed, b, p):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(b, p.m, p.N)), rng.normal(size=(b, p.n, p.N + 1))


def solve_shared(capi, p, X0, opts=None, refs=None, **kw):
    sv = capi.Solver(p.n, p.m, p.N, X0.shape[0], **kw)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, p.P, p.u_min, p.u_max)
    if refs is None:
        sv.set_reference(p.x_ref, p.u_ref)
    else:
        sv.set_reference(*refs, per_instance=True)
    sv.update_initialization(X0)
    sv.calculate(opts)
    return sv


def check_against_direct_form(name, sv, ps, designs, got, g_u, g_x, skip=()):
    """Every group of every instance against the direct form; returns the rows the reference counts."""
    res = sv.get_results()
    worst = dict.fromkeys(pr.GROUPS, 0.0)
    rows = []
    for i, p in enumerate(ps):
        H, F, d = designs if isinstance(designs, tuple) else designs[i]
        r = {k: res[k][i] for k in ("u", "e_u", "e_x")}
        act, lower = pr.sides(r["u"], p.u_min, p.u_max, d)
        rows.append(int(act.sum()))
        if i in skip:
            continue
        assert got["rows"][i] == rows[-1], (i, got["rows"][i], rows[-1])
        ref = pr.params_direct(pr.prob_of(p), H, F, act, lower, r, g_u[i], g_x[i])
        for k, e in pr.worst_gaps({k: got[k][i] for k in pr.GROUPS}, ref).items():
            worst[k] = max(worst[k], e)
    print(f"{name}: rows {min(rows)} .. {max(rows)}; worst error per group: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items())
          + f"; tolerance {pc.gpu_tol(name):g}")
    assert max(worst.values()) <= pc.gpu_tol(name), worst
    return rows


def shared_design(sv):
    g = sv.get_design()
    return g["H"], g["F"], g["d"]


@pytest.mark.parametrize("name", ["di", "r326_refs", "quad", "quad_big"])
def test_shared_designs_every_group(capi, mo, name):
    ps, X0 = pc.problems(mo, name)
    refs = pc.r326_instance_refs(len(X0)) if name == "r326_refs" else None
    sv = solve_shared(capi, ps[0], X0, refs=refs)
    assert np.all(sv.get_results()["status"] == 0)
    g_u, g_x = _loss(41, len(X0), ps[0])
    got = sv.sensitivity_params_vjp(g_u, g_x)
    rows = check_against_direct_form(name, sv, ps, shared_design(sv), got, g_u, g_x)
    # dL/dx0 is almpc_sensitivity_vjp's, bit for bit; a NULL g_x is a g_x of zeros, bit for bit
    g_x0, vrows = sv.sensitivity_vjp(g_u, g_x)
    assert got["x0"].tobytes() == g_x0.tobytes() and np.array_equal(got["rows"], vrows)
    a0 = sv.sensitivity_params_vjp(g_u, None)
    a1 = sv.sensitivity_params_vjp(g_u, np.zeros_like(g_x))
    for k in pr.GROUPS + ("rows",):
        assert np.ascontiguousarray(a0[k]).tobytes() == np.ascontiguousarray(a1[k]).tobytes(), k
    # only what is asked for comes back, with the same bits
    part = sv.sensitivity_params_vjp(g_u, g_x, want=("f", "u_max"))
    assert sorted(part) == ["f", "rows", "u_max"]
    assert part["f"].tobytes() == got["f"].tobytes() and part["u_max"].tobytes() == got["u_max"].tobytes()
    part = sv.sensitivity_params_vjp(g_u, g_x, want=("A", "S"))
    assert np.ascontiguousarray(part["A"]).tobytes() == np.ascontiguousarray(got["A"]).tobytes()
    sv.close()
    if name == "quad_big":   # both tiers
        assert sum(r > 32 for r in rows) >= 1 and sum(r <= 32 for r in rows) >= 1, rows
    if name == "r326_refs":
        assert np.abs(got["S"]).max() > 0 and len(X0) % 4 != 0
    assert min(rows) < max(rows)


def test_per_instance_models(capi, mo):
    ps, X0 = pc.problems(mo, "quadfam")
    b = len(X0)
    sv = capi.Solver(12, 4, 10, b)
    sv.design_batched(np.stack([p.A for p in ps]), np.stack([p.B for p in ps]), ps[0].Q, ps[0].R, None, np.stack([p.P for p in ps]),
                      pc.QUAD_UMIN, pc.QUAD_UMAX)
    sv.update_initialization(X0)
    sv.calculate()
    assert np.all(sv.get_results()["status"] == 0)
    g_u, g_x = _loss(43, b, ps[0])
    got = sv.sensitivity_params_vjp(g_u, g_x)
    designs = [tuple(sv.get_design_instance(i)[k] for k in ("H", "F", "d")) for i in range(b)]
    rows = check_against_direct_form("quadfam", sv, ps, designs, got, g_u, g_x)
    g_x0, _ = sv.sensitivity_vjp(g_u, g_x)
    sv.close()
    assert got["x0"].tobytes() == g_x0.tobytes()
    assert 0 < sum(rows) < b * 40


def test_whole_stack_against_differences_of_the_devices_own_designs(capi, mo):
    """dL/dQ, dL/dR, dL/dA, dL/dumax, each contracted with one direction, against central differences of the device's own designs and
    steps (the only test that rebuilds designs: nine small ones), h = 1e-6, bound 1e-5 of max(1, |value|).  Measured on an MI355X:
    Q 8.7e-6, R 6.7e-6 (both values are 0.04: what is seen is the step's own 1e-11 over 2h, summed over 32 instances), A 1.2e-8,
    u_max 2.3e-10."""
    p, X0 = pc.case(mo, "di")
    g_u, g_x = _loss(47, len(X0), p)
    sv = solve_shared(capi, p, X0)
    got = sv.sensitivity_params_vjp(g_u, g_x, want=("Q", "R", "A", "u_max"))

    def total_loss(**change):
        s2 = solve_shared(capi, dataclasses.replace(p, **change), X0)
        r = s2.get_results()
        s2.close()
        assert np.all(r["status"] == 0)
        return float((g_u * r["u"]).sum() + (g_x * r["x"]).sum())

    rng = np.random.default_rng(53)
    sym = lambda M: 0.5 * (M + M.T)
    dirs = {"Q": sym(rng.normal(size=(2, 2))), "R": sym(rng.normal(size=(1, 1))), "A": rng.normal(size=(2, 2)), "u_max": rng.normal(size=1)}
    sv.close()
    for k, D in dirs.items():
        base = getattr(p, k)
        fd = (total_loss(**{k: base + FD_H * D}) - total_loss(**{k: base - FD_H * D})) / (2 * FD_H)
        val = float((got[k].sum(axis=0) * D).sum())   # (a shared design: the caller sums over the batch)
        err = abs(val - fd) / max(1.0, abs(val))
        print(f"dL/d{k} . direction: {val:.9g}, central differences of the device's steps {fd:.9g}, error {err:.2e}")
        assert err <= FD_RTOL, (k, val, fd)


def test_unsolved_instances_get_minus_one_and_zeros(capi, mo):
    p = mo.quadrotor(N=30)
    b = 48
    X0 = mo.quadrotor_x0_batch(b, amplitude=3.0)
    sv = solve_shared(capi, p, X0, capi.default_opts(polish_max_iter=1), structured_fallback=False)
    res = sv.get_results()
    bad, good = np.nonzero(res["status"] != 0)[0], np.nonzero(res["status"] == 0)[0]
    assert bad.size >= 1 and good.size >= 1, np.bincount(res["status"])
    g_u, g_x = _loss(59, b, p)
    got = sv.sensitivity_params_vjp(g_u, g_x)
    for i in bad:
        assert got["rows"][i] == -1
        assert not any(got[k][i].any() for k in pr.GROUPS)
    # the others are unaffected: the first 16 states are those of the "quad" case, whose CPU gap is on record
    checked = [i for i in good if i < 16]
    check_against_direct_form("quad", sv, [p] * b, shared_design(sv), got, g_u, g_x, skip=set(range(b)) - set(checked))
    sv.close()
    assert len(checked) >= 1 and np.all(got["rows"][good] >= 0)


def test_a_call_disturbs_nothing(capi, mo):
    p, X0 = pc.case(mo, "quad")
    g_u, g_x = _loss(61, len(X0), p)
    twins = [solve_shared(capi, p, X0) for _ in range(2)]
    v0 = twins[0].sensitivity_vjp(g_u, g_x)
    twins[0].sensitivity_params_vjp(g_u, g_x)
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
        for k in ("x", "e_x", "u", "e_u", "status", "iters", "polish_iters"):
            assert pair[0][k].tobytes() == pair[1][k].tobytes(), k


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
        got.append(s.sensitivity_params_vjp(g_u, g_x))
        s.close()
    assert got[0]["rows"].max() > 32
    for k in pr.GROUPS + ("rows",):
        assert np.ascontiguousarray(got[0][k]).tobytes() == np.ascontiguousarray(got[1][k]).tobytes(), k


def _refused(capi, sv, code=ERR_UNSUPPORTED):
    with pytest.raises(capi.AlmpcError) as e:
        sv.sensitivity_params_vjp(np.zeros((sv.batch, sv.m, sv.N)))
    assert e.value.code == code, e.value
    assert (sv.L.almpc_last_error(sv.h) or b"").decode().strip()


def test_refusals(capi, mo):
    p = mo.double_integrator(N=10)
    X0 = 0.5 * np.random.default_rng(1).normal(size=(4, 2))
    # before a step; an out without a pointer, no out, no g_u
    sv = capi.Solver(2, 1, 10, 4)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    _refused(capi, sv, ERR_INVALID)
    sv.update_initialization(X0); sv.calculate()
    g_u = np.zeros((4, 10, 1))
    gp = g_u.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    empty = capi.almpc_param_grads()
    assert sv.L.almpc_sensitivity_params_vjp(sv.h, gp, None, 0.0, ctypes.byref(empty)) == ERR_INVALID
    assert sv.L.almpc_sensitivity_params_vjp(sv.h, gp, None, 0.0, None) == ERR_INVALID
    x0 = np.empty((4, 2))
    only_x0 = capi.almpc_param_grads(x0=x0.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert sv.L.almpc_sensitivity_params_vjp(sv.h, None, None, 0.0, ctypes.byref(only_x0)) == ERR_INVALID
    assert sv.L.almpc_sensitivity_params_vjp(sv.h, gp, None, 0.0, ctypes.byref(only_x0)) == 0
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)   # a new design: no step of it yet
    _refused(capi, sv, ERR_INVALID)
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
    # the SQP loop and the re-linearisation pipeline of a black-box model
    f = mo.synthetic_fnn()
    n, m, N = 4, 2, 10
    x_ref, u_ref = np.zeros((n, N + 1)), np.zeros((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    Al, Bl = capi.fnn_linearize(f.W_in, f.W_h, f.b_h, f.W_out, x_ref[:, -1][None], u_ref[:, -1][None], act=f.act)
    P = capi.dare(Al[0], Bl[0], Q, R)
    x0 = 0.05 * np.random.default_rng(2).normal(size=(4, n))
    sv = capi.Solver(n, m, N, 4)
    sv.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act)
    sv.update_initialization(x0)
    sv.relin_fnn_step()
    _refused(capi, sv)
    sv.close()
    sv = capi.Solver(n, m, N, 4)
    sv.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act)
    sv.sqp_fnn_start(x0)
    sv.sqp_fnn_iterate(1)
    _refused(capi, sv)
    sv.close()


def test_controller_mirror(pkg, capi, mo):
    """sensitivity_params(C) of the Python mirror is Solver.sensitivity_params_vjp of its handle: a batched controller, and one
    instance without the batch axis."""
    p = mo.double_integrator(N=10)
    X, U = pkg.Hyperrectangle([-100.0] * 2, [100.0] * 2), pkg.Hyperrectangle(p.u_min, p.u_max)
    sys_ = pkg.ConstrainedLinearControlDiscreteSystem(p.A, p.B, X, U)
    X0 = 3.0 * np.random.default_rng(7).normal(size=(8, 2))
    g_u, g_x = _loss(71, 8, p)
    for b in (8, 1):
        C = pkg.proceed_controller(sys_, "model_predictive_control", 10, 1, [0.0, 0.0], [0.0], mpc_batch=b)
        pkg._model_predictive_control_computation(C, X0[:b])
        gu, gx = (g_u, g_x) if b > 1 else (g_u[0], g_x[0])
        got = pkg.sensitivity_params(C, gu, gx, want=("x0", "Q", "B", "u_min"))
        sv = C.tuning.modeler.solver
        own = sv.sensitivity_params_vjp(g_u[:b], g_x[:b], want=("x0", "Q", "B", "u_min"))
        assert sorted(got) == ["B", "Q", "rows", "u_min", "x0"]
        for k, v in own.items():
            assert np.array_equal(got[k], v[0] if b == 1 else v), k
        assert got["Q"].shape == ((2, 2) if b == 1 else (8, 2, 2)) and got["B"].shape == ((2, 1) if b == 1 else (8, 2, 1))
        sv.close()
    assert "sensitivity_params" in importlib.import_module(pkg.__name__ + ".controller").__all__
