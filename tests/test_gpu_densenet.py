"""GPU tests of the DenseNet model family (include/almpc.h, the almpc_*densenet* calls) on every network path: batched linearisation
(wave and workgroup builds), the re-linearisation pipeline (condensed and structured), the SQP loop (Gauss-Newton, exact Hessian,
structured QP), the group form and the mirror.  Reference: the numpy restatement tests/densenet_ref.py."""
import numpy as np
import pytest

import densenet_ref as dn
import sqp_exact_ref as ex
import sqp_solve_ref as sref

pytestmark = pytest.mark.gpu
ACTS = ("identity", "relu", "tanh", "sigmoid", "swish")


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("shape", [(16, 2), (64, 3), (16, 0)])   # wave path (two points per wave), workgroup path, no hidden layer
def test_linearize_every_activation(capi, mo, shape):
    H, L = shape
    n, m, b = 4, 2, 512
    r = np.random.default_rng(7)
    x, u = 1.5 * r.normal(size=(b, n)), 1.5 * r.normal(size=(b, m))
    for act in ACTS:
        f = dn.synthetic_densenet(n, m, H=H, L=L, act=act)
        A, B, fv = capi.densenet_linearize(f.W_in, f.W_h, f.b_h, f.W_out, x, u, act=act, want_f=True)
        for i in range(0, b, 3):
            Ar, Br = f.jacobian(x[i], u[i])
            assert _rel(A[i], Ar) <= 1e-12 and _rel(B[i], Br) <= 1e-12, (act, i)
            assert _rel(fv[i], f.forward(x[i], u[i])) <= 1e-12, (act, i)
        if L == 0:   # no hidden layer: the Fnn kernels on the same W_in / W_out
            Af, Bf, ff = capi.fnn_linearize(f.W_in, [], [], f.W_out, x, u, act=act, want_f=True)
            assert _rel(A, Af) <= 1e-14 and _rel(B, Bf) <= 1e-14 and _rel(fv, ff) <= 1e-14, act


def test_unknown_activation_is_refused(capi):
    f = dn.synthetic_densenet(4, 2, H=16, L=2, act="tanh")
    L = capi.load()
    W_in, W_h, b_h, W_out = dn.pack(f)
    for code in (5, (1 << 8) | 2, -1):   # past the activations, a network code, negative
        A = np.empty(16); B = np.empty(8)
        rc = L.almpc_densenet_linearize(0, 4, 2, 16, 2, code, capi._ptr(W_in), capi._ptr(W_h), capi._ptr(b_h), capi._ptr(W_out), 1,
                                        capi._ptr(np.zeros(4)), capi._ptr(np.zeros(2)), capi._ptr(A), capi._ptr(B), None)
        assert rc == -4, code   # ALMPC_ERR_UNSUPPORTED


def _relin_setup(capi, f, batch, N, structured=False, box=None):
    n, m = 4, 2
    x_ref = np.array([0.2, -0.1, 0.05, 0.0])[:, None] * np.ones((n, N + 1))
    u_ref = np.array([0.1, -0.2])[:, None] * np.ones((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    Al, Bl = f.jacobian(x_ref[:, -1], u_ref[:, -1])
    P = capi.dare(Al, Bl, Q, R)
    s = capi.Solver(n, m, N, batch, structured=structured)
    s.relin_densenet_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act,
                           xmin=None if box is None else -box, xmax=box)
    return s, x_ref, u_ref, P


@pytest.mark.parametrize("structured", [False, True])
def test_relin_pipeline(capi, mo, structured):
    """configs[3] shape (1024 instances, N 20, tanh): every instance's model is the restatement's linearisation, u the exact oracle's
    on it; advance steps the network itself.  Structured: the same with a state box."""
    batch, N = 1024, 20
    f = dn.synthetic_densenet(act="tanh")
    box = np.array([10.0, 10.0, 10.0, 10.0]) if structured else None
    s, x_ref, u_ref, P = _relin_setup(capi, f, batch, N, structured, box)
    X0 = x_ref[:, 0][None, :] + 0.5 * mo.splitmix_normal(0x5EED0004, 21, batch, 4)
    s.update_initialization(X0)
    s.relin_fnn_step(capi.default_opts())
    r = s.get_results()
    if structured:   # (an open-loop unstable linearisation can leave no trajectory inside the box: status 3, checked below)
        assert np.all((r["status"] == 0) | (r["status"] == 3)) and (r["status"] == 0).mean() >= 0.95, np.bincount(r["status"])
        for i in np.nonzero(r["status"] == 3)[0][:8]:
            Ai, Bi = f.jacobian(X0[i], u_ref[:, 0])
            with pytest.raises(ValueError):
                mo.solve_mpc_exact(mo.make_problem(Ai, Bi, N, [-1, -1], [1, 1], x_ref=x_ref, u_ref=u_ref, P=P, x_min=-box, x_max=box), X0[i])
    else:
        assert np.all(r["status"] == 0), np.bincount(r["status"])
    for i in np.nonzero(r["status"] == 0)[0]:   # the device's predicted errors are those of the restated linearisation
        Ai, Bi = f.jacobian(X0[i], u_ref[:, 0])
        ex_, eu = r["e_x"][i], r["e_u"][i]
        pred = np.stack([Ai @ ex_[:, k] + Bi @ eu[:, k] for k in range(N)], axis=1)
        assert _rel(ex_[:, 1:], pred) <= 1e-9, i
    for i in range(0, batch, 31):
        if r["status"][i] != 0:
            continue
        Ai, Bi = f.jacobian(X0[i], u_ref[:, 0])
        p = mo.make_problem(Ai, Bi, N, [-1, -1], [1, 1], x_ref=x_ref, u_ref=u_ref, P=P, x_min=None if box is None else -box,
                            x_max=box)
        e = mo.solve_mpc_exact(p, X0[i])
        assert np.abs(r["u"][i] - e["u"]).max() <= 1e-6, i
    s.relin_fnn_advance()
    s.relin_fnn_step(capi.default_opts())
    r2 = s.get_results()
    xn = r2["x"][:, :, 0]
    for i in range(0, batch, 7):
        if r["status"][i] != 0:
            continue
        xw = f.forward(X0[i], r["u"][i][:, 0])
        assert np.abs(xn[i] - xw).max() <= 1e-12 * max(1.0, np.abs(xw).max()), i
    s.close()


def _sqp_solver(capi, f, kw, b, N, qp_solver="condensed"):
    s = capi.Solver(4, 2, N, b)
    s.sqp_densenet_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"],
                         kw["u_max"], act=f.act, qp_solver=qp_solver)
    return s


def _bench(b, N, H=16, L=2):
    _, kw, X0 = sref.bench_setup(b=b, N=N)
    return dn.synthetic_densenet(H=H, L=L, act="tanh"), kw, X0


def test_sqp_gauss_newton_matches_the_restatement(capi, mo):
    b, N, iters = 64, 50, 10
    f, kw, X0 = _bench(b, N)
    s = _sqp_solver(capi, f, kw, b, N)
    s.sqp_fnn_start(X0)
    s.sqp_fnn_iterate(iters)
    r = s.get_results(want=("u", "x"))
    s.close()
    worst = 0.0
    for i in range(0, b, 4):
        X, U, _ = mo.sqp_fnn(f, X0[i], kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"], iters)
        worst = max(worst, np.abs(r["u"][i] - U).max())
        assert np.abs(r["x"][i] - mo.fnn_rollout(f, X0[i], r["u"][i])).max() <= 1e-9 or np.abs(r["x"][i] - X).max() <= 1e-7, i
    assert worst <= 1e-9, worst


def test_sqp_structured_qp_gives_the_condensed_iterates(capi):
    b, N, iters = 32, 20, 6
    f, kw, X0 = _bench(b, N)
    out = []
    for qp in ("condensed", "structured"):
        s = _sqp_solver(capi, f, kw, b, N, qp_solver=qp)
        s.sqp_fnn_start(X0)
        s.sqp_fnn_iterate(iters)
        out.append(s.get_results(want=("u", "x")))
        s.close()
    assert np.abs(out[0]["u"] - out[1]["u"]).max() <= 1e-9
    assert np.abs(out[0]["x"] - out[1]["x"]).max() <= 1e-9


def test_sqp_exact_first_qp_matches_the_restatement(capi, mo, monkeypatch):
    monkeypatch.setattr(ex, "stage_hessian", dn.stage_hessian)
    b, N = 8, 50
    f, kw, X0 = _bench(b, N)
    s = _sqp_solver(capi, f, kw, b, N)
    s.sqp_fnn_set_hessian("exact")
    s.sqp_fnn_start(X0)
    s.sqp_fnn_iterate(1, step_rule="merit")
    U = np.clip(kw["u_ref"], -1.0, 1.0)
    for i in range(b):
        X = mo.fnn_rollout(f, X0[i], U)
        A, B, c = [], [], []
        for k in range(N):
            Ak, Bk = f.jacobian(X[:, k], U[:, k])
            A.append(Ak); B.append(Bk); c.append(f.forward(X[:, k], U[:, k]) - X[:, k + 1])
        He, qe, *_ = ex.exact_qp(f, X, U, A, B, c, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"])
        Hd, qd = s.get_design_instance(i)["H"], s.get_gradient_instance(i)
        assert np.abs(Hd - He).max() <= 1e-10 * np.abs(He).max(), i
        assert np.abs(qd - qe).max() <= 1e-10 * max(1.0, np.abs(qe).max()), i
    s.close()


def test_sqp_exact_solve_is_certified(capi, mo, monkeypatch):
    monkeypatch.setattr(ex, "stage_hessian", dn.stage_hessian)
    b, N, tol = 64, 50, 1e-6
    f, kw, X0 = _bench(b, N)
    s = _sqp_solver(capi, f, kw, b, N)
    s.sqp_fnn_set_hessian("exact")
    s.sqp_fnn_start(X0)
    out = s.sqp_fnn_solve(30, tol)
    r = s.get_results(want=("u", "x"))
    s.close()
    assert (out["status"] == 0).mean() >= 0.9, np.bincount(out["status"])
    for i in np.nonzero(out["status"] == 0)[0]:
        assert out["kkt"][i] <= tol and np.abs(r["x"][i] - mo.fnn_rollout(f, X0[i], r["u"][i])).max() <= 1e-9, i
        assert mo.nlp_kkt_residual(f, X0[i], r["u"][i], kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"],
                                   kw["u_max"]) <= 10 * tol, i
    for i in range(0, b, 8):
        e = ex.sqp_solve_exact(f, X0[i], kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"], 30, tol)
        assert e["status"] == out["status"][i] and abs(e["iters"] - out["iters"][i]) <= 1, (i, e["status"], e["iters"], out["iters"][i])


def test_sqp_exact_refuses_a_densenet_past_the_lds_budget(capi):
    """H 64, L 2: y, its adjoint and d y / d z have 3 H rows, past the per-wave scratch of four waves in 64 KB; H 16, L 2 fits."""
    b, N = 4, 10
    _, kw, X0 = sref.bench_setup(b=b, N=N)
    for H, ok in ((16, True), (64, False)):
        f = dn.synthetic_densenet(H=H, L=2, act="tanh")
        s = _sqp_solver(capi, f, kw, b, N)
        if ok:
            s.sqp_fnn_set_hessian("exact")
        else:
            with pytest.raises(capi.AlmpcError) as e:
                s.sqp_fnn_set_hessian("exact")
            assert e.value.code == -4 and "DenseNet" in str(e.value)   # ALMPC_ERR_UNSUPPORTED
        s.close()


def test_group_of_two_equals_one_handle(capi):
    b, N = 40, 30
    f, kw, X0 = _bench(b, N)
    s = _sqp_solver(capi, f, kw, b, N)
    s.sqp_fnn_start(X0)
    one = s.sqp_fnn_solve(20, 1e-6)
    r1 = s.get_results(want=("u",))
    s.close()
    g = capi.Group(4, 2, N, b, devices=[0, 0])
    g.sqp_densenet_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"],
                         kw["u_max"], act="tanh")
    g.sqp_fnn_start(X0)
    two = g.sqp_fnn_solve(20, 1e-6)
    r2 = g.get_results()
    g.close()
    assert np.array_equal(one["status"], two["status"]) and np.array_equal(one["iters"], two["iters"])
    assert np.array_equal(r1["u"], r2["u"])


def _mirror_system(pkg, cls, f, lo, hi, n=4):
    return pkg.ConstrainedBlackBoxControlDiscreteSystem(cls(f.W_in, f.W_h, f.b_h, f.W_out, f.act), n, lo.size,
                                                       pkg.Hyperrectangle(-5.0 * np.ones(n), 5.0 * np.ones(n)), pkg.Hyperrectangle(lo, hi))


def _mirror_u(pkg, system, x0, xr, ur, N=10, **kw):
    refs = pkg._design_reference_mpc(xr, ur, N)
    C = pkg._model_predictive_control_design(system, N, 1, refs, **kw)
    pkg.update_initialization(C, x0)
    pkg.calculate(C)
    return np.array(C.computation_results.u), C


def _mirror_every_mode(pkg, mo, f, x0, xr, ur, lo, hi, N=10):
    n, m = xr.size, ur.size
    sysd = _mirror_system(pkg, pkg.DenseNet, f, lo, hi, n)
    x_ref, u_ref = xr[:, None] * np.ones((n, N + 1)), ur[:, None] * np.ones((m, N))
    # linear: the restated linear problem of the reference's LinearProgramming branch
    u_lin, C = _mirror_u(pkg, sysd, x0, xr, ur, N)
    p = mo.fnn_linear_problem(f, N, lo, hi, x_ref, u_ref)
    assert np.abs(u_lin - mo.solve_mpc_exact(p, x0)["u"]).max() <= 1e-5
    # linear + step: the instance's own linearisation at x0
    u_step, _ = _mirror_u(pkg, sysd, x0, xr, ur, N, mpc_linearization="step")
    A, B = f.jacobian(x0, u_ref[:, 0])
    p2 = mo.make_problem(A, B, N, lo, hi, x_ref=x_ref, u_ref=u_ref, P=p.P)
    assert np.abs(u_step - mo.solve_mpc_exact(p2, x0)["u"]).max() <= 1e-5
    # non_linear: a certified KKT point of the NLP on the DenseNet
    u_nl, C = _mirror_u(pkg, sysd, x0, xr, ur, N, mpc_programming_type="non_linear", mpc_sqp_tolerance=1e-7, mpc_sqp_iterations=30)
    assert mo.nlp_kkt_residual(f, x0, u_nl, x_ref, u_ref, C.tuning.weights.Q, C.tuning.weights.R, C.tuning.weights.S, p.P, lo, hi) <= 1e-6
    return u_lin


def test_mirror_runs_densenet_on_every_mode(pkg, mo):
    f = dn.synthetic_densenet(act="tanh")
    _mirror_every_mode(pkg, mo, f, np.array([0.5, -0.3, 0.2, 0.1]), np.array([0.2, -0.1, 0.05, 0.0]), np.array([0.1, -0.2]),
                       -np.ones(2), np.ones(2))
    # the same weights handed to the Fnn layout are refused, not read as some other network
    with pytest.raises(ValueError):
        pkg._capi.fnn_linearize(f.W_in, f.W_h, f.b_h, f.W_out, np.zeros((1, 4)), np.zeros((1, 2)), act="tanh")


def test_mirror_runs_the_reference_scenario(pkg, mo):
    """The reference's DenseNet scenario (test/computation_mpc_test.jl:323-440): the QTP system (n 4, m 2, inputs in [0, 4] x [0, 3.26]),
    horizon 5, references 0.65 and 1.2, x0 = 0.6 * ones, the LP and NLP controllers; synthetic weights (its trained model is not in the
    reference checkout)."""
    f = dn.synthetic_densenet(4, 2, H=16, L=2, act="tanh", seed=0xD15E)
    _mirror_every_mode(pkg, mo, f, 0.6 * np.ones(4), 0.65 * np.ones(4), 1.2 * np.ones(2), np.zeros(2), np.array([4.0, 3.26]), N=5)
