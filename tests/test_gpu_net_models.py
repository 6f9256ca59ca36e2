"""GPU tests of the ResNet and PolyNet model families (include/almpc.h ALMPC_NET_*) on every network path: batched linearisation,
the re-linearisation pipeline (condensed and structured), the SQP loop (Gauss-Newton and exact Hessian), the group form and the
mirror.  Reference: the numpy restatement tests/net_ref.py."""
import numpy as np
import pytest

import net_ref
import sqp_exact_ref as ex
import sqp_solve_ref as sref

pytestmark = pytest.mark.gpu
KINDS = ("fnn", "resnet", "polynet")
ACTS = ("identity", "relu", "tanh", "sigmoid", "swish")


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("shape", [(16, 2), (64, 3), (16, 0)])   # wave path (two points per wave), workgroup path, no hidden layer
def test_linearize_every_kind_and_activation(capi, shape):
    H, L = shape
    n, m, b = 4, 2, 512
    r = np.random.default_rng(7)
    x, u = 1.5 * r.normal(size=(b, n)), 1.5 * r.normal(size=(b, m))   # pre-activations on both sides of the relu kinks
    for act in ACTS:
        base = net_ref.synthetic_net("fnn", H=H, L=L, act=act)
        out = {}
        for kind in KINDS:
            f = net_ref.as_kind(base, kind)
            A, B, fv = capi.fnn_linearize(f.W_in, f.W_h, f.b_h, f.W_out, x, u, act=act, want_f=True, net=kind)
            out[kind] = (A, B, fv)
            for i in range(0, b, 3):
                Ar, Br = f.jacobian(x[i], u[i])
                assert _rel(A[i], Ar) <= 1e-12 and _rel(B[i], Br) <= 1e-12, (kind, act, i)
                assert _rel(fv[i], f.forward(x[i], u[i])) <= 1e-12, (kind, act, i)
        if L == 0:   # all kinds are the same network
            for kind in KINDS[1:]:
                for a, c in zip(out[kind], out["fnn"]):
                    assert np.array_equal(a, c), (kind, act)
        else:
            assert not np.allclose(out["resnet"][0], out["fnn"][0]) and not np.allclose(out["polynet"][0], out["resnet"][0])


def test_unknown_network_codes_are_refused(capi):
    f = net_ref.synthetic_net("fnn", act="tanh")
    L = capi.load()
    for code in ((3 << 8) | 2, (1 << 8) | 5, -1):   # unknown kind, unknown activation, negative
        A = np.empty(16); B = np.empty(8)
        rc = L.almpc_fnn_linearize(0, 4, 2, 16, 2, code, capi._ptr(np.asfortranarray(f.W_in)),
                                   capi._ptr(np.ascontiguousarray(np.stack([w.T for w in f.W_h]))),
                                   capi._ptr(np.ascontiguousarray(np.stack(f.b_h))), capi._ptr(np.asfortranarray(f.W_out)), 1,
                                   capi._ptr(np.zeros(4)), capi._ptr(np.zeros(2)), capi._ptr(A), capi._ptr(B), None)
        assert rc == -4, code   # ALMPC_ERR_UNSUPPORTED


def _relin_setup(capi, f, kind, batch, N, structured=False, box=None):
    n, m = 4, 2
    x_ref = np.array([0.2, -0.1, 0.05, 0.0])[:, None] * np.ones((n, N + 1))
    u_ref = np.array([0.1, -0.2])[:, None] * np.ones((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    Al, Bl = f.jacobian(x_ref[:, -1], u_ref[:, -1])
    P = capi.dare(Al, Bl, Q, R)
    s = capi.Solver(n, m, N, batch, structured=structured)
    s.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act, net=kind,
                      xmin=None if box is None else -box, xmax=box)
    return s, x_ref, u_ref, P


@pytest.mark.parametrize("kind", ["resnet", "polynet"])
@pytest.mark.parametrize("structured", [False, True])
def test_relin_pipeline(capi, mo, kind, structured):
    """configs[3] shape (1024 instances, N 20, tanh): every instance's model is the restatement's linearisation, u the exact oracle's
    on it, every status 0; advance steps the network itself.  Structured: the same with a state box."""
    batch, N = 1024, 20
    f = net_ref.synthetic_net(kind, act="tanh")
    box = np.array([10.0, 10.0, 10.0, 10.0]) if structured else None
    s, x_ref, u_ref, P = _relin_setup(capi, f, kind, batch, N, structured, box)
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


def _sqp_solver(capi, f, kind, kw, b, N):
    s = capi.Solver(4, 2, N, b)
    s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"],
                    kw["u_max"], act=f.act, net=kind)
    return s


def _bench(kind, b, N):
    _, kw, X0 = sref.bench_setup(b=b, N=N)
    return net_ref.synthetic_net(kind, act="tanh"), kw, X0


@pytest.mark.parametrize("kind", ["resnet", "polynet"])
def test_sqp_gauss_newton_matches_the_restatement(capi, mo, kind):
    b, N, iters = 64, 50, 10
    f, kw, X0 = _bench(kind, b, N)
    s = _sqp_solver(capi, f, kind, kw, b, N)
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


@pytest.mark.parametrize("kind", ["resnet", "polynet"])
def test_sqp_exact_first_qp_matches_the_restatement(capi, mo, kind, monkeypatch):
    monkeypatch.setattr(ex, "stage_hessian", net_ref.stage_hessian)
    b, N = 8, 50
    f, kw, X0 = _bench(kind, b, N)
    s = _sqp_solver(capi, f, kind, kw, b, N)
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


@pytest.mark.parametrize("kind", ["resnet", "polynet"])
def test_sqp_exact_solve_is_certified(capi, mo, kind, monkeypatch):
    monkeypatch.setattr(ex, "stage_hessian", net_ref.stage_hessian)
    b, N, tol = 64, 50, 1e-6
    f, kw, X0 = _bench(kind, b, N)
    s = _sqp_solver(capi, f, kind, kw, b, N)
    s.sqp_fnn_set_hessian("exact")
    s.sqp_fnn_start(X0)
    out = s.sqp_fnn_solve(30, tol)
    r = s.get_results(want=("u", "x"))
    s.close()
    assert (out["status"] == 0).mean() >= 0.9, np.bincount(out["status"])
    # certificate: the device's stopping residual (the adjoint one of sqp_solve_ref) and the oracle's single-shooting KKT residual.  The
    # two measures differ by a factor at the same point (the restatement's own converged ResNet instance 4: 6.9e-8 against 4.1e-7)
    for i in np.nonzero(out["status"] == 0)[0]:
        assert out["kkt"][i] <= tol and np.abs(r["x"][i] - mo.fnn_rollout(f, X0[i], r["u"][i])).max() <= 1e-9, i
        assert mo.nlp_kkt_residual(f, X0[i], r["u"][i], kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"],
                                   kw["u_max"]) <= 10 * tol, i
    for i in range(0, b, 8):
        e = ex.sqp_solve_exact(f, X0[i], kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"], 30, tol)
        assert e["status"] == out["status"][i] and abs(e["iters"] - out["iters"][i]) <= 1, (i, e["status"], e["iters"], out["iters"][i])


def test_sqp_exact_refuses_a_polynet_past_the_lds_budget(capi):
    """H 64, L 2: the ResNet's per-wave scratch fits 16 KB, the PolyNet's (2 L activation sites) does not."""
    b, N = 4, 10
    _, kw, X0 = sref.bench_setup(b=b, N=N)
    for kind, ok in (("resnet", True), ("polynet", False)):
        f = net_ref.synthetic_net(kind, H=64, L=2, act="tanh")
        s = _sqp_solver(capi, f, kind, kw, b, N)
        if ok:
            s.sqp_fnn_set_hessian("exact")
        else:
            with pytest.raises(capi.AlmpcError) as e:
                s.sqp_fnn_set_hessian("exact")
            assert e.value.code == -4 and "PolyNet" in str(e.value)   # ALMPC_ERR_UNSUPPORTED
        s.close()


def test_group_of_two_equals_one_handle(capi):
    b, N = 40, 30
    f, kw, X0 = _bench("resnet", b, N)
    s = _sqp_solver(capi, f, "resnet", kw, b, N)
    s.sqp_fnn_start(X0)
    one = s.sqp_fnn_solve(20, 1e-6)
    r1 = s.get_results(want=("u",))
    s.close()
    g = capi.Group(4, 2, N, b, devices=[0, 0])
    g.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"],
                    kw["u_max"], act="tanh", net="resnet")
    g.sqp_fnn_start(X0)
    two = g.sqp_fnn_solve(20, 1e-6)
    r2 = g.get_results()
    g.close()
    assert np.array_equal(one["status"], two["status"]) and np.array_equal(one["iters"], two["iters"])
    assert np.array_equal(r1["u"], r2["u"])


def _mirror_system(pkg, cls, f):
    return pkg.ConstrainedBlackBoxControlDiscreteSystem(cls(f.W_in, f.W_h, f.b_h, f.W_out, f.act), 4, 2,
                                                       pkg.Hyperrectangle(-5.0 * np.ones(4), 5.0 * np.ones(4)),
                                                       pkg.Hyperrectangle(-np.ones(2), np.ones(2)))


def _mirror_u(pkg, system, x0, N=10, **kw):
    refs = pkg._design_reference_mpc(np.array([0.2, -0.1, 0.05, 0.0]), np.array([0.1, -0.2]), N)
    C = pkg._model_predictive_control_design(system, N, 1, refs, **kw)
    pkg.update_initialization(C, x0)
    pkg.calculate(C)
    return np.array(C.computation_results.u), C


def test_mirror_runs_resnet_on_every_mode(pkg, mo):
    f = net_ref.synthetic_net("resnet", act="tanh")
    sysr = _mirror_system(pkg, pkg.ResNet, f)
    x0 = np.array([0.5, -0.3, 0.2, 0.1])
    N = 10
    x_ref = np.array([0.2, -0.1, 0.05, 0.0])[:, None] * np.ones((4, N + 1))
    u_ref = np.array([0.1, -0.2])[:, None] * np.ones((2, N))
    # linear: the restated linear problem of the reference's LinearProgramming branch
    u_lin, _ = _mirror_u(pkg, sysr, x0)
    p = mo.fnn_linear_problem(f, N, [-1, -1], [1, 1], x_ref, u_ref)
    assert np.abs(u_lin - mo.solve_mpc_exact(p, x0)["u"]).max() <= 1e-5
    # linear + step: the instance's own linearisation at x0
    u_step, _ = _mirror_u(pkg, sysr, x0, mpc_linearization="step")
    A, B = f.jacobian(x0, u_ref[:, 0])
    p2 = mo.make_problem(A, B, N, [-1, -1], [1, 1], x_ref=x_ref, u_ref=u_ref, P=p.P)
    assert np.abs(u_step - mo.solve_mpc_exact(p2, x0)["u"]).max() <= 1e-5
    # non_linear: a certified KKT point of the NLP on the ResNet
    u_nl, C = _mirror_u(pkg, sysr, x0, mpc_programming_type="non_linear", mpc_sqp_tolerance=1e-7, mpc_sqp_iterations=30)
    assert mo.nlp_kkt_residual(f, x0, u_nl, x_ref, u_ref, C.tuning.weights.Q, C.tuning.weights.R, C.tuning.weights.S, p.P,
                               -np.ones(2), np.ones(2)) <= 1e-6
    # the same weights as an Fnn give another controller (no silent Fnn dispatch); an Icnn is an Fnn bit for bit
    u_fnn, _ = _mirror_u(pkg, _mirror_system(pkg, pkg.Fnn, f), x0)
    assert np.abs(u_fnn - u_lin).max() > 1e-3
    u_icnn, _ = _mirror_u(pkg, _mirror_system(pkg, pkg.Icnn, f), x0)
    assert np.array_equal(u_icnn, u_fnn)

    class DenseNet(pkg.Fnn):
        pass

    with pytest.raises(NotImplementedError):
        _mirror_u(pkg, _mirror_system(pkg, DenseNet, f), x0)
