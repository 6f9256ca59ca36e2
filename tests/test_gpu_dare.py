"""GPU tests of k_dare (csrc/almpc_dare.hip.h): the batched DARE entry point almpc_dare_batched against scipy, and the per-instance
terminal weights it gives almpc_design_batched(P = NULL) and the re-linearisation pipeline (almpc_set_terminal_weight).

Tolerances.  A terminal weight: max|P - P_scipy| <= 1e-9 max|P_scipy|, the bound tests/test_capi_abi.py holds the host DARE to (the
kernel runs the same algorithm in FP64; the host's measured error on these inputs is 1.5e-10).  A solution: |u - u*|_inf <= 1e-5
against the exact oracle built with scipy's P_i."""
import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

P_RTOL = 1e-9
U_TOL = 1e-5
ERR_UNSUPPORTED, ERR_NUMERIC = -4, -6


def random_models(n, m, batch):
    rng = np.random.default_rng(1000 + n)
    A = rng.standard_normal((batch, n, n)) / np.sqrt(n) * rng.uniform(0.6, 1.3, (batch, 1, 1))
    B = rng.standard_normal((batch, n, m))
    return A, B, 100.0 * np.eye(n), 0.1 * np.eye(m)


def bad_model():
    """An unstable mode no input reaches: blkdiag([[1.2, 0], [0, 0.5]], 0.5 I2), row 0 of B zero (n 4, m 2)."""
    A = np.zeros((4, 4))
    A[0, 0], A[1, 1], A[2, 2], A[3, 3] = 1.2, 0.5, 0.5, 0.5
    B = np.random.default_rng(3).standard_normal((4, 2))
    B[0, :] = 0.0
    return A, B


def scipy_dare(A, B, Q, R):
    return sla.solve_discrete_are(A, B, Q, R)


def check_weights(P, st, A, B, Q, R):
    assert np.all(st == 0), np.nonzero(st)[0]
    worst = 0.0
    for i in range(A.shape[0]):
        Ps = scipy_dare(A[i], B[i], Q, R)
        worst = max(worst, np.abs(P[i] - Ps).max() / np.abs(Ps).max())
    print(f"n {A.shape[1]} m {B.shape[2]}: max relative error against scipy {worst:.3e}")
    assert worst <= P_RTOL
    assert np.array_equal(P, P.transpose(0, 2, 1))   # symmetric bit for bit


@pytest.mark.parametrize("n,m", [(1, 1), (2, 1), (4, 2), (12, 4), (16, 16), (17, 3), (32, 8), (33, 3), (48, 16)])
def test_dare_batched_matches_scipy(capi, n, m):
    A, B, Q, R = random_models(n, m, 67)
    P, st = capi.dare_batched(A, B, Q, R)
    check_weights(P, st, A, B, Q, R)


def test_dare_batched_perturbed_quadrotors(capi, mo):
    p = mo.quadrotor()
    rng = np.random.default_rng(7)
    A = p.A[None] * (1.0 + 0.05 * rng.standard_normal((256, 12, 12)))
    B = p.B[None] * (1.0 + 0.05 * rng.standard_normal((256, 12, 4)))
    P, st = capi.dare_batched(A, B, 100.0 * np.eye(12), 0.1 * np.eye(4))
    check_weights(P, st, A, B, 100.0 * np.eye(12), 0.1 * np.eye(4))


def test_failing_instances_are_reported_and_leave_the_others_alone(capi):
    A, B, Q, R = random_models(4, 2, 40)
    Ab, Bb = bad_model()
    A2, B2 = A.copy(), B.copy()
    for i in (3, 17):
        A2[i], B2[i] = Ab, Bb
    sentinel = np.full((40, 4, 4), -12345.678)
    Pg, stg = capi.dare_batched(A, B, Q, R, P_init=sentinel)
    P2, st2 = capi.dare_batched(A2, B2, Q, R, P_init=sentinel)
    assert np.all(stg == 0)
    assert sorted(np.nonzero(st2)[0].tolist()) == [3, 17]
    keep = np.ones(40, dtype=bool)
    keep[[3, 17]] = False
    assert np.array_equal(P2[~keep], sentinel[~keep])   # a failed instance's slot is not written
    assert np.array_equal(P2[keep], Pg[keep])            # bit-identical: no instance depends on its neighbours


def test_limits_and_singular_R(capi):
    A, B, Q, R = random_models(49, 2, 3)
    with pytest.raises(capi.AlmpcError) as e:
        capi.dare_batched(A, B, Q, R)
    assert e.value.code == ERR_UNSUPPORTED
    A, B, Q, R = random_models(4, 17, 3)
    with pytest.raises(capi.AlmpcError) as e:
        capi.dare_batched(A, B, Q, R)
    assert e.value.code == ERR_UNSUPPORTED
    A, B, Q, R = random_models(4, 2, 3)
    with pytest.raises(capi.AlmpcError) as e:
        capi.dare_batched(A, B, Q, np.array([[1.0, 2.0], [2.0, 4.0]]))
    assert e.value.code == ERR_NUMERIC


# ---- almpc_set_terminal_weight: almpc_design_batched(P = NULL) ---------------------------------------------------------------------

UMIN, UMAX = [-1.0, -1.0], [1.0, 1.0]


@pytest.mark.parametrize("structured", [False, True])
def test_design_batched_takes_its_terminal_weights_from_the_device(capi, mo, structured):
    n, m, N, b = 4, 2, 10, 33
    A, B, Q, R = random_models(n, m, b)
    X0 = np.random.default_rng(5).uniform(-1.0, 1.0, (b, n))
    s = capi.Solver(n, m, N, b, structured=structured)
    s.set_terminal_weight("dare_device")
    s.design_batched(A, B, Q, R, None, None, UMIN, UMAX)
    Ps = [scipy_dare(A[i], B[i], Q, R) for i in range(b)]
    for i in range(b):
        assert np.abs(s.terminal_weight_instance(i) - Ps[i]).max() <= P_RTOL * np.abs(Ps[i]).max(), i
    s.update_initialization(X0)
    s.calculate()
    r = s.get_results()
    assert np.all(r["status"] == 0), np.bincount(r["status"])
    worst = 0.0
    for i in range(b):
        e = mo.solve_mpc_exact(mo.make_problem(A[i], B[i], N, UMIN, UMAX, P=Ps[i]), X0[i])
        worst = max(worst, np.abs(r["u"][i] - e["u"]).max())
    print(f"design_batched, structured {structured}: max |u - u*| {worst:.3e}")
    assert worst <= U_TOL
    # an instance without a stabilising solution is the host path's error, naming the instance
    A2, B2 = A.copy(), B.copy()
    A2[5], B2[5] = bad_model()
    with pytest.raises(capi.AlmpcError) as e:
        s.design_batched(A2, B2, Q, R, None, None, UMIN, UMAX)
    assert e.value.code == ERR_NUMERIC and "instance 5" in str(e.value)
    with pytest.raises(capi.AlmpcError) as e:   # R[1,1] == 0: the reference's branch rule drops R, no DARE is left
        s.design_batched(A, B, Q, np.diag([0.0, 0.1]), None, None, UMIN, UMAX)
    assert e.value.code == ERR_NUMERIC
    # mode 0 and a new design: the host loop again, the same weights to the tolerance of both
    s.set_terminal_weight("given")
    s.design_batched(A, B, Q, R, None, None, UMIN, UMAX)
    assert np.abs(s.terminal_weight_instance(7) - Ps[7]).max() <= P_RTOL * np.abs(Ps[7]).max()
    s.close()


# ---- almpc_set_terminal_weight: the re-linearisation pipeline -----------------------------------------------------------------------

X_REF0, U_REF0 = np.array([0.2, -0.1, 0.05, 0.0]), np.array([0.1, -0.2])


def _network(mo, kind, act):
    if kind == "densenet":
        import densenet_ref
        return densenet_ref.synthetic_densenet(act=act)
    if kind == "fnn":
        return mo.synthetic_fnn(act=act)
    import net_ref
    return net_ref.synthetic_net(kind, act=act)


def _linearize(capi, f, kind, X, u):
    U = np.repeat(np.asarray(u)[None], X.shape[0], 0)
    if kind == "densenet":
        return capi.densenet_linearize(f.W_in, f.W_h, f.b_h, f.W_out, X, U, act=f.act)
    return capi.fnn_linearize(f.W_in, f.W_h, f.b_h, f.W_out, X, U, act=f.act, net=kind)


def _relin_handle(capi, f, kind, batch, N, structured=False, mode="dare_device", S=None, box=None, terminal="none", group=False, P=None):
    n, m = 4, 2
    x_ref = X_REF0[:, None] * np.ones((n, N + 1))
    u_ref = U_REF0[:, None] * np.ones((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    if P is None:   # the reference's rule: the DARE of the linearisation at the last reference
        Al, Bl = f.jacobian(x_ref[:, -1], u_ref[:, -1])
        P = capi.dare(Al, Bl, Q, R)
    s = capi.Group(n, m, N, batch, devices=[0, 0], structured=structured) if group else capi.Solver(n, m, N, batch, structured=structured)
    s.set_terminal_weight(mode)
    kw = dict(act=f.act, xmin=None if box is None else -box, xmax=box, terminal=terminal)
    if kind == "densenet":
        s.relin_densenet_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, S, P, UMIN, UMAX, **kw)
    else:
        s.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, S, P, UMIN, UMAX, net=kind, **kw)
    return s, x_ref, u_ref, Q, R, P


def _check_relin_step(capi, mo, s, f, kind, X, r, N, x_ref, u_ref, Q, R, s_rate=0.0, box=None, terminal="none", label=""):
    """After a step from the states X: terminal weights = scipy's DARE of the library's own linearisation, u = the exact oracle's on
    that per-instance problem (or both say infeasible), terminal status all 0."""
    b = X.shape[0]
    A, B = _linearize(capi, f, kind, X, u_ref[:, 0])
    assert np.all(s.relin_terminal_status() == 0)
    worst_p = worst_u = 0.0
    ninf = 0
    for i in range(b):
        Ps = scipy_dare(A[i], B[i], Q, R)
        worst_p = max(worst_p, np.abs(s.terminal_weight_instance(i) - Ps).max() / np.abs(Ps).max())
        p = mo.make_problem(A[i], B[i], N, UMIN, UMAX, x_ref=x_ref, u_ref=u_ref, s=s_rate, P=Ps,
                            x_min=None if box is None else -box, x_max=box, terminal=terminal)
        try:
            e = mo.solve_mpc_exact(p, X[i])
        except ValueError:
            assert r["status"][i] == 3, (label, i, r["status"][i])
            ninf += 1
            continue
        assert r["status"][i] == 0, (label, i, r["status"][i])
        worst_u = max(worst_u, np.abs(r["u"][i] - e["u"]).max())
    print(f"relin {label}: max relative error of P {worst_p:.3e}, max |u - u*| {worst_u:.3e}, infeasible {ninf} of {b}")
    assert worst_p <= P_RTOL
    assert worst_u <= U_TOL
    return ninf


RELIN_CASES = [   # kind, activation, structured, N, S, state box + terminal equality
    ("fnn", "tanh", False, 10, None, False), ("fnn", "relu", False, 10, None, False),
    ("fnn", "tanh", True, 20, None, False), ("fnn", "relu", True, 20, None, False),
    ("fnn", "tanh", False, 10, None, True), ("fnn", "tanh", True, 20, None, True),
    ("fnn", "tanh", False, 10, 0.3, False), ("fnn", "tanh", True, 20, 0.3, False),
    ("resnet", "tanh", False, 10, None, False), ("densenet", "tanh", False, 10, None, False),
]


@pytest.mark.parametrize("kind,act,structured,N,S,rows", RELIN_CASES)
def test_relin_pipeline_solves_every_step_with_its_own_terminal_weights(capi, mo, kind, act, structured, N, S, rows):
    b, n, m = 33, 4, 2
    f = _network(mo, kind, act)
    box = np.array([1.5, 1.5, 1.5, 1.5]) if rows else None
    terminal = "equality" if rows else "none"
    s, x_ref, u_ref, Q, R, _ = _relin_handle(capi, f, kind, b, N, structured, S=None if S is None else S * np.eye(m), box=box, terminal=terminal)
    X0 = np.random.default_rng(11).uniform(-1.0, 1.0, (b, n))
    s.update_initialization(X0)
    s.relin_fnn_step(capi.default_opts())
    r = s.get_results()
    label = f"{kind} {act} structured {structured} N {N} S {S} rows {rows}"
    kw = dict(s_rate=0.0 if S is None else S, box=box, terminal=terminal)
    _check_relin_step(capi, mo, s, f, kind, X0, r, N, x_ref, u_ref, Q, R, label=label + " cold", **kw)
    # the closed loop of the network itself, then a warm step: the same checks at the new states
    s.relin_fnn_advance()
    s.relin_fnn_step(capi.default_opts(warm_start=1))
    r2 = s.get_results()
    X1 = r2["x"][:, :, 0].copy()
    moved = r["status"] == 0
    assert np.abs(X1[moved] - np.stack([f.forward(X0[i], r["u"][i][:, 0]) for i in np.nonzero(moved)[0]])).max() <= 1e-12
    _check_relin_step(capi, mo, s, f, kind, X1, r2, N, x_ref, u_ref, Q, R, label=label + " warm", **kw)
    s.close()


def _no_input_network(mo, act="relu"):
    """synthetic_fnn with the two input columns of W_in zeroed (B_i = 0) and W_out scaled so that the Jacobian at the origin has
    spectral radius 1.2: an unstable mode no input reaches, no stabilising solution."""
    f = mo.synthetic_fnn(act=act)
    f.W_in = f.W_in.copy()
    f.W_in[:, 4:] = 0.0
    A0, _ = f.jacobian(np.zeros(4), np.zeros(2))
    f.W_out = f.W_out * (1.2 / np.abs(np.linalg.eigvals(A0)).max())
    return f


@pytest.mark.parametrize("act", ["identity", "relu"])
@pytest.mark.parametrize("structured,N", [(False, 10), (True, 20)])
def test_an_instance_without_a_solution_falls_back_to_the_setups_weight(capi, mo, structured, N, act):
    """B_i = 0 everywhere.  With the identity activation every Jacobian is the one at the origin (spectral radius 1.2): no instance has
    a stabilising solution, every terminal status is 1 and the step is bit for bit the step of a handle set up with the mode off.
    With relu the Jacobian changes with x0 and some linearisations are stable -- those have a solution (B = 0: the Lyapunov
    equation's) and must get it; the others must fall back, and they still equal the mode-off handle bit for bit."""
    b, n = 33, 4
    f = _no_input_network(mo, act)
    g = mo.synthetic_fnn()   # (the setup's P: the weight of the network that still has its inputs)
    Q, R = 100.0 * np.eye(4), 0.1 * np.eye(2)
    P = capi.dare(*g.jacobian(X_REF0, U_REF0), Q, R)
    X0 = np.random.default_rng(11).uniform(-1.0, 1.0, (b, n))
    A, B = _linearize(capi, f, "fnn", X0, U_REF0)
    assert not B.any()
    unstable = np.array([np.abs(np.linalg.eigvals(A[i])).max() >= 1.0 for i in range(b)])
    if act == "identity":
        assert unstable.all()
    out = {}
    for mode in ("dare_device", "given"):
        s, *_ = _relin_handle(capi, f, "fnn", b, N, structured, mode=mode, P=P)
        s.update_initialization(X0)
        s.relin_fnn_step(capi.default_opts())
        out[mode] = s.get_results()
        if mode == "dare_device":
            st = s.relin_terminal_status()
            print(f"fallback, {act}, structured {structured}: {int(st.sum())} of {b} instances took the setup's weight")
            assert np.array_equal(st == 1, unstable)
            for i in range(b):
                want = P if unstable[i] else scipy_dare(A[i], B[i], Q, R)
                assert np.abs(s.terminal_weight_instance(i) - want).max() <= (0.0 if unstable[i] else P_RTOL * np.abs(want).max()), i
        else:
            with pytest.raises(capi.AlmpcError):
                s.relin_terminal_status()
        s.close()
    for k in ("x", "u", "status"):
        assert np.array_equal(out["dare_device"][k][unstable], out["given"][k][unstable]), k


def test_group_equals_one_handle(capi, mo):
    b, N, n = 33, 10, 4
    f = mo.synthetic_fnn(act="tanh")
    X0 = np.random.default_rng(11).uniform(-1.0, 1.0, (b, n))
    one, *_ = _relin_handle(capi, f, "fnn", b, N)
    g, *_ = _relin_handle(capi, f, "fnn", b, N, group=True)
    one.update_initialization(X0); g.update_initialization(X0, resident=True)
    for step in range(2):
        o = None if step == 0 else capi.default_opts(warm_start=1)
        one.relin_fnn_step(o); g.relin_fnn_step(o)
        a, c = one.get_results(), g.get_results()
        for k in ("status", "u", "x", "iters", "polish_iters"):
            assert np.array_equal(a[k], c[k]), (step, k)
        assert np.array_equal(one.relin_terminal_status(), g.relin_terminal_status())
        for i in (0, 16, 17, 32):
            assert np.array_equal(one.terminal_weight_instance(i), g.terminal_weight_instance(i)), i
        one.relin_fnn_advance(); g.relin_fnn_advance()
    one.close(); g.close()


def test_mirror_terminal_weight_step(pkg, capi, mo):
    """proceed_controller(..., mpc_linearization="step", mpc_terminal_weight="step"): two closed-loop steps equal the C ABI's."""
    f = mo.synthetic_fnn(act="tanh")
    sys_ = pkg.ConstrainedBlackBoxControlDiscreteSystem(pkg.Fnn(f.W_in, f.W_h, f.b_h, f.W_out, f.act), 4, 2,
                                                        pkg.Hyperrectangle([-10] * 4, [10] * 4), pkg.Hyperrectangle(UMIN, UMAX))
    b, N = 33, 10
    C = pkg.proceed_controller(sys_, "model_predictive_control", N, 1, list(X_REF0), list(U_REF0), mpc_batch=b,
                               mpc_linearization="step", mpc_terminal_weight="step")
    mod = C.tuning.modeler
    s, *_ = _relin_handle(capi, f, "fnn", b, N)
    X = np.random.default_rng(11).uniform(-1.0, 1.0, (b, 4))
    for step in range(2):
        res = pkg._model_predictive_control_computation(C, X)
        s.update_initialization(X)
        s.relin_fnn_step(mod.opts)
        r = s.get_results()
        assert np.array_equal(res.u, r["u"]) and np.array_equal(res.x, r["x"]), step
        assert np.array_equal(mod.solver.relin_terminal_status(), s.relin_terminal_status())
        assert np.array_equal(mod.solver.terminal_weight_instance(3), s.terminal_weight_instance(3))
        X = np.stack([f.forward(X[i], r["u"][i][:, 0]) for i in range(b)])
    mod.solver.close(); s.close()
    with pytest.raises(ValueError):
        pkg.proceed_controller(sys_, "model_predictive_control", N, 1, list(X_REF0), list(U_REF0), mpc_batch=b, mpc_terminal_weight="step")
