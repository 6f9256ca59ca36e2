"""GPU tests of k_c2d (csrc/almpc_c2d.hip.h): the batched zero-order hold almpc_c2d_batched against scipy's expm of the augmented
matrix, and the continuous-time models it gives almpc_design_shared, almpc_design_batched and the re-linearisation pipeline
(almpc_set_model_time).  Shared definitions: tests/c2d_ref.py.

Tolerances.  A discretised model: max|X - X_scipy| / max(1, max|X_scipy|) <= 1e-10 for A_d and B_d (the host function, the same
algorithm in FP64, measures at most 5.4e-13 on these inputs).  A terminal weight: 1e-9 relative against scipy's DARE of scipy's
discretisation (the bound of tests/test_gpu_dare.py).  A solution: |u - u*|_inf <= 1e-5 against the exact oracle on the
scipy-discretised problem."""
import importlib

import numpy as np
import pytest
import scipy.linalg as sla

import c2d_ref as cr

pytestmark = pytest.mark.gpu

P_RTOL = 1e-9
U_TOL = 1e-5
ERR_INVALID, ERR_UNSUPPORTED, ERR_NUMERIC = -1, -4, -6
UMIN, UMAX = [-1.0, -1.0], [1.0, 1.0]
TS = 0.25


def _worst(Ad, Bd, Ad_t, Bd_t):
    return max(cr.c2d_error(Ad[i], Bd[i], Ad_t[i], Bd_t[i]) for i in range(Ad.shape[0]))


@pytest.mark.parametrize("n,m", cr.SHAPES)
def test_c2d_batched_matches_scipy(capi, n, m):
    """n = 17, 33 cross the lanes-per-column tiers, (64, 16) is the LDS limit (one instance per workgroup)."""
    A, B = cr.models(n, m)
    for Ts in cr.SAMPLE_TIMES:
        Ad, Bd, st = capi.c2d_batched(A, B, Ts)
        assert np.all(st == 0), np.nonzero(st)[0]
        worst = _worst(Ad, Bd, *cr.truth(n, m, Ts))
        print(f"n {n} m {m} Ts {Ts}: max error against scipy {worst:.3e}")
        assert worst <= cr.TOL


def test_c2d_batched_perturbed_quadrotors(capi, pkg):
    wl = importlib.import_module(pkg.__name__ + ".workloads")
    Ac, Bc = wl.quadrotor_continuous_model()
    rng = np.random.default_rng(7)
    A = Ac[None] * (1.0 + rng.uniform(-0.05, 0.05, (256, 12, 12)))
    B = Bc[None] * (1.0 + rng.uniform(-0.05, 0.05, (256, 12, 4)))
    Ad, Bd, st = capi.c2d_batched(A, B, 0.1)
    assert np.all(st == 0)
    truth = [cr.zoh_scipy(A[i], B[i], 0.1) for i in range(256)]
    worst = _worst(Ad, Bd, [t[0] for t in truth], [t[1] for t in truth])
    print(f"256 perturbed quadrotors, Ts 0.1: max error against scipy {worst:.3e}")
    assert worst <= cr.TOL


def test_failing_instances_are_reported_and_leave_the_others_alone(capi):
    A, B = cr.models(4, 2, 40)
    A2 = A.copy()
    A2[3, 1, 2] = np.nan
    A2[17] = 1e300 * A[17]
    sentinel = (np.full((40, 4, 4), -12345.678), np.full((40, 4, 2), -12345.678))
    Ag, Bg, stg = capi.c2d_batched(A, B, 1.0, out_init=sentinel)
    A_, B_, st2 = capi.c2d_batched(A2, B, 1.0, out_init=sentinel)
    assert np.all(stg == 0)
    assert sorted(np.nonzero(st2)[0].tolist()) == [3, 17]
    keep = np.ones(40, dtype=bool)
    keep[[3, 17]] = False
    assert np.array_equal(A_[~keep], sentinel[0][~keep]) and np.array_equal(B_[~keep], sentinel[1][~keep])   # a failed instance's slots are not written
    assert np.array_equal(A_[keep], Ag[keep]) and np.array_equal(B_[keep], Bg[keep])   # bit-identical: no instance depends on its neighbours


def test_limits(capi):
    for n, m, Ts, code in ((65, 2, 1.0, ERR_UNSUPPORTED), (4, 17, 1.0, ERR_UNSUPPORTED), (4, 2, -1.0, ERR_INVALID)):
        with pytest.raises(capi.AlmpcError) as e:
            capi.c2d_batched(np.zeros((3, n, n)), np.zeros((3, n, m)), Ts)
        assert e.value.code == code, (n, m, Ts)


# ---- almpc_set_model_time: almpc_design_shared ---------------------------------------------------------------------------------------

def test_design_shared_discretises_the_continuous_quadrotor(capi, pkg, mo):
    wl = importlib.import_module(pkg.__name__ + ".workloads")
    Ac, Bc = wl.quadrotor_continuous_model()
    p = mo.quadrotor(N=10)   # the scipy-discretised problem
    b = 33
    s = capi.Solver(p.n, p.m, p.N, b)
    s.set_model_time("continuous", 0.1)
    s.design_shared(Ac, Bc, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    Ad, Bd = s.model_instance(0)
    err = cr.c2d_error(Ad, Bd, *wl.quadrotor_model())
    print(f"design_shared: model error {err:.3e}")
    assert err <= cr.TOL
    X0 = mo.quadrotor_x0_batch(b, 1.0)
    s.set_reference(p.x_ref, p.u_ref)
    s.update_initialization(X0)
    s.calculate()
    r = s.get_results()
    assert np.all(r["status"] == 0), np.bincount(r["status"])
    worst = max(np.abs(r["u"][i] - mo.solve_mpc_exact(p, X0[i])["u"]).max() for i in range(b))
    print(f"design_shared: max |u - u*| {worst:.3e}")
    assert worst <= U_TOL
    # the handle holds the discrete model: almpc_advance_plant steps it
    s.advance_plant()
    s.calculate()
    x1 = s.get_results()["x"][:, :, 0]
    want = np.stack([p.A @ X0[i] + p.B @ r["u"][i][:, 0] for i in range(b)])
    assert np.abs(x1 - want).max() <= 1e-9
    s.close()


# ---- almpc_set_model_time: almpc_design_batched --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dare_device", [False, True])
@pytest.mark.parametrize("structured", [False, True])
def test_design_batched_discretises_its_models_on_the_device(capi, mo, structured, dare_device):
    n, m, N, b = 4, 2, 10, 33
    A, B = cr.models(n, m, b)
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    truth = [cr.zoh_scipy(A[i], B[i], TS) for i in range(b)]
    Ps = [sla.solve_discrete_are(truth[i][0], truth[i][1], Q, R) for i in range(b)]
    X0 = np.random.default_rng(5).uniform(-1.0, 1.0, (b, n))
    s = capi.Solver(n, m, N, b, structured=structured)
    s.set_model_time("continuous", TS)
    s.set_terminal_weight("dare_device" if dare_device else "given")
    s.design_batched(A, B, Q, R, None, None, UMIN, UMAX)
    worst_m = worst_p = 0.0
    for i in range(b):
        worst_m = max(worst_m, cr.c2d_error(*s.model_instance(i), *truth[i]))
        worst_p = max(worst_p, np.abs(s.terminal_weight_instance(i) - Ps[i]).max() / np.abs(Ps[i]).max())
    s.update_initialization(X0)
    s.calculate()
    r = s.get_results()
    assert np.all(r["status"] == 0), np.bincount(r["status"])
    worst_u = 0.0
    for i in range(b):
        e = mo.solve_mpc_exact(mo.make_problem(truth[i][0], truth[i][1], N, UMIN, UMAX, P=Ps[i]), X0[i])
        worst_u = max(worst_u, np.abs(r["u"][i] - e["u"]).max())
    print(f"design_batched, structured {structured}, dare_device {dare_device}: model {worst_m:.3e}, P {worst_p:.3e}, max |u - u*| {worst_u:.3e}")
    assert worst_m <= cr.TOL and worst_p <= P_RTOL and worst_u <= U_TOL
    # a model that is not finite: the error names the instance
    A2 = A.copy()
    A2[5, 0, 1] = np.nan
    with pytest.raises(capi.AlmpcError) as e:
        s.design_batched(A2, B, Q, R, None, None, UMIN, UMAX)
    assert e.value.code == ERR_NUMERIC and "instance 5" in str(e.value)
    # mode 0 and a new design: the models are discrete again -- the same numbers from scipy's discretisation
    s.set_model_time("discrete")
    Ad, Bd = np.stack([t[0] for t in truth]), np.stack([t[1] for t in truth])
    s.design_batched(Ad, Bd, Q, R, None, None, UMIN, UMAX)
    assert np.array_equal(s.model_instance(7)[0], Ad[7]) and np.array_equal(s.model_instance(7)[1], Bd[7])
    s.update_initialization(X0)
    s.calculate()
    r2 = s.get_results()
    assert np.all(r2["status"] == 0)
    assert np.abs(r2["u"] - r["u"]).max() <= 2.0 * U_TOL
    s.close()


# ---- almpc_set_model_time: the re-linearisation pipeline ------------------------------------------------------------------------------

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


def _setup_weight(capi, f, kind, x_ref, u_ref, Q, R, Ts=TS):
    """The setup's P: the DARE of the discretised linearisation at the last reference, all by the library's own calls."""
    Al, Bl = _linearize(capi, f, kind, x_ref[:, -1][None], u_ref[:, -1])
    return capi.dare(*capi.c2d(Al[0], Bl[0], Ts), Q, R)


def _relin_handle(capi, f, kind, batch, N, structured=False, dare_device=False, group=False, Ts=TS):
    n, m = 4, 2
    x_ref = X_REF0[:, None] * np.ones((n, N + 1))
    u_ref = U_REF0[:, None] * np.ones((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    P = _setup_weight(capi, f, kind, x_ref, u_ref, Q, R, Ts)
    s = capi.Group(n, m, N, batch, devices=[0, 0], structured=structured) if group else capi.Solver(n, m, N, batch, structured=structured)
    s.set_model_time("continuous", Ts)
    s.set_terminal_weight("dare_device" if dare_device else "given")
    if kind == "densenet":
        s.relin_densenet_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, UMIN, UMAX, act=f.act)
    else:
        s.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, UMIN, UMAX, net=kind, act=f.act)
    return s, x_ref, u_ref, Q, R, P


def _check_relin_step(capi, mo, s, f, kind, X, r, N, x_ref, u_ref, Q, R, P, dare_device, label):
    """After a step from the states X: the model slots hold scipy's discretisation of the library's own continuous Jacobians, every
    status is 0, u is the exact oracle's on that per-instance problem with the setup's P or scipy's per-instance DARE.

    relu only: a Jacobian that lost rank (dead units) has an eigenvalue 0, its zero-order hold an eigenvalue exactly 1, and where no
    input reaches it the DARE has NO stabilising solution, so there is no reference for the weight.  Of the 33 + 33 states of this
    test that is instance 6 of the cold draw and 22 of the warm one (scipy raises) and instance 20 of the warm one (scipy and hm::dare
    both return a "solution" of magnitude 4e10 and 3e10 whose closed loop has spectral radius 1.000000000000, and they differ by
    20 %).  What a solver makes of such a model is decided by rounding: hm::dare refuses instances 6 and 22, k_dare (FMA contraction)
    refuses 6 and accepts 22 with a weight of 1e10 -- its acceptance test is the residual relative to max|P| (open
    item 8), not this change's to settle.  So an instance is "without a reference" when scipy raises or its solution is not
    stabilising (closed-loop radius >= 1 - 1e-8), there are at most two per draw and only with relu, and such an instance is checked
    for its model -- and, where the library did report terminal status 1, for the setup's P bit for bit and the solution with it."""
    b = X.shape[0]
    Ac, Bc = _linearize(capi, f, kind, X, u_ref[:, 0])
    tstat = s.relin_terminal_status() if dare_device else np.zeros(b, dtype=np.int32)
    worst_m = worst_u = 0.0
    ill = []
    for i in range(b):
        Ad, Bd = cr.zoh_scipy(Ac[i], Bc[i], TS)
        worst_m = max(worst_m, cr.c2d_error(*s.model_instance(i), Ad, Bd))
        Pi = P
        if dare_device:
            try:
                Pi = sla.solve_discrete_are(Ad, Bd, Q, R)
                K = np.linalg.solve(R + Bd.T @ Pi @ Bd, Bd.T @ Pi @ Ad)
                stabilising = np.abs(np.linalg.eigvals(Ad - Bd @ K)).max() < 1.0 - 1e-8
            except np.linalg.LinAlgError:
                stabilising = False
            if stabilising:
                assert tstat[i] == 0, (label, i)
                assert np.abs(s.terminal_weight_instance(i) - Pi).max() <= P_RTOL * np.abs(Pi).max(), (label, i)
            else:
                ill.append(i)
                if tstat[i] != 1:
                    continue
                Pi = P
                assert np.array_equal(s.terminal_weight_instance(i), P), (label, i)
        e = mo.solve_mpc_exact(mo.make_problem(Ad, Bd, N, UMIN, UMAX, x_ref=x_ref, u_ref=u_ref, P=Pi), X[i])
        assert r["status"][i] == 0, (label, i, r["status"][i])
        worst_u = max(worst_u, np.abs(r["u"][i] - e["u"]).max())
    print(f"relin {label}: model {worst_m:.3e}, max |u - u*| {worst_u:.3e}, setup's P for {int(tstat.sum())} of {b}, no stabilising DARE reference: {ill}")
    assert worst_m <= cr.TOL
    assert not ill or ("relu" in label and len(ill) <= 2)
    assert worst_u <= U_TOL


RELIN_CASES = [   # kind, activation, structured, N
    ("fnn", "tanh", False, 10), ("fnn", "relu", False, 10), ("resnet", "tanh", False, 10), ("polynet", "tanh", False, 10),
    ("densenet", "tanh", False, 10), ("fnn", "tanh", True, 20),
]


@pytest.mark.parametrize("dare_device", [False, True])
@pytest.mark.parametrize("kind,act,structured,N", RELIN_CASES)
def test_relin_pipeline_discretises_every_steps_jacobians(capi, mo, kind, act, structured, N, dare_device):
    b, n = 33, 4
    f = _network(mo, kind, act)
    s, x_ref, u_ref, Q, R, P = _relin_handle(capi, f, kind, b, N, structured, dare_device)
    label = f"{kind} {act} structured {structured} N {N} dare_device {dare_device}"
    X0 = np.random.default_rng(11).uniform(-1.0, 1.0, (b, n))
    s.update_initialization(X0)
    s.relin_fnn_step(capi.default_opts())
    _check_relin_step(capi, mo, s, f, kind, X0, s.get_results(), N, x_ref, u_ref, Q, R, P, dare_device, label + " cold")
    # the plant of a continuous network is the caller's integrator: no advance; a warm step from new states of the caller's
    with pytest.raises(capi.AlmpcError) as e:
        s.relin_fnn_advance()
    assert e.value.code == ERR_UNSUPPORTED
    X1 = np.random.default_rng(12).uniform(-1.0, 1.0, (b, n))
    s.update_initialization(X1)
    s.relin_fnn_step(capi.default_opts(warm_start=1))
    _check_relin_step(capi, mo, s, f, kind, X1, s.get_results(), N, x_ref, u_ref, Q, R, P, dare_device, label + " warm")
    s.close()


def test_refusals_with_the_mode_on(capi, mo):
    f = mo.synthetic_fnn(act="tanh")
    n, m, N, b = 4, 2, 10, 5
    x_ref, u_ref = X_REF0[:, None] * np.ones((n, N + 1)), U_REF0[:, None] * np.ones((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    P = _setup_weight(capi, f, "fnn", x_ref, u_ref, Q, R)
    s = capi.Solver(n, m, N, b)
    s.set_model_time("continuous", TS)
    with pytest.raises(capi.AlmpcError) as e:
        s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, UMIN, UMAX, act="tanh")
    assert e.value.code == ERR_UNSUPPORTED
    A = np.zeros((b, N, n, n))
    B = np.zeros((b, N, n, m))
    with pytest.raises(capi.AlmpcError) as e:
        s.design_ltv(A, B, None, np.zeros((b, n, N + 1)), np.zeros((b, m, N)), x_ref, u_ref, Q, R, None, P, UMIN, UMAX)
    assert e.value.code == ERR_UNSUPPORTED
    with pytest.raises(capi.AlmpcError) as e:
        s.set_model_time("continuous", 0.0)
    assert e.value.code == ERR_INVALID
    s.close()


def test_group_equals_one_handle(capi, mo):
    b, N, n = 33, 10, 4
    f = mo.synthetic_fnn(act="tanh")
    one, *_ = _relin_handle(capi, f, "fnn", b, N)
    g, *_ = _relin_handle(capi, f, "fnn", b, N, group=True)
    for step, seed in enumerate((11, 12)):
        X = np.random.default_rng(seed).uniform(-1.0, 1.0, (b, n))
        one.update_initialization(X); g.update_initialization(X)
        o = None if step == 0 else capi.default_opts(warm_start=1)
        one.relin_fnn_step(o); g.relin_fnn_step(o)
        a, c = one.get_results(), g.get_results()
        for k in ("status", "u", "x"):
            assert np.array_equal(a[k], c[k]), (step, k)
        for i in (0, 16, 17, 32):
            for Ma, Mc in zip(one.model_instance(i), g.model_instance(i)):
                assert np.array_equal(Ma, Mc), (step, i)
    one.close(); g.close()


# ---- the mirror -------------------------------------------------------------------------------------------------------------------------

def test_mirror_linear_continuous_system(pkg, capi, mo):
    """proceed_controller on a ConstrainedLinearControlContinuousSystem = the controller of the scipy-discretised discrete system.
    The mirror's sample time is an Int: the quadrotor in units of 0.1 s (0.1 Ac, 0.1 Bc) at mpc_sample_time = 1 is the benchmark plant."""
    wl = importlib.import_module(pkg.__name__ + ".workloads")
    Ac, Bc = wl.quadrotor_continuous_model()
    Ac, Bc = 0.1 * Ac, 0.1 * Bc
    p = mo.quadrotor(N=10)
    X, U = pkg.Hyperrectangle([-10.0] * 12, [10.0] * 12), pkg.Hyperrectangle(p.u_min, p.u_max)
    b = 33
    X0 = mo.quadrotor_x0_batch(b, 1.0)
    out = []
    for sys_, Ts in ((pkg.ConstrainedLinearControlContinuousSystem(Ac, Bc, X, U), 1), (pkg.ConstrainedLinearControlDiscreteSystem(*cr.zoh_scipy(Ac, Bc, 1.0), X, U), 1)):
        C = pkg.proceed_controller(sys_, "model_predictive_control", 10, Ts, [0.0] * 12, [0.0] * 4, mpc_batch=b)
        out.append(np.array(pkg._model_predictive_control_computation(C, X0).u))
        assert isinstance(C.system, pkg.ConstrainedLinearControlDiscreteSystem)
        C.tuning.modeler.solver.close()
    diff = np.abs(out[0] - out[1]).max()
    print(f"mirror, linear continuous system: max |u - u(scipy-discretised)| {diff:.3e}")
    assert diff <= 1e-9


def test_mirror_black_box_continuous_system_step(pkg, capi, mo):
    """mpc_linearization = "step" with a ConstrainedBlackBoxControlContinuousSystem: two steps equal the C ABI pipeline bit for bit.
    The mirror's sample time is an Int: the network in units of 0.25 s (W_out / 4) at mpc_sample_time = 1 is the network of the tests
    above at Ts = 0.25."""
    f = mo.synthetic_fnn(act="tanh")
    f.W_out = 0.25 * f.W_out
    sys_ = pkg.ConstrainedBlackBoxControlContinuousSystem(pkg.Fnn(f.W_in, f.W_h, f.b_h, f.W_out, f.act), 4, 2,
                                                          pkg.Hyperrectangle([-10] * 4, [10] * 4), pkg.Hyperrectangle(UMIN, UMAX))
    b, N = 33, 10
    C = pkg.proceed_controller(sys_, "model_predictive_control", N, 1, list(X_REF0), list(U_REF0), mpc_batch=b, mpc_linearization="step")
    mod = C.tuning.modeler
    s, *_ = _relin_handle(capi, f, "fnn", b, N, Ts=1.0)
    for seed in (11, 12):
        X = np.random.default_rng(seed).uniform(-1.0, 1.0, (b, 4))
        res = pkg._model_predictive_control_computation(C, X)
        s.update_initialization(X)
        s.relin_fnn_step(mod.opts)
        r = s.get_results()
        assert np.array_equal(res.u, r["u"]) and np.array_equal(res.x, r["x"]), seed
        for Ma, Mc in zip(mod.solver.model_instance(3), s.model_instance(3)):
            assert np.array_equal(Ma, Mc)
    mod.solver.close(); s.close()
