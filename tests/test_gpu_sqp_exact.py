"""GPU tests of the exact-Hessian mode of the Fnn SQP loop (almpc_sqp_fnn_set_hessian(h, ALMPC_SQP_HESSIAN_EXACT)): the device's exact
QP against the restatement tests/sqp_exact_ref.py, and tolerance solves against its outcome on the benchmark batch
(tests/golden/fnn_sqp_solve_exact.json)."""
import json
import os

import numpy as np
import pytest

import sqp_exact_ref as ex
import sqp_solve_ref as ref
from test_gpu_sqp_solve import _nlp_kkt, _solver

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_one_exact_iteration_builds_the_restatements_qp(capi, mo):
    """The QP of the first exact iteration (stage Hessians from the device multipliers, condensed, plus the active-bound shift) is the
    restatement's at 1e-10 relative: this covers W_k and lam of every stage."""
    b, N = 8, 50
    f, kw, X0 = ref.bench_setup(b=b, N=N)
    s = _solver(capi, kw, f, b, N)
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


def test_exact_solve_at_the_benchmark_batch(capi, mo):
    """256 instances, N 50, solve(30, 1e-6) in exact mode: the restatement's verdicts (255 converged, instance 69 at the limit),
    iteration counts within one of it, and the oracle's certificate on every converged instance."""
    fx = json.load(open(os.path.join(GOLDEN, "fnn_sqp_solve_exact.json")))
    f, kw, X0 = ref.bench_setup()
    s = _solver(capi, kw, f, 256, 50)
    s.sqp_fnn_set_hessian("exact")
    s.sqp_fnn_start(X0)
    out = s.sqp_fnn_solve(fx["max_iters"], fx["tol"])
    r = s.get_results(want=("u", "x"))
    s.close()
    want = np.array(fx["status"])
    assert np.array_equal(out["status"], want), np.nonzero(out["status"] != want)
    d = np.abs(out["iters"] - np.array(fx["iters"]))
    assert np.all(d <= 1), (np.nonzero(d > 1), out["iters"][d > 1])
    for i in np.nonzero(want == 0)[0]:
        assert np.abs(r["x"][i] - mo.fnn_rollout(f, X0[i], r["u"][i])).max() <= 1e-9
        assert _nlp_kkt(mo, f, kw, X0[i], r["u"][i]) <= fx["tol"] + 1e-9, i


def test_exact_group_of_two_equals_one_handle(capi, mo):
    f, kw, X0 = ref.bench_setup(b=40, N=30)
    s = _solver(capi, kw, f, 40, 30)
    s.sqp_fnn_set_hessian("exact")
    s.sqp_fnn_start(X0)
    one = s.sqp_fnn_solve(20, 1e-6)
    r1 = s.get_results(want=("u",))
    s.close()
    g = capi.Group(4, 2, 30, 40, devices=[0, 0])
    g.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"],
                    kw["u_max"], act="tanh")
    g.sqp_fnn_set_hessian("exact")
    g.sqp_fnn_start(X0)
    two = g.sqp_fnn_solve(20, 1e-6)
    r2 = g.get_results()
    g.close()
    assert np.array_equal(one["status"], two["status"]) and np.array_equal(one["iters"], two["iters"])
    assert np.array_equal(r1["u"], r2["u"])


def test_exact_mode_refusals(capi, mo):
    f, kw, X0 = ref.bench_setup(b=4, N=10)
    s = capi.Solver(4, 2, 10, 4)   # state rows
    s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"],
                    act="tanh", xmin=-5 * np.ones(4), xmax=5 * np.ones(4))
    with pytest.raises(capi.AlmpcError) as ei:
        s.sqp_fnn_set_hessian("exact")
    assert ei.value.code == -4
    s.close()
    s = _solver(capi, kw, f, 4, 10, qp_solver="structured")
    with pytest.raises(capi.AlmpcError) as ei:
        s.sqp_fnn_set_hessian("exact")
    assert ei.value.code == -4
    s.close()
    fr = mo.synthetic_fnn(act="relu")
    s = capi.Solver(4, 2, 10, 4)
    s.sqp_fnn_setup(fr.W_in, fr.W_h, fr.b_h, fr.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"],
                    kw["u_max"], act="relu")
    with pytest.raises(capi.AlmpcError) as ei:
        s.sqp_fnn_set_hessian("exact")
    assert ei.value.code == -4
    s.close()


def test_mirror_exact_hessian_with_tolerance(pkg, mo):
    f = mo.synthetic_fnn(act="tanh")
    sys_ = pkg.ConstrainedBlackBoxControlDiscreteSystem(pkg.Fnn(f.W_in, f.W_h, f.b_h, f.W_out, f.act), 4, 2,
                                                        pkg.Hyperrectangle([-10] * 4, [10] * 4), pkg.Hyperrectangle([-1, -1], [1, 1]))
    x_ref, u_ref = [0.2, -0.1, 0.05, 0.0], [0.1, -0.2]
    N, batch = 20, 16
    C = pkg.proceed_controller(sys_, "model_predictive_control", N, 1, x_ref, u_ref, mpc_batch=batch, mpc_programming_type="non_linear",
                               mpc_sqp_hessian="exact", mpc_sqp_tolerance=1e-6, mpc_sqp_iterations=30)
    P = C.tuning.terminal_ingredient.P
    X0 = np.asarray(x_ref)[None, :] + 0.6 * mo.splitmix_normal(0x5EED0009, 0, batch, 4)
    res = pkg._model_predictive_control_computation(C, X0)
    mod = C.tuning.modeler
    assert np.all(mod.last_sqp_status == 0) and np.all(mod.last_sqp_kkt <= 1e-6)
    xr, ur = np.tile(np.array(x_ref)[:, None], (1, N + 1)), np.tile(np.array(u_ref)[:, None], (1, N))
    for i in range(batch):
        k = mo.nlp_kkt_residual(f, X0[i], res.u[i], xr, ur, 100 * np.eye(4), 0.1 * np.eye(2), np.zeros((2, 2)), P, -np.ones(2), np.ones(2))
        assert k <= 1e-6 + 1e-9
    mod.solver.close()
    with pytest.raises(ValueError):
        pkg.proceed_controller(sys_, "model_predictive_control", N, 1, x_ref, u_ref, mpc_programming_type="non_linear", mpc_sqp_hessian="newton")
