"""GPU tests of the tolerance-terminated SQP solve for Fnn models (almpc_sqp_fnn_solve): per-instance stopping test at the iterate,
frozen instances, per-instance verdicts.  Checked against the restatement tests/sqp_solve_ref.py (its outcome on the benchmark batch
is the fixture tests/golden/fnn_sqp_solve_gn.json, written by tests/golden/make_sqp_solve_fixture.py) and against the oracle's
method-independent first-order certificate nlp_kkt_residual."""
import json
import os

import numpy as np
import pytest

import sqp_solve_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _solver(capi, kw, f, b, N, qp_solver="condensed", R=None):
    s = capi.Solver(4, 2, N, b)
    s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"] if R is None else R, kw["S"], kw["P"],
                    kw["u_min"], kw["u_max"], act="tanh", qp_solver=qp_solver)
    return s


def _nlp_kkt(mo, f, kw, x0, U):
    return mo.nlp_kkt_residual(f, x0, U, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"])


def test_solve_at_the_benchmark_batch_matches_the_restatement(capi, mo):
    """256 instances, N 50, merit rule, 40 iterations, tol 1e-6: status 1 for exactly the instances the restatement leaves
    unconverged, status 0 with a certified KKT point for every other one, iteration counts within one of the restatement's."""
    fx = json.load(open(os.path.join(GOLDEN, "fnn_sqp_solve_gn.json")))
    f, kw, X0 = ref.bench_setup()
    s = _solver(capi, kw, f, 256, 50)
    s.sqp_fnn_start(X0)
    out = s.sqp_fnn_solve(fx["max_iters"], fx["tol"])
    r = s.get_results(want=("u", "x"))
    s.close()
    want = np.array(fx["status"])
    assert np.array_equal(out["status"], want), np.nonzero(out["status"] != want)
    assert np.all(np.abs(out["iters"] - np.array(fx["iters"])) <= 1), np.nonzero(np.abs(out["iters"] - np.array(fx["iters"])) > 1)
    assert np.all(out["iters"][want == 1] == fx["max_iters"])
    for i in range(256):
        if want[i] != 0:
            assert out["kkt"][i] > fx["tol"]
            continue
        assert out["kkt"][i] <= fx["tol"]
        U = r["u"][i]
        assert np.abs(r["x"][i] - mo.fnn_rollout(f, X0[i], U)).max() <= 1e-9
        k = _nlp_kkt(mo, f, kw, X0[i], U)
        assert k <= fx["tol"] + 1e-9, (i, k)
        assert abs(k - out["kkt"][i]) <= 1e-9 + 1e-6 * k, (i, k, out["kkt"][i])
    for i in (3, 42):   # the device iterate against the restatement's, one converged and one left at the limit
        rr = ref.sqp_solve(f, X0[i], kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"],
                           fx["max_iters"], fx["tol"])
        assert np.abs(r["u"][i] - rr["U"]).max() <= 1e-5


def test_stopping_test_at_the_start_is_the_oracle_residual(capi, mo):
    """A tolerance every start meets: the test at the start (the network's own rollout: zero defects) freezes every instance at once,
    its residual is the oracle's nlp_kkt_residual there, and the iterate is untouched."""
    f, kw, X0 = ref.bench_setup(b=16, N=30)
    s = _solver(capi, kw, f, 16, 30)
    s.sqp_fnn_start(X0)
    out = s.sqp_fnn_solve(3, 1e9)
    r = s.get_results(want=("u",))
    s.close()
    assert np.all(out["status"] == 0) and np.all(out["iters"] == 0)
    U0 = np.clip(kw["u_ref"], -1.0, 1.0)
    for i in range(16):
        assert np.abs(r["u"][i] - U0).max() == 0.0
        k = _nlp_kkt(mo, f, kw, X0[i], U0)
        assert abs(out["kkt"][i] - k) <= 1e-10 * k, (i, out["kkt"][i], k)


def test_converged_instances_are_frozen_bitwise(capi, mo):
    """An instance converged within k iterations has bit-identical results after k and after k + 5 iterations; the instances still
    live after k go on."""
    f, kw, X0 = ref.bench_setup(b=32)
    s = _solver(capi, kw, f, 32, 50)
    s.sqp_fnn_start(X0)
    a = s.sqp_fnn_solve(8, 1e-6)
    ra = s.get_results(want=("u", "x"))
    s.sqp_fnn_start(X0)
    b = s.sqp_fnn_solve(13, 1e-6)
    rb = s.get_results(want=("u", "x"))
    s.close()
    done = a["status"] == 0
    assert 0 < done.sum() < 32
    assert np.all(b["status"][done] == 0) and np.array_equal(a["iters"][done], b["iters"][done])
    assert np.array_equal(a["kkt"][done], b["kkt"][done])
    assert np.array_equal(ra["u"][done], rb["u"][done]) and np.array_equal(ra["x"][done], rb["x"][done])
    assert (b["status"][~done] == 0).sum() > 0 and np.any(ra["u"][~done] != rb["u"][~done])


def test_solve_on_the_structured_route_and_with_input_rate_weight(capi, mo):
    """The test is the same on the stage-wise QP route; with an input-rate weight S the gradient carries its terms."""
    f, kw, X0 = ref.bench_setup(b=24, N=20)
    s = _solver(capi, kw, f, 24, 20, qp_solver="structured")
    s.sqp_fnn_start(X0)
    out = s.sqp_fnn_solve(30, 1e-7)
    r = s.get_results(want=("u",))
    s.close()
    assert np.all((out["status"] == 0) | (out["status"] == 1)) and (out["status"] == 0).sum() >= 20
    for i in np.nonzero(out["status"] == 0)[0]:
        assert _nlp_kkt(mo, f, kw, X0[i], r["u"][i]) <= 1e-7 + 1e-9
    kwS = dict(kw, S=0.2 * np.eye(2))
    s = capi.Solver(4, 2, 20, 24)
    s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kwS["S"], kw["P"], kw["u_min"],
                    kw["u_max"], act="tanh")
    s.sqp_fnn_start(X0)
    out = s.sqp_fnn_solve(1, 1e9)
    s.close()
    for i in range(24):
        k = _nlp_kkt(mo, f, kwS, X0[i], np.clip(kw["u_ref"], -1.0, 1.0))
        assert abs(out["kkt"][i] - k) <= 1e-10 * k


def test_solve_error_behaviour(capi, mo):
    f, kw, X0 = ref.bench_setup(b=4, N=10)
    s = _solver(capi, kw, f, 4, 10)
    with pytest.raises(capi.AlmpcError) as ei:
        s.sqp_fnn_solve(5, 1e-6)          # not started
    assert ei.value.code == -5
    s.sqp_fnn_start(X0)
    for bad in ((0, 1e-6), (5, 0.0), (5, -1.0)):
        with pytest.raises(capi.AlmpcError) as ei:
            s.sqp_fnn_solve(*bad)
        assert ei.value.code == -1
    s.close()
    s = _solver(capi, kw, f, 4, 10, R=np.zeros((2, 2)))   # the residual divides by 2 R_aa
    s.sqp_fnn_start(X0)
    with pytest.raises(capi.AlmpcError) as ei:
        s.sqp_fnn_solve(5, 1e-6)
    assert ei.value.code == -4
    s.sqp_fnn_iterate(2)                  # the fixed-count loop still runs on such a handle
    s.close()


def test_group_of_two_equals_one_handle(capi, mo):
    f, kw, X0 = ref.bench_setup(b=40, N=30)
    s = _solver(capi, kw, f, 40, 30)
    s.sqp_fnn_start(X0)
    one = s.sqp_fnn_solve(25, 1e-6)
    r1 = s.get_results(want=("u",))
    s.close()
    g = capi.Group(4, 2, 30, 40, devices=[0, 0])
    g.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"],
                    kw["u_max"], act="tanh")
    g.sqp_fnn_start(X0)
    two = g.sqp_fnn_solve(25, 1e-6)
    r2 = g.get_results()
    g.close()
    assert np.array_equal(one["status"], two["status"]) and np.array_equal(one["iters"], two["iters"])
    assert np.array_equal(one["kkt"], two["kkt"])
    assert np.array_equal(r1["u"], r2["u"])


def test_mirror_non_linear_with_tolerance(pkg, mo):
    """proceed_controller(...; mpc_programming_type = "non_linear", mpc_sqp_tolerance = 1e-6): calculate! solves every instance to
    the tolerance and records the verdicts; an iteration limit too small raises unless mpc_allow_unsolved."""
    f = mo.synthetic_fnn(act="tanh")
    sys_ = pkg.ConstrainedBlackBoxControlDiscreteSystem(pkg.Fnn(f.W_in, f.W_h, f.b_h, f.W_out, f.act), 4, 2,
                                                        pkg.Hyperrectangle([-10] * 4, [10] * 4), pkg.Hyperrectangle([-1, -1], [1, 1]))
    x_ref, u_ref = [0.2, -0.1, 0.05, 0.0], [0.1, -0.2]
    N, batch = 20, 16
    C = pkg.proceed_controller(sys_, "model_predictive_control", N, 1, x_ref, u_ref, mpc_batch=batch, mpc_programming_type="non_linear",
                               mpc_sqp_iterations=30, mpc_sqp_tolerance=1e-6)
    P = C.tuning.terminal_ingredient.P
    X0 = np.asarray(x_ref)[None, :] + 0.6 * mo.splitmix_normal(0x5EED0009, 0, batch, 4)
    res = pkg._model_predictive_control_computation(C, X0)
    mod = C.tuning.modeler
    assert np.all(mod.last_sqp_status == 0) and np.all(mod.last_sqp_kkt <= 1e-6) and np.all(mod.last_sqp_iters <= 30)
    xr, ur = np.tile(np.array(x_ref)[:, None], (1, N + 1)), np.tile(np.array(u_ref)[:, None], (1, N))
    for i in range(batch):
        k = mo.nlp_kkt_residual(f, X0[i], res.u[i], xr, ur, 100 * np.eye(4), 0.1 * np.eye(2), np.zeros((2, 2)), P, -np.ones(2), np.ones(2))
        assert k <= 1e-6 + 1e-9
    mod.sqp["iterations"], mod.sqp["tolerance"] = 1, 1e-14   # out of reach in one iteration from the shifted warm start
    with pytest.raises(ArithmeticError):
        pkg._model_predictive_control_computation(C, X0)
    assert np.any(mod.last_sqp_status == 1)
    mod.allow_unsolved = True
    pkg._model_predictive_control_computation(C, X0)
    C.tuning.modeler.solver.close()
    with pytest.raises(ValueError):
        pkg.proceed_controller(sys_, "model_predictive_control", N, 1, x_ref, u_ref, mpc_programming_type="non_linear",
                               mpc_sqp_tolerance=1e-6, mpc_sqp_step=0.5)
