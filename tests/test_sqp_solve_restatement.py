"""CPU checks of the restatement behind almpc_sqp_fnn_solve (tests/sqp_solve_ref.py) and of its fixture on the benchmark batch."""
import json
import os

import numpy as np

import sqp_solve_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _args(kw):
    return kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"]


def test_adjoint_residual_at_zero_defect_is_nlp_kkt_residual(mo):
    f, kw, X0 = ref.bench_setup(b=6, N=30)
    for S in (kw["S"], 0.2 * np.eye(2)):
        k2 = dict(kw, S=S)
        for i in range(6):
            U = np.clip(kw["u_ref"] + 0.3 * mo.splitmix_normal(0x5EED0011, i, 1, 60).reshape(2, 30), -1.0, 1.0)
            X = mo.fnn_rollout(f, X0[i], U)
            r, d, _ = ref.adjoint_residual(f, X, U, *_args(k2))
            assert d <= 1e-15
            k = mo.nlp_kkt_residual(f, X0[i], U, *_args(k2))
            assert abs(r - k) <= 1e-12 * k


def test_without_stopping_it_is_the_oracle_loop(mo):
    """With a tolerance nothing reaches, the restatement is mpc_oracle.sqp_fnn(adaptive=True), decision by decision."""
    f, kw, X0 = ref.bench_setup(b=4, N=20)
    for i in range(4):
        r = ref.sqp_solve(f, X0[i], *_args(kw), 9, 1e-300)
        X, U, _ = mo.sqp_fnn(f, X0[i], *_args(kw), 9, adaptive=True)
        assert r["status"] == 1 and r["iters"] == 9
        assert np.array_equal(r["U"], U) and np.array_equal(r["X"], X)


def test_fixture_of_the_benchmark_batch():
    """Gauss-Newton under the merit rule leaves 6 of the 256 benchmark instances unconverged after 40 iterations (linear
    contraction); the fixture's verdicts are re-derived here for a sample, including one of the six."""
    fx = json.load(open(os.path.join(GOLDEN, "fnn_sqp_solve_gn.json")))
    st, it = np.array(fx["status"]), np.array(fx["iters"])
    assert st.size == 256 and list(np.nonzero(st)[0]) == [42, 50, 69, 115, 226, 235]
    assert np.all(it[st == 1] == 40) and np.all(np.array(fx["kkt"])[st == 0] <= 1e-6)
    assert int(np.median(it[st == 0])) == 9 and it[st == 0].max() == 37
    f, kw, X0 = ref.bench_setup()
    for i in (0, 3, 50):
        r = ref.sqp_solve(f, X0[i], *_args(kw), fx["max_iters"], fx["tol"])
        assert (r["status"], r["iters"]) == (fx["status"][i], fx["iters"][i]), i
        assert abs(r["kkt"] - fx["kkt"][i]) <= 1e-9 * max(1.0, fx["kkt"][i])
