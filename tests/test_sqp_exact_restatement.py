"""CPU checks of the exact-Hessian restatement (tests/sqp_exact_ref.py) and of its fixture on the benchmark batch."""
import json
import os

import numpy as np
import pytest

import sqp_exact_ref as ex
import sqp_solve_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("act", ["tanh", "sigmoid", "swish", "identity"])
def test_stage_hessian_is_the_derivative_of_the_jacobian_transpose(mo, act):
    """W = d/dz [A' lam; B' lam] by central differences (relative 1e-7)."""
    f = mo.synthetic_fnn(act=act)
    for s in range(3):
        z = 0.5 * mo.splitmix_normal(0x5EED0021, s, 1, 6)[0]
        lam = mo.splitmix_normal(0x5EED0022, s, 1, 4)[0]
        W = ex.stage_hessian(f, z[:4], z[4:], lam)
        assert np.array_equal(W, W.T)

        def grad(zz):
            A, B = f.jacobian(zz[:4], zz[4:])
            return np.concatenate([A.T @ lam, B.T @ lam])
        D = np.zeros((6, 6))
        for j in range(6):
            e = np.zeros(6)
            e[j] = 1e-5
            D[:, j] = (grad(z + e) - grad(z - e)) / 2e-5
        if act == "identity":
            assert np.abs(W).max() == 0.0 and np.abs(D).max() <= 1e-9
        else:
            assert np.abs(W - D).max() <= 1e-7 * np.abs(D).max()


def test_exact_qp_is_the_second_order_model(mo):
    """H_ex (without the shift) is the Hessian of the condensed Lagrangian: the QP objective's curvature along v equals the second
    difference of J + lam'(f - x+) along the linearised trajectory, to rounding."""
    f, kw, X0 = ref.bench_setup(b=2, N=12)
    U = np.clip(kw["u_ref"], -1.0, 1.0)
    X = mo.fnn_rollout(f, X0[1], U)
    A, B, c = [], [], []
    for k in range(12):
        Ak, Bk = f.jacobian(X[:, k], U[:, k])
        A.append(Ak); B.append(Bk); c.append(f.forward(X[:, k], U[:, k]) - X[:, k + 1])
    He, qe, lo, hi, H, q, delta = ex.exact_qp(f, X, U, A, B, c, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"],
                                              kw["u_min"], kw["u_max"])
    act = ((U <= -1.0) | (U >= 1.0)).T.reshape(-1)
    Hx = He - np.diag(delta * act)
    # zero defects: the condensed problem is the single-shooting NLP, whose Hessian in U is Hx (central second differences)
    def J(Uf):
        return mo.nlp_cost_and_gradient(f, X0[1], Uf.reshape(12, 2).T, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"])[0]
    u0 = U.T.reshape(-1)
    h = 1e-4
    for a, b_ in ((0, 0), (3, 7), (10, 11), (23, 5)):
        ea, eb = np.zeros(24), np.zeros(24)
        ea[a] = h; eb[b_] = h
        d2 = (J(u0 + ea + eb) - J(u0 + ea - eb) - J(u0 - ea + eb) + J(u0 - ea - eb)) / (4 * h * h)
        assert abs(d2 - Hx[a, b_]) <= 1e-5 * np.abs(Hx).max(), (a, b_, d2, Hx[a, b_])


def test_exact_fixture_of_the_benchmark_batch():
    """Exact Hessian, cold start, at most 30 iterations: 255 of the 256 benchmark instances converge (Gauss-Newton leaves 6 after 40),
    instance 69 needs more.  Re-derived here for a sample."""
    fx = json.load(open(os.path.join(GOLDEN, "fnn_sqp_solve_exact.json")))
    st, it = np.array(fx["status"]), np.array(fx["iters"])
    assert list(np.nonzero(st)[0]) == [69]
    assert int(np.median(it)) == 4 and it[st == 0].max() <= 20
    f, kw, X0 = ref.bench_setup()
    for i in (0, 42):
        r = ex.sqp_solve_exact(f, X0[i], kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"],
                               fx["max_iters"], fx["tol"])
        assert (r["status"], r["iters"], r["gn_fallbacks"]) == (fx["status"][i], fx["iters"][i], fx["gn_fallbacks"][i]), i
