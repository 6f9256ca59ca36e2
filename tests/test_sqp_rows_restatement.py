"""CPU tests of tests/sqp_rows_ref.py, the restatement of the Fnn SQP loop with state-row multipliers in its stopping test and exact
Hessian (almpc_sqp_fnn_set_row_multipliers): it reduces to the plain test without rows, converges where the plain test cannot, and
agrees with a certificate that knows nothing of the method."""
import numpy as np
import pytest

import sqp_rows_ref as rr
import sqp_solve_ref as sref

TOL = 1e-6


def test_no_rows_and_zero_multipliers_is_the_plain_residual_bit_for_bit(mo):
    f, kw, X0 = sref.bench_setup(b=3, N=12)
    n, m, N = 4, 2, 12
    rng = np.random.default_rng(5)
    for i in range(3):
        U = np.clip(kw["u_ref"] + 0.4 * rng.standard_normal((m, N)), -1.0, 1.0)
        X = mo.fnn_rollout(f, X0[i], U) + 1e-3 * rng.standard_normal((n, N + 1))
        a = sref.adjoint_residual(f, X, U, **kw)
        b = rr.adjoint_residual_rows(f, X, U, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"],
                                     np.zeros((n, N)))
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
        assert b[3] == (a[0], 0.0, 0.0)


@pytest.mark.parametrize("exact", [False, True], ids=["gauss_newton", "exact"])
def test_state_box_instances_converge_with_the_row_multipliers(mo, exact):
    """Instances 0, 5, 16 of the state-box fixture: the loop converges, the certificate agrees, and the test WITHOUT the row multipliers
    reads more than 1 at the very same iterates -- the sentence the feature exists for."""
    f, kw, xlo, xhi, X0 = rr.state_box_fixture()
    args = (kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"])
    limit = {False: {0: 15, 5: 15, 16: 34}, True: {0: 5, 5: 6, 16: 5}}[exact]
    for i in (0, 5, 16):
        r = rr.sqp_solve_rows(f, X0[i], *args, xlo, xhi, "none", 40, TOL, adaptive=True, exact=exact)
        assert r["status"] == 0 and r["kkt"] <= TOL, (i, r["status"], r["kkt"])
        assert r["iters"] <= limit[i], (i, r["iters"])
        assert r["kkt_plain"] > 1.0, (i, r["kkt_plain"])
        cert, nmult = rr.nlp_rows_certificate(f, X0[i], r["U"], *args, xlo, xhi)
        assert cert <= TOL + 1e-9, (i, cert)
        # signs, and nothing off the bounds
        Xs, mu = r["X"][:, 1:], r["mu"]
        assert np.count_nonzero(mu) >= 17
        assert np.all(np.abs(Xs - xhi[:, None])[mu > 0] <= TOL) and np.all(np.abs(Xs - xlo[:, None])[mu < 0] <= TOL)
        off = (Xs < xhi[:, None] - 1e-6) & (Xs > xlo[:, None] + 1e-6)
        assert np.all(mu[off] == 0.0)
        if exact:
            assert r["gn_fallbacks"] >= 2   # the first iterations' shifted exact Hessian is indefinite


def test_infeasible_first_qp_is_status_3(mo):
    f, kw, xlo, xhi, X0 = rr.state_box_fixture()
    args = (kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"])
    for i in (9, 18, 19):
        r = rr.sqp_solve_rows(f, X0[i], *args, xlo, xhi, "none", 3, TOL)
        assert r["status"] == 3 and np.all(r["mu"] == 0.0)


def test_terminal_equality_multipliers(mo):
    """Terminal equality at the network's equilibrium, N 8: converges in both modes with |mu_N| of order one, where the plain residual
    stays at 1e-3 or more."""
    f, kw, X0 = rr.terminal_equality_fixture()
    assert np.abs(kw["x_ref"][:, 0] - np.array([-0.29799659, -0.39539931, -0.18897132, -0.02852847])).max() <= 1e-8
    # (an equilibrium far below the 1e-9 the equality is checked to: otherwise the equality is infeasible and the input useless)
    assert np.abs(f.forward(kw["x_ref"][:, 0], kw["u_ref"][:, 0]) - kw["x_ref"][:, 0]).max() <= 1e-12
    args = (kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"])
    for i in (0, 3, 7):
        for exact in (False, True):
            r = rr.sqp_solve_rows(f, X0[i], *args, None, None, "equality", 15, TOL, exact=exact)
            assert r["status"] == 0 and r["iters"] <= (4 if exact else 10), (i, exact, r["status"], r["iters"])
            assert np.abs(r["X"][:, -1] - kw["x_ref"][:, -1]).max() <= 1e-9
            assert np.all(r["mu"][:, :-1] == 0.0) and np.abs(r["mu"][:, -1]).max() > 1e-3
            assert r["kkt_plain"] > 1e-3
            cert, _ = rr.nlp_rows_certificate(f, X0[i], r["U"], *args, None, None, "equality")
            assert cert <= TOL + 1e-9
