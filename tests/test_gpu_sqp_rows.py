"""GPU tests of the state-row multipliers of the Fnn SQP loop (almpc_sqp_fnn_set_row_multipliers), through the C ABI: the finishes hand
the multipliers of every iteration's QP out, the stopping test of almpc_sqp_fnn_solve and the exact Hessian take them into the adjoint.
Checked against the restatement tests/sqp_rows_ref.py and its method-independent certificate.  The state-box batch is the one of
tests/test_gpu_sqp.py::test_sqp_with_state_box (sqp_rows_ref.state_box_fixture): 24 instances, Fnn 4-2-16x2 tanh, N 20; instances 9, 18
and 19 have an infeasible first QP."""
import numpy as np
import pytest

import sqp_rows_ref as rr

pytestmark = pytest.mark.gpu
TOL = 1e-6
INFEASIBLE = [9, 18, 19]


def _args(kw):
    return (kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"])


def _box_solver(capi, rows=True, b=24, make=None):
    f, kw, xlo, xhi, X0 = rr.state_box_fixture(b=b)
    s = capi.Solver(4, 2, 20, b) if make is None else make(4, 2, 20, b)
    s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"],
                    act="tanh", xmin=xlo, xmax=xhi)
    if rows:
        s.sqp_fnn_set_row_multipliers(True)
    return s, f, kw, xlo, xhi, X0


def _iterate(capi, s, iters, **k):
    """sqp_fnn_iterate on a batch with infeasible instances: the call names them with ALMPC_ERR_NUMERIC after finishing the others"""
    with pytest.raises(capi.AlmpcError) as ei:
        s.sqp_fnn_iterate(iters, **k)
    assert ei.value.code == -6 and "infeasible" in str(ei.value)


@pytest.mark.parametrize("hessian", ["gauss_newton", "exact"])
def test_first_qp_multipliers_are_the_restatements(capi, mo, hessian):
    """One iteration from the start.  Gauss-Newton: the QP is decided by k_polish_gen / k_polish_gen64 and its multipliers are the
    restatement's to 1e-9 of max |mu| (both solve one QP exactly).  Exact mode: the shifted exact Hessian of the first iteration is
    indefinite for every instance of this batch (the restatement counts the fallback), so the SAME Gauss-Newton QP is decided by
    k_sdual behind k_sgains -- this pins the convention of its multipliers (the 0.5 in its sources).  Its bound: k_sdual accepts a
    working set whose rows sit on their bounds to 1e-8 of the row's width (its confirmation test) and the multipliers follow through
    (G_WW)^-1; two digits are left for its conditioning: 1e-6 of max |mu|.  A factor 2 or a sign would be 1e6 times that."""
    s, f, kw, xlo, xhi, X0 = _box_solver(capi)
    s.sqp_fnn_set_hessian(hessian)
    s.sqp_fnn_start(X0)
    assert np.all(s.sqp_fnn_state_multipliers() == 0.0)   # before the first QP
    _iterate(capi, s, 1)
    mu = s.sqp_fnn_state_multipliers()
    skipped = list(np.flatnonzero(s.sqp_fnn_skipped()))
    s.close()
    assert mu.shape == (24, 4, 20)
    assert skipped == INFEASIBLE
    bound = 1e-9 if hessian == "gauss_newton" else 1e-6
    worst = 0.0
    for i in range(24):
        r = rr.sqp_solve_rows(f, X0[i], *_args(kw), xlo, xhi, "none", 1, TOL, adaptive=False, exact=hessian == "exact")
        if i in INFEASIBLE:
            assert r["status"] == 3 and np.all(mu[i] == 0.0)
            continue
        assert r["status"] == 1 and r["iters"] == 1
        if hessian == "exact":
            assert r["gn_fallbacks"] == 1
        assert np.count_nonzero(r["mu"]) > 0
        err = np.abs(mu[i] - r["mu"]).max() / np.abs(r["mu"]).max()
        worst = max(worst, err)
        print(f"first QP {hessian} instance {i}: max|mu| {np.abs(r['mu']).max():.3e} rel err {err:.2e} rows {np.count_nonzero(r['mu'])}")
        assert err <= bound, (i, err)
        assert np.array_equal(mu[i] != 0.0, r["mu"] != 0.0), i
    print(f"first QP {hessian}: worst relative error {worst:.2e}")


def _check_solve(mo, f, kw, xlo, xhi, X0, out, res, mu, ref, good):
    for i in good:
        assert out["kkt"][i] <= TOL, (i, out["kkt"][i])
        assert abs(int(out["iters"][i]) - ref[i]["iters"]) <= 1, (i, out["iters"][i], ref[i]["iters"])
        U, X = res["u"][i], res["x"][i]
        cert, _ = rr.nlp_rows_certificate(f, X0[i], U, *_args(kw), xlo, xhi)
        print(f"instance {i}: iters {out['iters'][i]} (restatement {ref[i]['iters']}) kkt {out['kkt'][i]:.2e} certificate {cert:.2e}")
        assert cert <= TOL + 1e-9, (i, cert)
        assert np.abs(X - mo.fnn_rollout(f, X0[i], U)).max() <= 1e-9, i
        assert np.all(X <= xhi[:, None] + 1e-9) and np.all(X >= xlo[:, None] - 1e-9), i
        nact = int(((X[:, 1:] >= xhi[:, None] - 1e-6) | (X[:, 1:] <= xlo[:, None] + 1e-6)).sum())
        assert nact >= 17, (i, nact)
        assert np.all(mu[i][(X[:, 1:] < xhi[:, None] - 1e-6) & (X[:, 1:] > xlo[:, None] + 1e-6)] == 0.0), i


def test_gauss_newton_solve_converges_with_state_rows(capi, mo):
    """solve(40, 1e-6) on the state-box batch: status 3 for exactly 9, 18, 19 and status 0 for the other 21 (the restatement needs at most
    34 iterations), counts within one of the restatement's, kkt <= tol, the certificate of the returned inputs, the trajectory the
    network's own rollout inside the box with at least 17 active rows.  With the switch off -- the behaviour before this feature -- the
    same call leaves all 21 at status 1 with a residual above 1."""
    s, f, kw, xlo, xhi, X0 = _box_solver(capi)
    s.sqp_fnn_start(X0)
    out = s.sqp_fnn_solve(40, TOL)
    res = s.get_results(want=("u", "x"))
    mu = s.sqp_fnn_state_multipliers()
    s.close()
    good = [i for i in range(24) if i not in INFEASIBLE]
    print("status", out["status"].tolist(), "iters", out["iters"].tolist())
    assert list(np.flatnonzero(out["status"] == 3)) == INFEASIBLE
    assert np.all(out["status"][good] == 0), out["status"]
    ref = {i: rr.sqp_solve_rows(f, X0[i], *_args(kw), xlo, xhi, "none", 40, TOL) for i in good}
    assert all(r["status"] == 0 for r in ref.values()) and max(r["iters"] for r in ref.values()) <= 34
    _check_solve(mo, f, kw, xlo, xhi, X0, out, res, mu, ref, good)
    s, *_ = _box_solver(capi, rows=False)
    s.sqp_fnn_start(X0)
    off = s.sqp_fnn_solve(40, TOL)
    assert np.all(s.sqp_fnn_state_multipliers() == 0.0)
    s.close()
    print("switch off: status", off["status"].tolist(), "kkt", np.round(off["kkt"], 3).tolist())
    assert list(np.flatnonzero(off["status"] == 3)) == INFEASIBLE
    assert np.all(off["status"][good] == 1) and np.all(off["kkt"][good] > 1.0)


def test_exact_solve_converges_with_state_rows(capi, mo):
    """set_hessian("exact") with the switch on, solve(12, 1e-6): all 21 converge (the restatement: 5 - 6 iterations), counts within one,
    the certificate as under Gauss-Newton, and strictly fewer iterations at the maximum than the Gauss-Newton run."""
    s, f, kw, xlo, xhi, X0 = _box_solver(capi)
    s.sqp_fnn_set_hessian("exact")
    s.sqp_fnn_start(X0)
    out = s.sqp_fnn_solve(12, TOL)
    res = s.get_results(want=("u", "x"))
    mu = s.sqp_fnn_state_multipliers()
    s.sqp_fnn_set_hessian("gauss_newton")
    s.sqp_fnn_start(X0)
    gn = s.sqp_fnn_solve(40, TOL)
    s.close()
    good = [i for i in range(24) if i not in INFEASIBLE]
    print("status", out["status"].tolist(), "iters", out["iters"].tolist(), "gauss-newton iters", gn["iters"].tolist())
    assert list(np.flatnonzero(out["status"] == 3)) == INFEASIBLE
    assert np.all(out["status"][good] == 0), out["status"]
    ref = {i: rr.sqp_solve_rows(f, X0[i], *_args(kw), xlo, xhi, "none", 12, TOL, exact=True) for i in good}
    assert all(r["status"] == 0 and r["iters"] <= 6 for r in ref.values())
    _check_solve(mo, f, kw, xlo, xhi, X0, out, res, mu, ref, good)
    assert np.all(gn["status"][good] == 0)
    assert out["iters"][good].max() < gn["iters"][good].max()


@pytest.mark.parametrize("hessian", ["gauss_newton", "exact"])
def test_terminal_equality_multipliers(capi, mo, hessian):
    """Terminal equality at the network's equilibrium, N 8, 16 instances, no box: all converge in both modes, x_{N+1} = x_ref to 1e-9, and
    the multipliers of the equality rows (up to 1.3) are the restatement's.  Their bound: the two loops stop at iterates that both pass
    tol = 1e-6 but need not be the same iterate (counts within one); existing tests hold device and restatement inputs to 1e-5 there,
    and the multiplier is -(2 P e_N + ...) with 2 |P| = 300 per unit of state: 5e-3 absolute.  Everything off the equality rows is 0."""
    f, kw, X0 = rr.terminal_equality_fixture()
    b, N = 16, 8
    s = capi.Solver(4, 2, N, b)
    s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"],
                    act="tanh", terminal="equality")
    s.sqp_fnn_set_row_multipliers(True)
    s.sqp_fnn_set_hessian(hessian)
    s.sqp_fnn_start(X0)
    out = s.sqp_fnn_solve(15, TOL)
    res = s.get_results(want=("u", "x"))
    mu = s.sqp_fnn_state_multipliers()
    s.close()
    print("status", out["status"].tolist(), "iters", out["iters"].tolist(), "kkt", out["kkt"].tolist())
    assert np.all(out["status"] == 0) and np.all(out["kkt"] <= TOL)
    big = 0.0
    for i in range(b):
        r = rr.sqp_solve_rows(f, X0[i], *_args(kw), None, None, "equality", 15, TOL, exact=hessian == "exact")
        assert r["status"] == 0 and r["iters"] <= (4 if hessian == "exact" else 10)
        assert abs(int(out["iters"][i]) - r["iters"]) <= 1, (i, out["iters"][i], r["iters"])
        assert np.abs(res["x"][i][:, -1] - kw["x_ref"][:, -1]).max() <= 1e-9, i
        assert np.abs(res["x"][i] - mo.fnn_rollout(f, X0[i], res["u"][i])).max() <= 1e-9, i
        assert np.all(mu[i][:, :-1] == 0.0)
        err = np.abs(mu[i][:, -1] - r["mu"][:, -1]).max()
        print(f"instance {i}: iters {out['iters'][i]} ({r['iters']}) mu_N {mu[i][:, -1]} restatement {r['mu'][:, -1]} plain residual {r['kkt_plain']:.1e}")
        assert err <= 5e-3, (i, err)
        big = max(big, np.abs(mu[i][:, -1]).max())
        cert, _ = rr.nlp_rows_certificate(f, X0[i], res["u"][i], *_args(kw), None, None, "equality")
        assert cert <= TOL + 1e-9, (i, cert)
    assert big > 0.1   # the multipliers are not a rounding-level quantity on this input


def test_frozen_instances_and_the_switch_off(capi, mo):
    """Converged instances are bit-identical after 20 and 25 iterations, multipliers included; under Gauss-Newton iterate(25) gives
    bit-identical x, u and skipped flags with the switch on and off; with it off set_hessian("exact") on a state-row handle is refused."""
    runs = []
    for iters in (20, 25):
        s, f, kw, xlo, xhi, X0 = _box_solver(capi)
        s.sqp_fnn_start(X0)
        out = s.sqp_fnn_solve(iters, TOL)
        runs.append((out, s.get_results(want=("u", "x")), s.sqp_fnn_state_multipliers()))
        s.close()
    (o1, r1, m1), (o2, r2, m2) = runs
    conv = np.flatnonzero(o1["status"] == 0)
    assert len(conv) >= 20 and np.all(o2["status"][conv] == 0)
    assert np.array_equal(o1["iters"][conv], o2["iters"][conv]) and np.array_equal(o1["kkt"][conv], o2["kkt"][conv])
    assert np.array_equal(r1["u"][conv], r2["u"][conv]) and np.array_equal(r1["x"][conv], r2["x"][conv])
    assert np.array_equal(m1[conv], m2[conv]) and np.all(np.abs(m1[conv]).max(axis=(1, 2)) > 0.0)
    pair = []
    for rows in (True, False):
        s, f, kw, xlo, xhi, X0 = _box_solver(capi, rows=rows)
        s.sqp_fnn_start(X0)
        _iterate(capi, s, 25)
        pair.append((s.get_results(want=("u", "x")), s.sqp_fnn_skipped(), s.sqp_fnn_state_multipliers()))
        if not rows:
            with pytest.raises(capi.AlmpcError) as ei:
                s.sqp_fnn_set_hessian("exact")
            assert ei.value.code == -4
        s.close()
    (ra, ka, ma), (rb, kb, mb) = pair
    assert np.array_equal(ra["u"], rb["u"]) and np.array_equal(ra["x"], rb["x"]) and np.array_equal(ka, kb)
    assert np.all(mb == 0.0) and np.abs(ma).max() > 0.0
    # a handle without state rows: the switch is accepted and changes nothing
    f, kw, X0 = rr.terminal_equality_fixture()
    s = capi.Solver(4, 2, 8, 16)
    s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"], act="tanh")
    s.sqp_fnn_set_row_multipliers(True)
    s.sqp_fnn_start(X0)
    a = s.sqp_fnn_solve(15, TOL)
    ua = s.get_results(want=("u",))["u"]
    assert np.all(s.sqp_fnn_state_multipliers() == 0.0)
    s.sqp_fnn_set_row_multipliers(False)
    s.sqp_fnn_start(X0)
    c = s.sqp_fnn_solve(15, TOL)
    assert np.array_equal(a["status"], c["status"]) and np.array_equal(a["kkt"], c["kkt"]) and np.array_equal(ua, s.get_results(want=("u",))["u"])
    s.close()
    # the stage-wise QP route with state rows does not hand the multipliers out: refused while the switch is on
    f, kw, xlo, xhi, X0 = rr.state_box_fixture()
    s = capi.Solver(4, 2, 20, 24)
    s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"],
                    act="tanh", xmin=xlo, xmax=xhi, qp_solver="structured")
    s.sqp_fnn_set_row_multipliers(True)
    s.sqp_fnn_start(X0)
    with pytest.raises(capi.AlmpcError) as ei:
        s.sqp_fnn_solve(5, TOL)
    assert ei.value.code == -4 and "stage-wise" in str(ei.value)
    s.close()


def test_group_of_two_equals_one_handle(capi, mo):
    s, f, kw, xlo, xhi, X0 = _box_solver(capi)
    s.sqp_fnn_set_hessian("exact")
    s.sqp_fnn_start(X0)
    one = s.sqp_fnn_solve(12, TOL)
    u1, m1 = s.get_results(want=("u",))["u"], s.sqp_fnn_state_multipliers()
    s.close()
    g, *_ = _box_solver(capi, make=lambda n, m, N, b: capi.Group(n, m, N, b, devices=[0, 0]))
    g.sqp_fnn_set_hessian("exact")
    g.sqp_fnn_start(X0)
    two = g.sqp_fnn_solve(12, TOL)
    u2, m2 = g.get_results()["u"], g.sqp_fnn_state_multipliers()
    g.close()
    for k in ("status", "iters", "kkt"):
        assert np.array_equal(one[k], two[k]), k
    assert np.array_equal(u1, u2) and np.array_equal(m1, m2)


def test_mirror_state_constraint_with_tolerance_and_exact_hessian(pkg, mo):
    """proceed_controller(..., "non_linear", mpc_state_constraint, mpc_sqp_tolerance, mpc_sqp_hessian = "exact"): the combination a
    reference user lands on.  The multipliers are switched on by the controller; a feasible sub-batch is solved and they are kept."""
    f, kw, xlo, xhi, X0 = rr.state_box_fixture()
    X0 = X0[[i for i in range(24) if i not in INFEASIBLE][:12]]
    n, m, N, batch = 4, 2, 20, 12
    sys_ = pkg.ConstrainedBlackBoxControlDiscreteSystem(pkg.Fnn(f.W_in, f.W_h, f.b_h, f.W_out, f.act), n, m,
                                                        pkg.Hyperrectangle(xlo, xhi), pkg.Hyperrectangle([-1, -1], [1, 1]))
    x_ref, u_ref = [0.2, -0.1, 0.05, 0.0], [0.1, -0.2]
    C = pkg.proceed_controller(sys_, "model_predictive_control", N, 1, x_ref, u_ref, mpc_batch=batch, mpc_programming_type="non_linear",
                               mpc_state_constraint=True, mpc_sqp_tolerance=TOL, mpc_sqp_hessian="exact", mpc_sqp_iterations=12)
    res = pkg._model_predictive_control_computation(C, X0)
    mod = C.tuning.modeler
    P = C.tuning.terminal_ingredient.P
    assert np.all(mod.last_sqp_status == 0) and np.all(mod.last_sqp_kkt <= TOL)
    mu = mod.last_sqp_state_multipliers
    assert mu.shape == (batch, n, N) and np.all(np.count_nonzero(mu.reshape(batch, -1), axis=1) >= 17)
    args = (kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], P, kw["u_min"], kw["u_max"])
    for i in range(batch):
        cert, _ = rr.nlp_rows_certificate(f, X0[i], res.u[i], *args, xlo, xhi)
        assert cert <= TOL + 1e-9, (i, cert)
    mod.solver.close()
