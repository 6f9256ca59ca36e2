"""GPU tests of the rows form of k_sens (csrc/almpc_sens.hip.h: k_sens<.., .., true>, k_sens_rows_table): almpc_sensitivity_rows,
almpc_sensitivity_rows_vjp and their group forms on shared designs with a state box and / or the terminal equality.

Reference per instance: tests/sens_rows_ref.py (the G form in numpy FP64, projected where the handle's Ghat is) fed with H, F, d from
almpc_get_design and the handle's OWN returned u and x under the contract's active-set rules, so both sides differentiate the same
face.  Every case also asserts that no returned state row lies between 1e-9 and 1e-5 of max(1, |bound|) from its bound, so a
misclassified row cannot pass unseen.

Tolerance: ten times the CPU gap of the case (tests/sens_rows_cases.py: gpu_tol = 10 MEASURED_GAP).  On the oracle's solutions the G
form and the projected G form differ from the direct KKT form by 4.6e-13 ... 4.8e-13 on the double integrator, 5.7e-15 ... 8.5e-15 on
the two random models, 3.5e-11 (box) and 3.9e-11 (box and equality) on the quadrotor, worst cond(Ghat_WW) 4.0e7 and 1.4e8
(tests/test_sens_rows_restatement.py prints them and holds later runs to them).  So on the device, of max(1, max|J_i|) and for a VJP
of max(1, max|g_x0_i|): 4.6e-12 ... 4.8e-12, 5.7e-14 ... 8.5e-14, 3.5e-10 and 3.9e-10; the factor of ten is for the device's own G and
Ghat.  Every test prints its worst figure.
"""
import dataclasses
import os

import numpy as np
import pytest

import sens_ref as sr
import sens_rows_cases as sc
import sens_rows_ref as rr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4


def solve(capi, p, X0, opts=None, make=None, refs=None):
    sv = make() if make else capi.Solver(p.n, p.m, p.N, X0.shape[0])
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, xmin=p.x_min, xmax=p.x_max, terminal=p.terminal)
    if refs is None:
        sv.set_reference(p.x_ref, p.u_ref)
    else:
        sv.set_reference(*refs, per_instance=True)
    sv.update_initialization(X0)
    sv.calculate(opts)
    return sv


class Ref:
    """The numpy side of one handle: design operands once, then per instance the active rows and the Jacobians."""

    def __init__(self, sv, p, projected):
        g = sv.get_design()
        self.p, self.H, self.F, self.d = p, g["H"], g["F"], g["d"]
        self.st, self.ix, self.eq = rr.state_rows(p.n, p.N, p.x_min is not None, p.terminal == "equality")
        self.Gam, self.Phi = rr.row_tables(p.A, p.B, p.N, self.st, self.ix)
        self.ops = rr.rows_operands(self.H, self.F, self.d, self.Gam, self.Phi)
        self.projected = projected and self.eq.any()
        if self.projected:
            self.ops = rr.project(*self.ops, p.nz + np.nonzero(self.eq)[0])

    def active(self, u, x):
        p = self.p
        gaps = rr.bound_gaps(x, p.x_min, p.x_max, self.st, self.ix, self.eq)
        bad = (gaps > 1e-9) & (gaps < 1e-5)
        assert not bad.any(), ("a returned state row between 1e-9 and 1e-5 of its bound", gaps[bad])
        return sr.active_rows(u, p.u_min, p.u_max, self.d), rr.active_state_rows(x, p.x_min, p.x_max, self.st, self.ix, self.eq)

    def jac(self, au, ax):
        if self.projected:
            return rr.jac_projected(self.ops, self.d, au, ax, self.eq)
        return rr.jac_gform(self.ops, self.d, au, ax)

    def vjp(self, au, ax, g_u, g_x):
        p = self.p
        if self.projected:
            return rr.vjp_projected(self.ops, self.d, au, ax, self.eq, p.A, p.B, g_u, g_x)
        return rr.vjp_gform(self.ops, self.d, au, ax, p.A, p.B, g_u, g_x)


def check_jacobians(sv, ref, res, sens, tol):
    """K0, dU, dX and rows of every solved instance, rows = -1 and zeros of the others; returns (worst error / scale, the active
    masks (None: not solved))."""
    p = ref.p
    worst, acts = 0.0, []
    for i in range(res["u"].shape[0]):
        if res["status"][i] != 0:
            acts.append(None)
            assert sens["rows"][i] == -1, (i, sens["rows"][i])
            assert not sens["K0"][i].any() and not sens["dU"][i].any() and not sens["dX"][i].any(), i
            continue
        au, ax = ref.active(res["u"][i], res["x"][i])
        acts.append((au, ax))
        J = ref.jac(au, ax)
        dX = sr.dx_from_du(p.A, p.B, J, p.N)
        K0, dU = sr.shaped(J, p.m, p.N)
        sj, sx = max(1.0, np.abs(J).max()), max(1.0, np.abs(dX).max())
        assert sens["rows"][i] == au.sum() + ax.sum(), (i, sens["rows"][i], int(au.sum()), int(ax.sum()))
        for name, got, want, s in (("K0", sens["K0"][i], K0, sj), ("dU", sens["dU"][i], dU, sj), ("dX", sens["dX"][i], dX, sx)):
            err = np.abs(got - want).max() / s
            worst = max(worst, err)
            assert err <= tol, (i, name, err, tol)
        assert np.array_equal(sens["dX"][i][:, 0, :], np.eye(p.n))
        assert not sens["dU"][i].transpose(1, 0, 2).reshape(p.nz, p.n)[au].any(), "input rows of W are exactly zero"
    return worst, acts


def _rows(acts):
    return [int(a[0].sum() + a[1].sum()) for a in acts if a is not None]


def _loss(rng, b, p):
    return rng.normal(size=(b, p.m, p.N)), rng.normal(size=(b, p.n, p.N + 1))


def check_vjp(ref, sens, acts, g_x0, vrows, g_u, g_x, tol):
    worst = 0.0
    for i, a in enumerate(acts):
        if a is None:
            assert vrows[i] == -1 and not g_x0[i].any(), i
            continue
        want = ref.vjp(a[0], a[1], g_u[i], g_x[i])
        own = sr.vjp_from_jacobians(sens["dU"][i], sens["dX"][i], g_u[i], g_x[i])
        for other in (want, own):
            err = np.abs(g_x0[i] - other).max() / sr.vjp_scale(want)
            worst = max(worst, err)
            assert err <= tol, (i, err, tol)
    assert np.array_equal(vrows, sens["rows"])
    return worst


@pytest.mark.parametrize("name", sc.GPU_CASES)
def test_every_case_against_the_restatement(capi, mo, name):
    p, X0 = sc.case(mo, name)
    sv = solve(capi, p, X0)
    res = sv.get_results()
    assert set(np.unique(res["status"])) <= {capi.SOLVED, capi.INFEASIBLE}, np.bincount(res["status"])
    ref = Ref(sv, p, projected=True)
    sens = sv.sensitivity_rows()
    worst, acts = check_jacobians(sv, ref, res, sens, sc.gpu_tol(name))
    wv = 0.0
    if name.startswith(("di", "quad")):
        g_u, g_x = _loss(np.random.default_rng(17), X0.shape[0], p)
        g_x0, vrows = sv.sensitivity_rows_vjp(g_u, g_x)
        wv = check_vjp(ref, sens, acts, g_x0, vrows, g_u, g_x, sc.gpu_tol(name))
        a0, r0 = sv.sensitivity_rows_vjp(g_u, None)
        a1, r1 = sv.sensitivity_rows_vjp(g_u, np.zeros_like(g_x))
        assert a0.tobytes() == a1.tobytes() and np.array_equal(r0, r1) and np.abs(a0).max() > 0
    sv.close()
    rows = _rows(acts)
    nstate = [int((a[1] & ~ref.eq).sum()) for a in acts if a is not None]
    unsolved = sum(a is None for a in acts)
    beyond = sum(r - (p.n if ref.projected else 0) > 32 for r in rows)
    print(f"{name}: {unsolved} of {len(acts)} infeasible; rows {min(rows)} .. {max(rows)}, state-box rows up to {max(nstate)}, "
          f"{beyond} instances in the second tier; worst error / scale: J {worst:.3e}, VJP {wv:.3e} (tolerance {sc.gpu_tol(name):g})")
    if p.x_min is not None:
        assert max(nstate) > 0 and min(nstate) == 0, nstate
    if name == "quad_box":
        assert beyond >= 1 and unsolved >= 1
    if name in ("quad_both", "r637_box", "r637_both"):
        assert unsolved >= 1


def test_projected_and_unprojected_handles_agree(capi, mo):
    """The quadrotor with the box and the terminal equality, once projected (the equality rows never enter S) and once under
    ALMPC_NO_EQ_PROJECTION (they are ordinary members of W): the same rows, the same Jacobians within the tolerance."""
    p, X0 = sc.case(mo, "quad_both")
    tol = sc.gpu_tol("quad_both")
    out = {}
    for switch in (False, True):
        if switch:
            os.environ["ALMPC_NO_EQ_PROJECTION"] = "1"
        try:
            sv = solve(capi, p, X0)   # (a handle's switches are what almpc_create finds)
        finally:
            os.environ.pop("ALMPC_NO_EQ_PROJECTION", None)
        res = sv.get_results()
        ref = Ref(sv, p, projected=not switch)
        sens = sv.sensitivity_rows()
        worst, acts = check_jacobians(sv, ref, res, sens, tol)
        g_u, g_x = _loss(np.random.default_rng(23), X0.shape[0], p)
        g_x0, vrows = sv.sensitivity_rows_vjp(g_u, g_x)
        wv = check_vjp(ref, sens, acts, g_x0, vrows, g_u, g_x, tol)
        sv.close()
        rows = _rows(acts)
        tier2 = sum(r - (p.n if not switch else 0) > 32 for r in rows)
        print(f"{'unprojected' if switch else 'projected'}: rows {min(rows)} .. {max(rows)}, {tier2} instances in the second tier; "
              f"worst error / scale: J {worst:.3e}, VJP {wv:.3e}")
        out[switch] = (res, sens, tier2)
    (ra, sa, ta), (rb, sb, tb) = out[False], out[True]
    assert np.array_equal(ra["status"], rb["status"]) and np.array_equal(sa["rows"], sb["rows"])
    assert tb >= 1 and ta < tb, "unprojected working sets beyond 32 rows, the same instances in the first tier when projected"
    for i in np.nonzero(ra["status"] == 0)[0]:
        for k in ("K0", "dU", "dX"):
            s = max(1.0, np.abs(sa[k][i]).max())
            assert np.abs(sa[k][i] - sb[k][i]).max() <= 2 * tol * s, (i, k)


def test_per_instance_references_and_input_rate_weight(capi, mo):
    p, X0 = sc.case(mo, "di_box")
    b = X0.shape[0]
    rng = np.random.default_rng(3)
    xr = np.zeros((b, 2, 11)); xr[:, 0, :] = rng.normal(size=(b, 1))   # a position set-point per instance (an equilibrium)
    ur = 0.3 * rng.uniform(-1, 1, size=(b, 1, 1)) * np.ones((b, 1, 10))
    sv = solve(capi, p, X0, refs=(xr, ur))
    res = sv.get_results()
    worst, acts = check_jacobians(sv, Ref(sv, p, True), res, sv.sensitivity_rows(), sc.gpu_tol("di_box"))
    sv.close()
    ns = [int(a[1].sum()) for a in acts if a is not None]
    assert len(ns) >= b // 2 and max(ns) > 0 and min(ns) == 0, ns
    # an input-rate weight: S enters H only
    ps = dataclasses.replace(mo.make_problem(p.A, p.B, 10, [-1.0], [1.0], s=0.5), x_min=p.x_min, x_max=p.x_max)
    sv = solve(capi, ps, X0)
    res = sv.get_results()
    assert np.abs(sv.get_design()["H"] - mo.condense(p)[2]).max() > 0.1
    worst_s, acts = check_jacobians(sv, Ref(sv, ps, True), res, sv.sensitivity_rows(), sc.gpu_tol("di_box"))
    sv.close()
    ns = [int(a[1].sum()) for a in acts if a is not None]
    print(f"per-instance references: worst {worst:.3e}; S != 0: worst {worst_s:.3e}")
    assert len(ns) >= b // 2 and max(ns) > 0 and min(ns) == 0, ns


def test_instances_redone_by_the_stagewise_fallback_take_part(capi, mo):
    p, X0 = sc.case(mo, "di_both")
    sv = solve(capi, p, X0, capi.default_opts(polish_max_iter=1))   # (the condensed finish gives up; the lazy redo runs first)
    sens = sv.sensitivity_rows()
    res = sv.get_results()
    assert np.all(res["status"] == 0), np.bincount(res["status"])
    worst, acts = check_jacobians(sv, Ref(sv, p, True), res, sens, sc.gpu_tol("di_both"))
    sv.close()
    print(f"after the redo: rows {min(_rows(acts))} .. {max(_rows(acts))}, worst error / scale {worst:.3e}")


def test_group_equals_one_handle(capi, mo):
    p, X0 = sc.case(mo, "quad_both")
    b = X0.shape[0]
    g_u, g_x = _loss(np.random.default_rng(8), b, p)
    got = []
    for make in (None, lambda: capi.Group(p.n, p.m, p.N, b, devices=[0, 0])):
        s = solve(capi, p, X0, make=make)
        sens = s.sensitivity_rows()
        sens["g_x0"], sens["vrows"] = s.sensitivity_rows_vjp(g_u, g_x)
        got.append(sens)
        s.close()
    assert got[0]["rows"].max() > 0 and got[0]["rows"].min() == -1
    for k in ("K0", "dU", "dX", "g_x0", "rows", "vrows"):
        assert np.ascontiguousarray(got[0][k]).tobytes() == np.ascontiguousarray(got[1][k]).tobytes(), k


def test_table_of_row_values_through_an_instance_with_empty_working_set(capi, mo):
    """T1 = A V + [0; Phi_rows] through its effect (the handle does not hand the table out): where W is empty du/dx0 = diag(d) V and the
    state rows of dX are T1's.  The same instance on the twin design without the box (k_sens's input-box operands dG, V) gives the
    same Jacobians -- the numbers the finish's own s0 table (rows 0 .. n-1) is built from."""
    p, X0 = sc.case(mo, "di_box")
    X0 = 0.01 * X0   # (no input and no state reaches a bound)
    sv = solve(capi, p, X0)
    sens = sv.sensitivity_rows()
    ref = Ref(sv, p, True)
    twin = solve(capi, dataclasses.replace(p, x_min=None, x_max=None), X0)
    plain = twin.sensitivity()
    sv.close(); twin.close()
    assert np.all(sens["rows"] == 0) and np.all(plain["rows"] == 0)
    T1 = ref.ops[1]
    worst = 0.0
    for i in range(X0.shape[0]):
        _, dU = sr.shaped(ref.d[:, None] * T1[:p.nz], p.m, p.N)
        rows_of_dx = np.array([sens["dX"][i][s, k, :] for k, s in zip(ref.st, ref.ix)])
        for got, want in ((sens["dU"][i], dU), (rows_of_dx, T1[p.nz:]), (sens["dU"][i], plain["dU"][i]), (sens["dX"][i], plain["dX"][i])):
            err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
            worst = max(worst, err)
            assert err <= sc.gpu_tol("di_box"), (i, err)
    print(f"T1 through an empty working set: worst error / scale {worst:.3e}")


def test_rows_form_is_the_old_path_bit_for_bit_on_an_input_box_design(capi, mo):
    p = mo.quadrotor(N=30)
    X0 = np.concatenate([mo.quadrotor_x0_batch(16, a, first_instance=16 * i) for i, a in enumerate((3.0, 1.0, 0.3))])
    sv = solve(capi, p, X0)
    g_u, g_x = _loss(np.random.default_rng(4), 48, p)
    for tau in (0.0, 1e-6):
        old = sv.sensitivity(act_tol=tau)
        new = sv.sensitivity_rows(act_tol_u=tau, act_tol_x=3e-3)
        for k in ("K0", "dU", "dX", "rows"):
            assert np.ascontiguousarray(old[k]).tobytes() == np.ascontiguousarray(new[k]).tobytes(), k
        for gx in (g_x, None):
            (a0, r0), (a1, r1) = sv.sensitivity_vjp(g_u, gx, act_tol=tau), sv.sensitivity_rows_vjp(g_u, gx, act_tol_u=tau, act_tol_x=3e-3)
            assert a0.tobytes() == a1.tobytes() and np.array_equal(r0, r1)
    assert old["rows"].max() > 0 and np.abs(old["dU"]).max() > 0
    sv.close()


def test_controller_takes_the_rows_form_with_state_rows(pkg, capi, mo):
    p, X0 = sc.case(mo, "di_box")
    X, U = pkg.Hyperrectangle(list(p.x_min), list(p.x_max)), pkg.Hyperrectangle(p.u_min, p.u_max)
    sys_ = pkg.ConstrainedLinearControlDiscreteSystem(p.A, p.B, X, U)
    b = 8
    C = pkg.proceed_controller(sys_, "model_predictive_control", 10, 1, [0.0, 0.0], [0.0], mpc_batch=b, mpc_state_constraint=True)
    pkg._model_predictive_control_computation(C, X0[:b])
    got = pkg.sensitivity(C, ("K0", "dU", "dX"))
    sv = C.tuning.modeler.solver
    res = sv.get_results()
    worst, acts = check_jacobians(sv, Ref(sv, p, True), res, got, sc.gpu_tol("di_box"))
    with pytest.raises(capi.AlmpcError):   # (the old call still refuses such a design)
        sv.sensitivity(("K0",))
    sv.close()
    assert max(int(a[1].sum()) for a in acts) > 0


def _refused(capi, sv, code=ERR_UNSUPPORTED):
    for call in (lambda: sv.sensitivity_rows(("K0",)), lambda: sv.sensitivity_rows_vjp(np.zeros((sv.batch, sv.m, sv.N)))):
        with pytest.raises(capi.AlmpcError) as e:
            call()
        assert e.value.code == code, e.value
        assert (sv.L.almpc_last_error(sv.h) or b"").decode().strip()


def test_refusals_that_remain(capi, mo):
    p, X0 = sc.case(mo, "di_both")
    X0 = 0.1 * X0[:4]
    kw = dict(xmin=p.x_min, xmax=p.x_max, terminal="equality")
    # before any step, a bad mask, nothing computed yet, a new design
    sv = capi.Solver(2, 1, 10, 4)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, **kw)
    _refused(capi, sv, ERR_INVALID)
    sv.update_initialization(X0); sv.calculate()
    assert sv.L.almpc_sensitivity_rows(sv.h, 0, 0.0, 0.0) == ERR_INVALID and sv.L.almpc_sensitivity_rows(sv.h, 8, 0.0, 0.0) == ERR_INVALID
    assert sv.L.almpc_get_sensitivity(sv.h, None, None, None, None) == ERR_INVALID
    assert sv.sensitivity_rows(("K0",))["rows"].min() >= 2
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, **kw)
    _refused(capi, sv, ERR_INVALID)
    sv.close()
    # per-instance models with state rows
    sv = capi.Solver(2, 1, 10, 4)
    sv.design_batched(np.tile(p.A, (4, 1, 1)), np.tile(p.B, (4, 1, 1)), p.Q, p.R, None, None, p.u_min, p.u_max, **kw)
    sv.update_initialization(X0); sv.calculate()
    _refused(capi, sv)
    assert "per-instance" in sv.L.almpc_last_error(sv.h).decode()
    sv.close()
    # structured handle
    sv = capi.Solver(2, 1, 10, 4, structured=True)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, **kw)
    sv.update_initialization(X0); sv.calculate()
    _refused(capi, sv)
    sv.close()
    # time-varying design
    sv = capi.Solver(2, 1, 10, 4)
    A_all, B_all = np.tile(p.A, (4, 10, 1, 1)), np.tile(p.B, (4, 10, 1, 1))
    xbar = np.zeros((4, 2, 11)); xbar[:, :, 0] = X0
    for k in range(10):
        xbar[:, :, k + 1] = xbar[:, :, k] @ p.A.T
    sv.design_ltv(A_all, B_all, None, xbar, np.zeros((4, 1, 10)), None, None, p.Q, p.R, None, p.P, p.u_min, p.u_max)
    _refused(capi, sv)
    sv.close()
    # the SQP loop and the re-linearisation pipeline of a black-box model
    f = mo.synthetic_fnn()
    n, m, N = 4, 2, 10
    x_ref, u_ref = np.zeros((n, N + 1)), np.zeros((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    Al, Bl = capi.fnn_linearize(f.W_in, f.W_h, f.b_h, f.W_out, x_ref[:, -1][None], u_ref[:, -1][None], act=f.act)
    P = capi.dare(Al[0], Bl[0], Q, R)
    x0 = 0.05 * np.random.default_rng(2).normal(size=(4, n))
    sv = capi.Solver(n, m, N, 4)
    sv.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act)
    sv.update_initialization(x0)
    sv.relin_fnn_step()
    _refused(capi, sv)
    sv.close()
    sv = capi.Solver(n, m, N, 4)
    sv.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act)
    sv.sqp_fnn_start(x0)
    sv.sqp_fnn_iterate(1)
    _refused(capi, sv)
    sv.close()
