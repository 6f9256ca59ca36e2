"""The black-box (NLP) family beyond the 4-2-16x2 model: the cases of tests/nlp_shape_cases.py against the references.  Run on an
MI355X: pytest -m gpu.

The switches (ALMPC_*) are read by almpc_create, and by almpc_fnn_linearize / almpc_densenet_linearize at every call: they are set before
the handle is made or the call goes out.  Tolerances are the project's: max(1e-12, 16 x the restatement's own gap to long double) on A, B
and f (test_linearize_every_kind_and_activation), 1e-11 max|H| and 1e-11 max(1, |q|) on the time-varying design and U_TOL on its solution
(tests/test_gpu_ltv.py), U_TOL and 1e-5 on the SQP iterates and rtol 1e-4 on its histories
(test_sqp_histories_match_the_restatement_per_iteration), 1e-10 on the exact mode's first QP
(test_sqp_exact_first_qp_matches_the_restatement), 1e-9 / 1e-6 / 1e-12 on the re-linearisation pipeline (test_relin_pipeline), and bit
for bit where the kernels promise the same arithmetic in the same order.

Lines that start with `nlp-shapes` print the measured maxima (pytest -s)."""
import functools
import subprocess
import sys

import numpy as np
import pytest

import nlp_shape_cases as nc
import sqp_solve_ref as sref

pytestmark = pytest.mark.gpu

U_TOL = 1e-5
X_TOL = 1e-5
GUARD = 0x7FF8DEADBEEF0123          # a NaN bit pattern no kernel produces
_ids = lambda c: c.id


def _note(what, key, value, bound=None):
    print("nlp-shapes %s %s %.3e%s" % (what, key, value, "" if bound is None else " of %.1e" % bound))


@functools.lru_cache(maxsize=None)
def _num_cus():
    """the device's compute units as torch.cuda.get_device_properties reports them, asked once and in a child process: torch brings a
    HIP runtime of its own, and loaded into this process it and the library's see no device.  Where the child fails: the MI355X's
    256, which the sibling tables assume."""
    code = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    try:
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
        return int(out.stdout.strip().splitlines()[-1])
    except (OSError, subprocess.SubprocessError, ValueError, IndexError):
        return nc.NUM_CUS


# ---------------------------------------------------------------------------- linearisation
def _guarded(records, size):
    """(the float64 buffer of records + 1 records handed to the C call, its words): every word the guard pattern"""
    words = np.full((records + 1) * size, GUARD, dtype=np.uint64)
    return words.view(np.float64), words


def _linearize(capi, c, x, u, env, monkeypatch):
    """A (p, n, n), B (p, n, m), f (p, n) of the C call under the switches `env`, with one record of A, B and f beyond the end that must
    come back untouched"""
    f, lib = nc.model(c), capi.load()
    n, m, p = c.n, c.m, x.shape[0]
    if c.kind == "densenet":
        H, nl, W_in, Wh, bh, W_out = capi._pack_densenet(f.W_in, f.W_h, f.b_h, f.W_out, n, m)
        fn, code = lib.almpc_densenet_linearize, capi._densenet_act(c.act)
    else:
        W_in, W_out = np.asfortranarray(f.W_in), np.asfortranarray(f.W_out)
        H, nl = W_in.shape[0], len(f.W_h)
        Wh = np.ascontiguousarray(np.stack([np.asfortranarray(W).T for W in f.W_h])) if nl else np.zeros((1, 1, 1))
        bh = np.ascontiguousarray(np.stack(f.b_h)) if nl else np.zeros((1, 1))
        fn, code = lib.almpc_fnn_linearize, capi.net_code(c.kind, c.act)
    x, u = np.ascontiguousarray(x), np.ascontiguousarray(u)
    (A, Aw), (B, Bw), (fv, fw) = _guarded(p, n * n), _guarded(p, n * m), _guarded(p, n)
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        rc = fn(0, n, m, H, nl, code, capi._ptr(W_in), capi._ptr(Wh), capi._ptr(bh), capi._ptr(W_out), p, capi._ptr(x), capi._ptr(u),
                capi._ptr(A), capi._ptr(B), capi._ptr(fv))
    assert rc == 0, (c.id, env, rc)
    for w, size in ((Aw, n * n), (Bw, n * m), (fw, n)):
        assert np.all(w[p * size:] == np.uint64(GUARD)), (c.id, env, "the record beyond the last point was written")
        assert not np.any(w[:p * size] == np.uint64(GUARD)), (c.id, env, "a record was not written")
    return (A[:p * n * n].reshape(p, n, n).transpose(0, 2, 1).copy(), B[:p * n * m].reshape(p, m, n).transpose(0, 2, 1).copy(),
            fv[:p * n].reshape(p, n).copy())


def _hold_linearisation(c, got, ref, tol, which=None):
    worst = 0.0
    for i in (range(len(ref[0])) if which is None else which):
        for g, r, name in zip(got, ref, "ABf"):
            e = nc.rel(g[i], r[i])
            worst = max(worst, e)
            assert e <= tol, (c.id, name, i, e)
    return worst


@pytest.mark.parametrize("case", nc.LIN, ids=_ids)
def test_linearisation_matches_the_restatement_on_every_build(capi, monkeypatch, case):
    """A, B and f of every point against the float64 restatement; the default build, one point per wave and the workgroup build equal
    bit for bit; nothing written beyond the last point (an odd count leaves a half-wave that computes on point 0 and stores nothing)"""
    x, u = nc.lin_points(case)
    ref = nc.lin_reference(case)
    got = _linearize(capi, case, x, u, {}, monkeypatch)
    _note("lin", case.id, _hold_linearisation(case, got, ref, nc.lin_tol(case)), nc.lin_tol(case))
    for env in case.envs:
        other = _linearize(capi, case, x, u, env, monkeypatch)
        for a, b, name in zip(got, other, "ABf"):
            assert np.array_equal(a, b), (case.id, nc.env_id(env), name, float(np.abs(a - b).max()))


@pytest.mark.parametrize("case", nc.LIN_BIG, ids=_ids)
def test_linearisation_second_pass_of_the_grid(capi, monkeypatch, case):
    """num_cus * 8 workgroups * 4 waves * ppw points and five more: the stride loop of k_fnn_jacobian_w takes a second, partial pass"""
    cus = _num_cus()
    env = case.envs[0] if case.envs else {}
    p = case.points(cus)
    assert nc.lin_build(*case.net, case.kind, env) == ("w", 64 // case.big, nc.NET[case.kind]) and nc.lin_grid(p, case.big, cus)[1] == 2
    x, u = nc.lin_points(case, cus)
    ref = nc.lin_reference(case, cus)
    got = _linearize(capi, case, x, u, env, monkeypatch)
    tol = nc.lin_tol(case)
    worst = max(nc.rel(g, r) for g, r in zip(got, ref))
    assert worst <= tol, (case.id, worst)
    f = nc.model(case)
    for g, r, name in zip(got, ref, "ABf"):        # every point on its own scale
        err = np.abs(g - r).reshape(p, -1).max(axis=1) / np.maximum(np.abs(r).reshape(p, -1).max(axis=1), 1e-300)
        assert err.max() <= tol, (case.id, name, int(err.argmax()), float(err.max()))
        worst = max(worst, float(err.max()))
    for i in range(p - 5, p):                       # the second pass, by name, against the per-point model
        Ar, Br = f.jacobian(x[i], u[i])
        assert nc.rel(got[0][i], Ar) <= tol and nc.rel(got[1][i], Br) <= tol and nc.rel(got[2][i], f.forward(x[i], u[i])) <= tol, (case.id, i)
    _note("lin", "%s cus %d points %d" % (case.id, cus, p), worst, tol)
    other = _linearize(capi, case, x, u, nc.FNN_WG, monkeypatch)
    for a, b, name in zip(got, other, "ABf"):
        assert np.array_equal(a, b), (case.id, name)


# ---------------------------------------------------------------------------- time-varying design
def _solver(capi, c, env, monkeypatch):
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return capi.Solver(c.n, c.m, c.N, c.batch)


@pytest.mark.parametrize("case", nc.LTV, ids=_ids)
def test_ltv_design_matches_the_oracle_on_both_builds(capi, monkeypatch, case):
    """H and q of k_design_ltv_reg<NC, 4> and of k_design_ltv (ALMPC_LTV_LDS) against mo.ltv_qp, the solution against the exact box-QP
    solver, every status 0 -- each build against the oracle, not against the other"""
    a, ref = nc.ltv_inputs(case), nc.ltv_reference(case)
    for env in case.all_envs():
        assert nc.ltv_build(*case.shape, env) is not None
        s = _solver(capi, case, env, monkeypatch)
        s.design_ltv(a["A_all"], a["B_all"], a["c_all"], a["xbar"], a["ubar"], a["x_ref"], a["u_ref"], a["Q"], a["R"], a["S"], a["P"],
                     a["umin"], a["umax"])
        s.update_initialization(a["xbar"][:, :, 0])
        s.calculate()
        r = s.get_results(want=("u", "e_u", "status", "iters", "polish_iters"))
        eh = eq = eu = 0.0
        for i in range(case.batch):
            H, q, v = ref[i]["H"], ref[i]["q"], ref[i]["v"]
            eh = max(eh, np.abs(s.get_design_instance(i)["H"] - H).max() / np.abs(H).max())
            eq = max(eq, np.abs(s.get_gradient_instance(i) - q).max() / max(1.0, np.abs(q).max()))
            eu = max(eu, np.abs(r["e_u"][i].T.reshape(-1) - v).max())
            eu = max(eu, np.abs(r["u"][i] - (a["ubar"][i] + v.reshape(case.N, case.m).T)).max())
        s.close()
        _note("ltv", case.id + " " + nc.env_id(env), eh, 1e-11)
        _note("ltv-q", case.id + " " + nc.env_id(env), eq, 1e-11)
        _note("ltv-u", case.id + " " + nc.env_id(env), eu, U_TOL)
        assert np.all(r["status"] == 0), (case.id, env, r["status"])
        assert eh <= 1e-11 and eq <= 1e-11 and eu <= U_TOL, (case.id, env, eh, eq, eu)


# ---------------------------------------------------------------------------- the SQP loop
def _sqp_solver(capi, c, env, monkeypatch):
    kw, X0 = nc.nlp_problem(c)
    f = nc.model(c)
    s = _solver(capi, c, env, monkeypatch)
    args = (f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"])
    if c.kind == "densenet":
        s.sqp_densenet_setup(*args, act=c.act)
    else:
        s.sqp_fnn_setup(*args, act=c.act, net=c.kind)
    return s, kw, X0, f


def _iterates(capi, c, env, monkeypatch, step_rule="fixed"):
    """[(u, x)] after sqp_fnn_start and after each of SQP_ITERS single iterations, and the histories"""
    s, kw, X0, f = _sqp_solver(capi, c, env, monkeypatch)
    # the start is read through an iteration with a step of 2^-60 (the results exist only after an iteration: at most 1e-18 |dx| from
    # the start's own rollout), then made again
    s.sqp_fnn_start(X0)
    s.sqp_fnn_iterate(1, step_scale=2.0 ** -60)
    r = s.get_results(want=("u", "x"))
    out, st, de = [(r["u"].copy(), r["x"].copy())], [], []
    s.sqp_fnn_start(X0)
    for _ in range(nc.SQP_ITERS):
        a, b = s.sqp_fnn_iterate(1, step_rule=step_rule)
        st.append(a[0]); de.append(b[0])
        r = s.get_results(want=("u", "x", "status"))
        assert np.all(r["status"] == 0), (c.id, env, r["status"])
        out.append((r["u"].copy(), r["x"].copy()))
    assert s.sqp_fnn_skipped().sum() == 0
    s.close()
    return out, np.array(st), np.array(de)


def _hold_iterates(c, mo, runs, ref, st, de, what):
    kw, X0 = nc.nlp_problem(c)
    f = nc.model(c)
    eu = ex_ = er = 0.0
    for i in range(c.batch):
        Xs, Us = nc.start_rollout(c, i)
        u0, x0 = runs[0][0][i], runs[0][1][i]
        assert np.abs(u0 - Us).max() <= 1e-15 and np.abs(x0 - Xs).max() <= 1e-12 * max(1.0, np.abs(Xs).max()), (c.id, i)
        for it in range(nc.SQP_ITERS):
            u, x = runs[it + 1][0][i], runs[it + 1][1][i]
            eu = max(eu, np.abs(u - ref[i]["U"][it]).max()); ex_ = max(ex_, np.abs(x - ref[i]["X"][it]).max())
        h = ref[i]["hist"][-1]
        if h is not None and h[1] <= 1e-9 and h[0] <= 1e-6:      # converged defects: x is the network's own rollout of u
            er = max(er, np.abs(x - mo.fnn_rollout(f, X0[i], u)).max())
    _note(what + "-u", c.id, eu, U_TOL); _note(what + "-x", c.id, ex_, X_TOL); _note(what + "-rollout", c.id, er, 1e-9)
    assert eu <= U_TOL and ex_ <= X_TOL and er <= 1e-9, (c.id, eu, ex_, er)
    H = np.array([[h if h is not None else (0.0, 0.0) for h in ref[i]["hist"]] for i in range(c.batch)])
    if all(h is not None for i in range(c.batch) for h in ref[i]["hist"]):
        np.testing.assert_allclose(st, H[:, :, 0].max(axis=0), rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(de, H[:, :, 1].max(axis=0), rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("case", nc.SQP, ids=_ids)
def test_sqp_iterates_match_the_restatement_per_iteration(capi, mo, monkeypatch, case):
    """sqp_fnn_start reproduces the rollout of the clipped u_ref; after each of four Gauss-Newton iterations u and x follow mo.sqp_fnn run
    for the same count, on every instance; the separate k_sqp_prepare launch changes no bit and the separate k_design_scale launch no more than its
    existing test allows; the LDS build of the
    design (k_design_ltv) follows the restatement as well"""
    ref = nc.sqp_reference(case)
    assert nc.sqp_supported(*case.shape)
    runs, st, de = _iterates(capi, case, {}, monkeypatch)
    _hold_iterates(case, mo, runs, ref, st, de, "sqp")
    for env in case.envs:
        other, st2, de2 = _iterates(capi, case, env, monkeypatch)
        if env == nc.LTV_LDS:
            _hold_iterates(case, mo, other, ref, st2, de2, "sqp-ltv_lds")
            continue
        d = max(max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()) for a, b in zip(runs, other))
        # k_sqp_prepare as a launch of its own: the same threads doing the same arithmetic, no bit changes.  k_design_scale as a launch of
        # its own: v0S_i = -G_i fS_i then comes from k_neg_gm and not from the inverse's launch, in another summation order (measured: up
        # to 4e-14 on u and x after four iterations) -- held to the 1e-9 of test_scaling_in_the_design_kernels_tail_equals_the_split_launches
        bound = 0.0 if env == nc.SPLIT_PREPARE else 1e-9
        _note("sqp-" + nc.env_id(env), case.id, d, bound)
        assert d <= bound, (case.id, nc.env_id(env), d)


@pytest.mark.parametrize("case", [c for c in nc.SQP if "chunked" in c.tags], ids=_ids)
def test_sqp_chunked_walk_under_the_merit_rule_and_the_solve(capi, mo, monkeypatch, case):
    """n = 16, N = 59: k_sqp_step and k_sqp_kkt stage 39 + 20 stages.  The merit rule (xback, dxback) against mo.sqp_fnn(adaptive);
    almpc_sqp_fnn_solve (k_sqp_kkt walks the chunks backwards) against sqp_solve_ref"""
    assert nc.sqp_chunks(*case.shape) == [39, 20]
    runs, st, de = _iterates(capi, case, {}, monkeypatch, step_rule="merit")
    _hold_iterates(case, mo, runs, nc.sqp_reference(case, True), st, de, "sqp-merit")
    s, kw, X0, f = _sqp_solver(capi, case, {}, monkeypatch)
    s.sqp_fnn_start(X0)
    out = s.sqp_fnn_solve(nc.SOLVE_ITERS, nc.SOLVE_TOL)
    r = s.get_results(want=("u", "x"))
    s.close()
    ref = nc.solve_reference(case)
    for i in range(case.batch):
        e = ref[i]
        assert e["status"] == out["status"][i] and abs(e["iters"] - out["iters"][i]) <= 1, (case.id, i, e["status"], e["iters"], out["iters"][i])
        if out["status"][i] == 0:
            assert out["kkt"][i] <= nc.SOLVE_TOL, (case.id, i, out["kkt"][i])
            assert np.abs(r["x"][i] - mo.fnn_rollout(f, X0[i], r["u"][i])).max() <= 1e-9, (case.id, i)
            res, dmax, _ = sref.adjoint_residual(f, r["x"][i], r["u"][i], *nc._args(kw))
            _note("solve-kkt", "%s[%d]" % (case.id, i), res, 10 * nc.SOLVE_TOL)
            assert res <= 10 * nc.SOLVE_TOL and dmax <= 10 * sref.DEFECT_TOL, (case.id, i, res, dmax)


@pytest.mark.parametrize("case", nc.SQP_REFUSED, ids=_ids)
def test_sqp_beyond_the_steps_rollout_is_refused_by_the_first_iteration(capi, monkeypatch, case):
    """n above 16: sqp_fnn_setup and sqp_fnn_start serve the shape (the linearisation, k_design_ltv_reg and k_sqp_step would), the step
    behind the QP does not -- the first iteration says so and leaves the handle usable"""
    assert nc.sqp_supported(*case.shape) and not nc.step_supported(*case.shape)
    s, kw, X0, f = _sqp_solver(capi, case, {}, monkeypatch)
    s.sqp_fnn_start(X0)
    with pytest.raises(capi.AlmpcError) as e:
        s.sqp_fnn_iterate(1)
    assert e.value.code == -4 and "fused rollout" in str(e.value)      # ALMPC_ERR_UNSUPPORTED
    s.sqp_fnn_start(X0)
    s.close()


# ---------------------------------------------------------------------------- the exact Hessian
@pytest.mark.parametrize("case", nc.EXACT, ids=_ids)
def test_exact_first_qp_matches_the_restatement(capi, monkeypatch, case):
    """H and q of the first QP of the exact mode (k_sqp_kkt's multipliers, k_fnn_lag_hessian, k_sqp_exact_qp) against
    sqp_exact_ref.exact_qp with the kind's own stage Hessian; a kind whose scratch does not pass sqp_exact_check is refused"""
    s, kw, X0, f = _sqp_solver(capi, case, {}, monkeypatch)
    if not nc.exact_supported(case.kind, *case.net, case.N, case.act):
        assert "refused" in case.tags
        with pytest.raises(capi.AlmpcError) as e:
            s.sqp_fnn_set_hessian("exact")
        assert e.value.code == -4      # ALMPC_ERR_UNSUPPORTED
        s.close()
        return
    assert "refused" not in case.tags
    s.sqp_fnn_set_hessian("exact")
    s.sqp_fnn_start(X0)
    s.sqp_fnn_iterate(1, step_rule="merit")
    ref = nc.exact_reference(case)
    eh = eq = 0.0
    for i in range(case.batch):
        He, qe = ref[i]
        eh = max(eh, np.abs(s.get_design_instance(i)["H"] - He).max() / np.abs(He).max())
        eq = max(eq, np.abs(s.get_gradient_instance(i) - qe).max() / max(1.0, np.abs(qe).max()))
    s.close()
    _note("exact-H", case.id, eh, 1e-10); _note("exact-q", case.id, eq, 1e-10)
    assert eh <= 1e-10 and eq <= 1e-10, (case.id, eh, eq)


# ---------------------------------------------------------------------------- re-linearisation
def _relin(capi, c, env, monkeypatch):
    kw, X0 = nc.nlp_problem(c)
    f, ref = nc.model(c), nc.relin_reference(c)
    s = _solver(capi, c, env, monkeypatch)
    s.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], None, ref["P"], kw["u_min"], kw["u_max"],
                      act=c.act, net=c.kind)
    s.update_initialization(X0)
    s.relin_fnn_step(capi.default_opts())
    r = s.get_results()
    models = [s.model_instance(i) for i in range(c.batch)]
    s.relin_fnn_advance()
    s.relin_fnn_step(capi.default_opts())
    r2 = s.get_results()
    s.close()
    return r, models, r2


@pytest.mark.parametrize("case", nc.RELIN, ids=_ids)
def test_relin_with_the_jacobian_in_the_design_kernels_head(capi, monkeypatch, case):
    """One step and one advance of the re-linearisation pipeline with the network linearised by k_design_instance_t<NC, MC> itself and
    (ALMPC_DBG_SPLIT_JACOBIAN) by k_fnn_jacobian_w in front of it: the same models and results bit for bit, the models the
    restatement's, the predicted errors those of the restated linearisation, u the exact oracle's, advance on the network itself"""
    kw, X0 = nc.nlp_problem(case)
    f, ref = nc.model(case), nc.relin_reference(case)
    assert nc.design_fuses_fnn(*case.shape, case.H, case.L) and not nc.design_fuses_fnn(*case.shape, case.H, case.L, env=nc.SPLIT_JACOBIAN)
    r, models, r2 = _relin(capi, case, {}, monkeypatch)
    assert np.all(r["status"] == 0), (case.id, r["status"])
    em = ep = eu = ea = 0.0
    for i in range(case.batch):
        A, B = ref["inst"][i]["A"], ref["inst"][i]["B"]
        em = max(em, nc.rel(models[i][0], A), nc.rel(models[i][1], B))
        e_x, e_u = r["e_x"][i], r["e_u"][i]
        pred = np.stack([A @ e_x[:, k] + B @ e_u[:, k] for k in range(case.N)], axis=1)
        ep = max(ep, nc.rel(e_x[:, 1:], pred))
        eu = max(eu, np.abs(r["u"][i] - ref["inst"][i]["exact"]["u"]).max())
        xw = f.forward(X0[i], r["u"][i][:, 0])
        ea = max(ea, np.abs(r2["x"][i][:, 0] - xw).max() / max(1.0, np.abs(xw).max()))
    _note("relin-model", case.id, em, 1e-12); _note("relin-pred", case.id, ep, 1e-9); _note("relin-u", case.id, eu, 1e-6)
    _note("relin-advance", case.id, ea, 1e-12)
    assert em <= 1e-12 and ep <= 1e-9 and eu <= 1e-6 and ea <= 1e-12, (case.id, em, ep, eu, ea)
    rs, ms, rs2 = _relin(capi, case, nc.SPLIT_JACOBIAN, monkeypatch)
    for i in range(case.batch):
        assert np.array_equal(models[i][0], ms[i][0]) and np.array_equal(models[i][1], ms[i][1]), (case.id, i)
    for a, b in ((r, rs), (r2, rs2)):
        for k in ("u", "x", "e_u", "e_x", "status", "iters", "polish_iters"):
            assert np.array_equal(a[k], b[k]), (case.id, k)
