"""GPU tests of the stage-wise solvers at every instantiated shape (pytest -m gpu): k_sdual (csrc/almpc_sdual.hip.h) in each of its
SD_SHAPES builds -- exact-fit and padded shapes, input box / state box / terminal equality / input-rate weight, both sweep paths
(DPP rows of 16 lanes, LDS), every scan grouping G = 64 / (NT + MC) down to 2 and 1, the builds with and without cached responses, the
capacity tiers, the horizon edge N = 64 G - 1 -- and k_riccati (csrc/almpc_riccati.hip.h) as a first solver in its specialised and its
generic build.  The cases and their well-posedness: tests/stagewise_shape_cases.py, tests/test_stagewise_shape_cases.py.
Oracles and tolerances as tests/test_gpu_stagewise.py: mpc_oracle.solve_mpc_exact at 1e-6 on u (1e-5 on x), status 3 <-> it raises
ValueError; the numpy restatement of k_sdual's algorithm at 1e-9 with equal counts of working-set changes where one launch decides;
mpc_oracle.solve_mpc_structured (the restatement of k_riccati) at 1e-8."""
import numpy as np
import pytest

import stagewise_shape_cases as sc

pytestmark = pytest.mark.gpu

U_TOL = 1e-6


def _solve(capi, c, p, X0, **kw):
    s = capi.Solver(p.n, p.m, p.N, len(X0), structured=True, **kw)
    s.design_shared(p.A, p.B, p.Q, p.R, p.S if c.S else None, None, p.u_min, p.u_max, xmin=p.x_min, xmax=p.x_max, terminal=p.terminal)
    s.set_reference(p.x_ref, p.u_ref)
    s.update_initialization(X0)
    s.calculate()
    r = s.get_results()
    s.close()
    return r


def _properties(p, X0, r):
    """every solved instance: dynamics, input box, state box, terminal equality (tests/test_gpu_stagewise.py)"""
    ok = r["status"] == 0
    ex, eu = r["e_x"][ok], r["e_u"][ok]
    if ok.any():
        pred = np.einsum("ij,bjk->bik", p.A, ex[:, :, :-1]) + np.einsum("ij,bjk->bik", p.B, eu)
        assert np.abs(pred - ex[:, :, 1:]).max() <= 1e-8 * max(1.0, np.abs(ex).max())
        assert np.all(r["u"][ok] >= p.u_min[None, :, None]) and np.all(r["u"][ok] <= p.u_max[None, :, None])
        if p.x_min is not None:
            assert np.all(r["x"][ok] >= p.x_min[None, :, None] - 1e-7) and np.all(r["x"][ok] <= p.x_max[None, :, None] + 1e-7)
        if p.terminal == "equality":
            assert np.abs(ex[:, :, -1]).max() <= 1e-7
    np.testing.assert_array_equal(r["x"][:, :, 0], X0)


def _check(c, ref, r, tag=""):
    """statuses, u and x of the sampled instances against the exact oracle; statuses, u and the count of working-set changes of four
    instances against the restatement.  Returns the largest |u - u_exact|."""
    assert set(np.unique(r["status"])) <= {0, 3}, np.bincount(r["status"])
    _properties(ref["p"], ref["X0"], r)
    err = 0.0
    for i, e in ref["exact"].items():
        if e is None:
            assert r["status"][i] == 3, (i, r["status"][i])
            continue
        assert r["status"][i] == 0, (i, r["status"][i])
        err = max(err, float(np.abs(r["u"][i] - e["u"]).max()))
        assert np.abs(r["u"][i] - e["u"]).max() <= U_TOL, (i, np.abs(r["u"][i] - e["u"]).max())
        assert np.abs(r["x"][i] - e["x"]).max() <= 1e-5, (i, np.abs(r["x"][i] - e["x"]).max())
    for i, o in ref["restated"].items():
        assert o["status"] == r["status"][i], (i, o["status"], r["status"][i])
        if o["status"] == 0:
            assert np.abs(r["u"][i] - o["u"]).max() <= 1e-9, (i, np.abs(r["u"][i] - o["u"]).max())
            if o["first_tier"]:
                assert o["iters"] == r["polish_iters"][i], (i, o["iters"], r["polish_iters"][i])
    print(f"max |u - u_exact| build {c.build} case {c.id}{tag}: {err:.2e}")
    return err


def _same(a, b):
    assert np.array_equal(a["status"], b["status"])
    ok = a["status"] == 0
    if ok.any():
        assert np.abs(a["u"][ok] - b["u"][ok]).max() <= 1e-9, np.abs(a["u"][ok] - b["u"][ok]).max()


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.id)
def test_every_build_against_the_exact_oracle(capi, case):
    ref = sc.reference(case)
    _check(case, ref, _solve(capi, case, ref["p"], ref["X0"]))


@pytest.mark.parametrize("cid", sc.VARIANT_CASES)
def test_every_build_without_cached_responses(capi, monkeypatch, cid):
    """ALMPC_SDUAL_NO_GHAT: the build that keeps the records r1[NT], sb[MC], r2[NT], r3[MC] in registers and runs two sweeps per
    working-set change: same statuses and optimum as the default, and the oracle's on its own"""
    case = sc.CASE_BY_ID[cid]
    ref = sc.reference(case)
    monkeypatch.delenv("ALMPC_SDUAL_NO_GHAT", raising=False)
    cached = _solve(capi, case, ref["p"], ref["X0"])
    monkeypatch.setenv("ALMPC_SDUAL_NO_GHAT", "1")
    sweeps = _solve(capi, case, ref["p"], ref["X0"])
    monkeypatch.delenv("ALMPC_SDUAL_NO_GHAT", raising=False)
    _check(case, ref, sweeps, " (no cached responses)")
    _same(cached, sweeps)


@pytest.mark.parametrize("cid", sc.WIDE_CASES)
def test_a_wide_build_with_the_table_built_but_not_used(capi, monkeypatch, cid):
    case = sc.CASE_BY_ID[cid]
    ref = sc.reference(case)
    monkeypatch.delenv("ALMPC_SDUAL_NO_GH", raising=False)
    default = _solve(capi, case, ref["p"], ref["X0"])
    monkeypatch.setenv("ALMPC_SDUAL_NO_GH", "1")
    plain = _solve(capi, case, ref["p"], ref["X0"])
    monkeypatch.delenv("ALMPC_SDUAL_NO_GH", raising=False)
    _check(case, ref, plain, " (table not used)")
    _same(default, plain)


@pytest.mark.parametrize("case,above,within", sc.TIER_CASES, ids=lambda v: f"{v.id}-amp{v.amp:g}" if isinstance(v, sc.Case) else None)
def test_capacity_tiers_at_the_wide_builds(capi, monkeypatch, case, above, within):
    """Working sets beyond the 32 rows of the first launch and beyond the 64 of the second (two positions per lane) at G = 2 and
    G = 1; the same again with tiers that do not hand each other the inverse of their working set."""
    ref = sc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    nact = [sc.active_inputs(p, e["u"]) for e in ref["exact"].values()]
    assert max(nact) > above, "the inputs do not reach the tier the test is about"
    if within:
        assert min(nact) <= 32
    monkeypatch.delenv("ALMPC_SDUAL_NO_SINV_HANDOVER", raising=False)
    r = _solve(capi, case, p, X0)
    assert np.all(r["status"] == 0), np.bincount(r["status"])
    _check(case, ref, r, f" (amplitude {case.amp:g}, {min(nact)}..{max(nact)} active rows)")
    monkeypatch.setenv("ALMPC_SDUAL_NO_SINV_HANDOVER", "1")
    r2 = _solve(capi, case, p, X0)
    monkeypatch.delenv("ALMPC_SDUAL_NO_SINV_HANDOVER", raising=False)
    _same(r, r2)


@pytest.mark.parametrize("cid", sc.SCREEN_CASES)
def test_infeasibility_verdicts_by_the_kernel_itself(capi, monkeypatch, cid):
    """ALMPC_SDUAL_NO_SCREEN: no reachability screen in front of the solve -- k_sdual itself finds the dependent row without a
    blocking multiplier: the statuses of the default run and of the oracle"""
    case = sc.CASE_BY_ID[cid]
    ref = sc.reference(case)
    assert sum(e is None for e in ref["exact"].values()) >= 1
    monkeypatch.delenv("ALMPC_SDUAL_NO_SCREEN", raising=False)
    default = _solve(capi, case, ref["p"], ref["X0"])
    monkeypatch.setenv("ALMPC_SDUAL_NO_SCREEN", "1")
    own = _solve(capi, case, ref["p"], ref["X0"])
    monkeypatch.delenv("ALMPC_SDUAL_NO_SCREEN", raising=False)
    _check(case, ref, own, " (no screen)")
    _same(default, own)
    assert np.all(own["polish_iters"][own["status"] == 3] >= 1)      # (decided by working-set changes, not in front of them)


@pytest.mark.parametrize("case", sc.EDGE_CASES, ids=lambda c: c.id)
def test_the_horizon_edge(capi, case):
    """N = 64 G - 1: the last stages use bit 63 of the working-set mask (their rows are active: test_stagewise_shape_cases.py)"""
    assert case.N == sc.n_max(case.build)
    ref = sc.reference(case)
    _check(case, ref, _solve(capi, case, ref["p"], ref["X0"]))


def test_one_stage_past_the_edge_is_the_primal_solvers_or_refused(capi, mo):
    """(17, 1, 64): outside sdual_shape_ok.  Input box only: k_riccati takes the handle; with a state box: ALMPC_ERR_UNSUPPORTED."""
    c = sc.Case(17, 1, 64, 0, "ubox", 3.0)
    assert c.N == sc.n_max(c.build) + 1
    p, X0 = sc.inputs(c)
    s = capi.Solver(p.n, p.m, p.N, len(X0), structured=True)
    s.design_shared(p.A, p.B, p.Q, p.R, None, None, p.u_min, p.u_max)
    s.set_reference(p.x_ref, p.u_ref)
    s.update_initialization(X0)
    s.calculate()
    r = s.get_results()
    assert np.all(r["status"] == 0)
    _properties(p, X0, r)
    for i in sc.RESTATED:
        e = mo.solve_mpc_exact(p, X0[i])
        assert np.abs(r["u"][i] - e["u"]).max() <= U_TOL and np.abs(r["x"][i] - e["x"]).max() <= 1e-5
        assert np.abs(r["u"][i] - mo.solve_mpc_structured(p, X0[i])["u"]).max() <= 1e-8
    with pytest.raises(capi.AlmpcError) as ei:
        s.design_shared(p.A, p.B, p.Q, p.R, None, None, p.u_min, p.u_max, xmin=-2.0 * np.ones(p.n), xmax=2.0 * np.ones(p.n))
    assert ei.value.code == -4
    s.close()


def _solve_primal(capi, p, X0):
    s = capi.Solver(p.n, p.m, p.N, len(X0), structured=True)
    s.design_shared(p.A, p.B, p.Q, p.R, None, None, p.u_min, p.u_max)
    s.set_reference(p.x_ref, p.u_ref)
    s.update_initialization(X0)
    s.calculate()
    r = s.get_results()
    s.close()
    return r


@pytest.mark.parametrize("case", sc.RICCATI_CASES, ids=lambda c: c.id)
def test_the_primal_solver_as_the_first_solver(capi, mo, monkeypatch, case):
    """ALMPC_STRUCTURED_PRIMAL: k_riccati decides every instance of a structured handle -- its builds specialised for (12, 4), (4, 2),
    (2, 1), each also through the generic one (ALMPC_RICCATI_GENERIC), and shapes only the generic one takes"""
    ref = sc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    monkeypatch.setenv("ALMPC_STRUCTURED_PRIMAL", "1")
    monkeypatch.delenv("ALMPC_RICCATI_GENERIC", raising=False)
    runs = [_solve_primal(capi, p, X0)]
    if (case.n, case.m) in sc.RICCATI_SHAPES:
        monkeypatch.setenv("ALMPC_RICCATI_GENERIC", "1")
        runs.append(_solve_primal(capi, p, X0))
        monkeypatch.delenv("ALMPC_RICCATI_GENERIC", raising=False)
    # what the primal solver does not build is refused under the switch
    s = capi.Solver(p.n, p.m, p.N, 2, structured=True)
    for kw in (dict(S=0.5 * np.eye(p.m)), dict(xmin=-2.0 * np.ones(p.n), xmax=2.0 * np.ones(p.n))):
        with pytest.raises(capi.AlmpcError) as ei:
            s.design_shared(p.A, p.B, p.Q, p.R, kw.get("S"), None, p.u_min, p.u_max, xmin=kw.get("xmin"), xmax=kw.get("xmax"))
        assert ei.value.code == -4
    s.close()
    monkeypatch.delenv("ALMPC_STRUCTURED_PRIMAL", raising=False)
    for k, r in enumerate(runs):
        assert np.all(r["status"] == 0), np.bincount(r["status"])
        _properties(p, X0, r)
        err = 0.0
        for i, e in ref["exact"].items():
            err = max(err, float(np.abs(r["u"][i] - e["u"]).max()))
            assert np.abs(r["u"][i] - e["u"]).max() <= U_TOL and np.abs(r["x"][i] - e["x"]).max() <= 1e-5, i
        for i in case.restated:
            assert np.abs(r["u"][i] - mo.solve_mpc_structured(p, X0[i])["u"]).max() <= 1e-8, i
        print(f"max |u - u_exact| k_riccati {'generic' if k or (case.n, case.m) not in sc.RICCATI_SHAPES else 'specialised'} case {case.id}: {err:.2e}")
    if len(runs) == 2:
        assert np.abs(runs[0]["u"] - runs[1]["u"]).max() <= 1e-9
        assert np.array_equal(runs[0]["polish_iters"], runs[1]["polish_iters"])


@pytest.mark.parametrize("n,m,N", [(11, 5, 8)])
@pytest.mark.parametrize("rows", ["ubox", "S_xbox"])
def test_per_instance_models_at_the_wide_builds(capi, mo, n, m, N, rows):
    """almpc_design_batched on a structured handle: the records of k_sgains (runtime NT, MC) read by the (16, 8) build; one model per
    instance, every instance against the exact oracle on its own model; with S and a state box as well.  ((20, 9, 6) would take the
    (32, 16) build without cached responses: left out, see stagewise_shape_cases.VARIANT_CASES.)"""
    b = 24
    rng = np.random.default_rng(1000 * n + 10 * m + N + 5)
    As, Bs = [], []
    for _ in range(b):
        A = rng.standard_normal((n, n)); A *= (0.7 + 0.3 * rng.random()) / np.max(np.abs(np.linalg.eigvals(A)))
        As.append(A); Bs.append(rng.standard_normal((n, m)))
    As, Bs = np.stack(As), np.stack(Bs)
    x_ref = 0.1 * rng.standard_normal(n)[:, None] * np.ones((n, N + 1)); u_ref = np.tile(np.linspace(-0.1, 0.1, N), (m, 1))
    umin, umax = -0.5 * np.ones(m), 0.7 * np.ones(m)
    X0 = 3.0 * rng.standard_normal((b, n))
    kw, des = {}, {}
    if rows == "S_xbox":
        X0 = np.clip(X0, -0.99 * sc.XBOX, 0.99 * sc.XBOX)
        kw = dict(s=0.5, x_min=-sc.XBOX * np.ones(n), x_max=sc.XBOX * np.ones(n))
        des = dict(S=0.5 * np.eye(m), xmin=kw["x_min"], xmax=kw["x_max"])
    s = capi.Solver(n, m, N, b, structured=True)
    s.design_batched(As, Bs, 10.0 * np.eye(n), 1.0 * np.eye(m), des.get("S"), None, umin, umax, xmin=des.get("xmin"), xmax=des.get("xmax"))
    s.set_reference(x_ref, u_ref)
    s.update_initialization(X0)
    s.calculate()
    r = s.get_results()
    s.close()
    assert set(np.unique(r["status"])) <= {0, 3}
    np.testing.assert_array_equal(r["x"][:, :, 0], X0)
    n_ok = nact = 0
    err = 0.0
    for i in range(b):
        p = mo.make_problem(As[i], Bs[i], N, umin, umax, x_ref=x_ref, u_ref=u_ref, q=10.0, r=1.0, **kw)
        e = sc.exact_or_none(p, X0[i])
        if e is None:
            assert r["status"][i] == 3, i
            continue
        assert r["status"][i] == 0, (i, r["status"][i])
        err = max(err, float(np.abs(r["u"][i] - e["u"]).max()))
        assert np.abs(r["u"][i] - e["u"]).max() <= U_TOL and np.abs(r["x"][i] - e["x"]).max() <= 1e-5, i
        n_ok += 1
        nact += sc.active_inputs(p, e["u"])
    assert n_ok >= (b if rows == "ubox" else 4) and nact >= 1
    print(f"max |u - u_exact| build {sc.pick_build(n + m if kw else n, m)} per-instance models ({n}, {m}, {N}) {rows}: {err:.2e}, {n_ok} solved")


@pytest.mark.parametrize("n,m,N", [(40, 3, 20), (20, 9, 6)])
def test_the_redo_on_a_condensed_handle_at_the_wide_builds(capi, mo, n, m, N):
    """A condensed handle takes n <= 64: n = 40 without S reaches the (48, 16) build, which no structured handle does.  A finish
    capped at two working-set changes leaves the saturated instances undecided; the stage-wise redo solves them, the others stay
    bit-identical."""
    c = sc.Case(n, m, N, 0, "ubox", 10.0)
    assert c.build == ((48, 16) if n == 40 else (32, 16))
    p, X0 = sc.inputs(c)
    opts = capi.default_opts(polish_max_iter=2)
    out = {}
    for fb in (False, True):
        s = capi.Solver(n, m, N, len(X0), structured_fallback=fb)
        s.design_shared(p.A, p.B, p.Q, p.R, None, None, p.u_min, p.u_max)
        s.set_reference(p.x_ref, p.u_ref)
        s.update_initialization(X0)
        s.calculate(opts)
        out[fb] = s.get_results()
        s.close()
    left = out[False]["status"] != 0
    assert left.sum() >= 1, "no instance was left to the redo"
    assert np.all(out[True]["status"] == 0)
    for key in ("u", "x", "polish_iters"):
        assert np.array_equal(out[False][key][~left], out[True][key][~left]), key
    err = 0.0
    for i in range(len(X0)):
        e = mo.solve_mpc_exact(p, X0[i])
        err = max(err, float(np.abs(out[True]["u"][i] - e["u"]).max()))
        assert np.abs(out[True]["u"][i] - e["u"]).max() <= U_TOL, (i, np.abs(out[True]["u"][i] - e["u"]).max())
        if left[i]:
            assert np.abs(out[True]["x"][i] - e["x"]).max() <= 1e-5, i
    print(f"max |u - u_exact| build {c.build} redo on a condensed handle ({n}, {m}, {N}): {err:.2e}, {int(left.sum())} redone")
