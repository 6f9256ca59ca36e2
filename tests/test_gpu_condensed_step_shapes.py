"""The condensed shared-model step (almpc_design_shared -> almpc_calculate) at every build and route: the cases of
tests/condensed_step_cases.py against the oracles.  Run on an MI355X: pytest -m gpu.

Every handle is created with structured_fallback=False: the verdict is the condensed step's own, an instance its finish leaves
without a certificate stays at status 1 and no stage-wise solver runs.  The switches (ALMPC_*) are read by almpc_create: they are set
before the handle is made.  Tolerances are the project's: IT_TOL on ADMM iterates (test_admm_only_matches_oracle_iterate), U_TOL and
10 X_TOL against the exact oracle (test_random_stable_plants_of_many_shapes), 1e-12 / 1e-10 between k_polish<true> and <false>
(test_polish_through_l2_build_matches_lds_build), 1e-9 / 1e-8 between the one-wave and the tile route
(test_one_wave_step_of_small_shared_problems_equals_the_two_launch_path), the dynamics residual of test_full_size_batch_properties
evaluated in long double, and bit for bit where the same device functions run on the same values.

Lines that start with `condensed-step` print the measured maxima (pytest -s)."""
import numpy as np
import pytest

import condensed_step_cases as cc

pytestmark = pytest.mark.gpu

IT_TOL = 1e-9
U_TOL = 1e-6
X_TOL = 1e-5
KEYS = ("u", "e_u", "x", "e_x", "status", "iters", "polish_iters")
PROFILES = [("scalar", 0.1), ("stiffness", 30.0)]
ITERATE_OPTS = [(1, 1), (2, 1), (7, 7)]
NO_WAVE = {"ALMPC_NO_SHARED_WAVE": "1"}
_ids = lambda c: c.id


def _note(what, key, value, bound=None):
    print("condensed-step %s %s %.3e%s" % (what, key, value, "" if bound is None else " of %.1e" % bound))


def _solver(capi, c, p, batch=cc.BATCH, rho=0.1, profile="scalar", refs=None):
    s = capi.Solver(p.n, p.m, p.N, batch, structured_fallback=False)
    s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=rho, rho_profile=profile)
    if refs is None:
        s.set_reference(p.x_ref, p.u_ref)
    else:
        s.set_reference(refs[0][:batch], refs[1][:batch], per_instance=True)
    return s


def _opts(capi, full_first=False, **kw):
    o = capi.default_opts(**kw)
    if full_first:
        o.reserved[0] |= capi.OPT_FULL_FIRST_PRODUCT
    return o


def _run(s, o=None):
    s.calculate(o)
    return s.get_results()


def _step(capi, c, p, X0, env, monkeypatch, opts=None, **kw):
    """one cold step on a fresh handle made under the switches `env`"""
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        s = _solver(capi, c, p, len(X0), **kw)
    s.update_initialization(X0)
    r = _run(s, opts)
    s.close()
    return r


def _same(a, b, what, keys=KEYS, rows=None):
    for k in keys:
        x, y = np.ascontiguousarray(a[k] if rows is None else a[k][:rows]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


def _routes(c):
    """(name, switches) of the routes a case runs with the finish on: the default one, and the tile route where the default is the
    one-wave step"""
    out = [(c.route, {})]
    if c.route == "wave":
        out.append((c.tile_route, NO_WAVE))
    return out


def _residual(p, r, who):
    """the dynamics residual of the device's own e_x and e_u in long double, relative to its bound 1e-9 max(1, |e_x|)"""
    A, B = p.A.astype(np.longdouble), p.B.astype(np.longdouble)
    ex, eu = r["e_x"].astype(np.longdouble), r["e_u"].astype(np.longdouble)
    res = float(np.abs(np.einsum("ij,bjk->bik", A, ex[:, :, :-1]) + np.einsum("ij,bjk->bik", B, eu) - ex[:, :, 1:]).max())
    bound = 1e-9 * max(1.0, float(np.abs(r["e_x"]).max()))
    _note("residual", who, res, bound)
    return res, bound


def _check_outputs(p, X0, r, who, refs=None):
    """what every step promises of its outputs, whatever produced the inputs: u inside the box, e_u = u - u_ref, e_x = x - x_ref,
    x[:, :, 0] = x0, and the deviation dynamics"""
    b = len(X0)
    xr = p.x_ref[None] if refs is None else refs[0][:b]
    ur = p.u_ref[None] if refs is None else refs[1][:b]
    assert np.isfinite(r["u"]).all() and np.isfinite(r["x"]).all(), who
    assert np.all(r["u"] <= p.u_max[None, :, None]) and np.all(r["u"] >= p.u_min[None, :, None]), who
    assert np.abs(r["e_u"] - (r["u"] - ur)).max() <= 1e-14, who
    assert np.abs(r["e_x"] - (r["x"] - xr)).max() <= 1e-12, who
    assert np.array_equal(r["x"][:, :, 0], X0), who
    res, bound = _residual(p, r, who)
    assert res <= bound, (who, res, bound)


def _check_exact(c, ref, r, who, which=None):
    err_u = err_x = 0.0
    for i in (c.exact if which is None else which):
        if i >= len(r["u"]):
            continue
        e = ref["exact"][i]
        err_u = max(err_u, float(np.abs(r["u"][i] - e["u"]).max()))
        err_x = max(err_x, float(np.abs(r["x"][i] - e["x"]).max()))
    _note("exact-u", who, err_u, U_TOL)
    _note("exact-x", who, err_x, 10 * X_TOL)
    assert err_u <= U_TOL and err_x <= 10 * X_TOL, (who, err_u, err_x)


# ---------------------------------------------------------------------------- a. the iterate of every k_admm build, finish off
@pytest.mark.parametrize("profile,rho", PROFILES)
@pytest.mark.parametrize("case", cc.CASES, ids=_ids)
def test_iterates_match_the_oracle(capi, mo, co, case, profile, rho):
    """k_admm<NRB, KS> with the finish off: iterates, iteration counts and status of the oracle after 1, 2 and 7 iterations, with and
    without relaxation, on both penalty profiles, from the affine first iterate and from the full first product.  The two shapes at
    the kr >= n + 9 boundary also say which form ran (the forms differ in the last bits, the same form twice does not)."""
    ref = cc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    des = mo.design_shared(p, rho=rho, rho_profile=profile)
    s = _solver(capi, case, p, rho=rho, profile=profile)
    s.update_initialization(X0)
    worst = 0.0
    for max_iter, check_every in ITERATE_OPTS:
        for alpha in (1.0, None):
            kw = dict(max_iter=max_iter, check_every=check_every, **({} if alpha is None else dict(alpha=alpha)))
            a = _run(s, _opts(capi, rho=rho, polish=0, **kw))
            f = _run(s, _opts(capi, full_first=True, rho=rho, polish=0, **kw))
            o = co.step_batch(p, des, X0, polish=False, **kw)
            what = (case.id, profile, max_iter, check_every, alpha)
            for r in (a, f):
                assert np.array_equal(r["iters"], o["iters"]) and np.array_equal(r["status"], o["status"]), what
                assert np.all(r["polish_iters"] == 0), what
                worst = max(worst, float(np.abs(r["u"] - o["u"]).max()))
                assert np.abs(r["u"] - o["u"]).max() <= IT_TOL, what
            if max_iter == 7 and "affine" in case.tags:
                assert not np.array_equal(a["u"], f["u"]), "the affine form did not run"
            if "full_first" in case.tags:
                assert np.array_equal(a["u"], f["u"]), "no room behind W: both runs take the full product"
    if "separate" in case.tags:     # the separate rollout behind the iterate: k_rollout<4> / <1>
        _check_outputs(p, X0, a, case.id + " nopolish " + profile)
    s.close()
    _note("iterate", "k_admm<%d,%d> %s %s" % (case.build + (case.id, profile)), worst, IT_TOL)


# ---------------------------------------------------------------------------- b. warm start of every k_admm build
@pytest.mark.parametrize("profile,rho", PROFILES)
@pytest.mark.parametrize("case", cc.CASES, ids=_ids)
def test_warm_start_continues_the_oracles_iteration(capi, mo, case, profile, rho):
    """a cold step that keeps its state, then a warm one from 0.9 x0 (px = H'x streamed in groups of eight fragments for every KS):
    the oracle's iteration chained the same way, from the (x, z, y) of its own cold run"""
    ref = cc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    des = mo.design_shared(p, rho=rho, rho_profile=profile)
    s = _solver(capi, case, p, rho=rho, profile=profile)
    worst = 0.0
    for kw in (dict(max_iter=7, check_every=7), dict(max_iter=3, check_every=1, alpha=1.0)):
        s.update_initialization(X0)
        cold = _run(s, _opts(capi, rho=rho, polish=0, **kw))
        s.update_initialization(0.9 * X0)
        warm = _run(s, _opts(capi, rho=rho, polish=0, warm_start=1, **kw))
        for i in range(cc.BATCH):
            c0 = cc.admm(des, cc.fs_of(p, des, X0[i]), **kw)
            c1 = cc.admm(des, cc.fs_of(p, des, 0.9 * X0[i]), c0["x"], c0["z"], c0["y"], **kw)
            for r, o in ((cold, c0), (warm, c1)):
                assert r["iters"][i] == o["iters"] and r["status"][i] == o["status"], (case.id, i, kw)
                err = float(np.abs(r["u"][i] - cc.admm_u(p, des, o)).max())
                worst = max(worst, err)
                assert err <= IT_TOL, (case.id, i, kw, err)
        assert np.abs(warm["u"] - cold["u"]).max() > 0.0
    s.close()
    _note("warm", "k_admm<%d,%d> %s %s" % (case.build + (case.id, profile)), worst, IT_TOL)


# ---------------------------------------------------------------------------- c. instances of one tile stop at different checks
@pytest.mark.parametrize("case", cc.tagged("freeze"), ids=_ids)
def test_instances_freeze_at_the_oracles_check(capi, mo, co, case):
    """amplitudes 0.01 and 3 alternate within each tile of a multi-wave build, 200 iterations with a check every 5: every instance
    stops at the oracle's check while its neighbours go on (tests/test_condensed_step_cases.py: no residual of any check lies within
    1e-6 of its threshold, so the counts are asked for without an allowance)"""
    p = cc.problem(case)
    X0 = cc.freeze_x0(case)
    des = mo.design_shared(p)
    s = _solver(capi, case, p)
    s.update_initialization(X0)
    r = _run(s, _opts(capi, polish=0, **cc.FREEZE_OPTS))
    s.close()
    o = co.step_batch(p, des, X0, polish=False, **cc.FREEZE_OPTS)
    print("condensed-step freeze", case.id, r["iters"].tolist(), "max |u - u_oracle| %.3e" % np.abs(r["u"] - o["u"]).max())
    assert np.array_equal(r["iters"], o["iters"]) and np.array_equal(r["status"], o["status"])
    assert np.all(r["status"] == 0)
    assert len(set(r["iters"][:cc.TILE].tolist())) >= 2


# ---------------------------------------------------------------------------- d. finish on, on the route the table names
@pytest.mark.parametrize("case", cc.CASES, ids=_ids)
def test_finish_on_every_route(capi, case, monkeypatch):
    """one cold step with default options on the route the table names (the shapes of the one-wave step also on the tile kernels):
    every instance solved by the condensed step itself, every third one against the exact oracle (the heavy cases: every one), the
    outputs' promises, and the two routes of a small shape against each other"""
    ref = cc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    out = {}
    for route, env in _routes(case):
        who = "%s %s" % (case.id, route)
        r = out[route] = _step(capi, case, p, X0, env, monkeypatch)
        assert np.all(r["status"] == 0), (who, np.nonzero(r["status"])[0].tolist())
        _check_outputs(p, X0, r, who)
        _check_exact(case, ref, r, who)
    if len(out) == 2:   # the one-wave step against the tile kernels
        w, t = out["wave"], out[case.tile_route]
        assert np.array_equal(w["iters"], t["iters"]) and np.array_equal(w["status"], t["status"])
        assert np.abs(w["u"] - t["u"]).max() <= 1e-9 and np.abs(w["x"] - t["x"]).max() <= 1e-8
    if case.heavy:      # the inputs do reach the second tier
        lo_band, hi_band = cc.HEAVY_BANDS[case.id]
        na = ref["nact"]
        assert ((na >= 33) & (na <= 48)).any() == lo_band and ((na >= 49) & (na <= 60)).any() == hi_band


@pytest.mark.parametrize("case", [c for c in cc.CASES if c.xref_glb], ids=_ids)
def test_finish_with_per_instance_references(capi, case, monkeypatch):
    """the blocked rollout reads x_ref from global memory (xref_glb), the tile kernels take the per-row loads and the full first product"""
    ref = cc.reference_glb(case)
    p, X0, refs = ref["p"], ref["X0"], ref["refs"]
    for route, env in _routes(case):
        who = "%s %s per-instance references" % (case.id, route)
        r = _step(capi, case, p, X0, env, monkeypatch, refs=refs)
        assert np.all(r["status"] == 0), who
        _check_outputs(p, X0, r, who, refs=refs)
        _check_exact(case, ref, r, who)


@pytest.mark.parametrize("case", cc.tagged("separate"), ids=_ids)
def test_separate_rollout_behind_the_finish(capi, case, monkeypatch):
    """k_rollout<4> / <1> behind k_polish (its inputs come from dW) and behind k_admm alone (from the iterate): the same outputs'
    promises; (64, 2, 60) asks for more than the 64 KiB of LDS a kernel has by default"""
    assert case.rollout[0] in ("separate4", "separate1") and cc.rollout_kind(*case.shape, polish=False) == case.rollout
    ref = cc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    on = _step(capi, case, p, X0, {}, monkeypatch)
    off = _step(capi, case, p, X0, {}, monkeypatch, opts=_opts(capi, polish=0))
    _check_outputs(p, X0, on, case.id + " " + case.rollout[0])
    _check_outputs(p, X0, off, case.id + " nopolish " + case.rollout[0])
    assert np.all(on["status"] == 0) and np.all(off["polish_iters"] == 0)
    _check_exact(case, ref, on, case.id + " " + case.rollout[0])


# ---------------------------------------------------------------------------- e. route pairs
@pytest.mark.parametrize("case", cc.tagged("unfused"), ids=_ids)
def test_one_kernel_step_equals_the_two_kernel_path(capi, case):
    """k_step_fused<8, 30 | 32> and k_admm + k_polish<true> run the same device functions: bit for bit, cold and warm"""
    assert case.route == "fused" and cc.pick_route(*case.shape, fuse_step=False) == "tile"
    ref = cc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    s = _solver(capi, case, p)
    out = {}
    for fused in (True, False):
        s.set_step_fusion(fused)
        s.update_initialization(X0)
        cold = _run(s)
        s.update_initialization(0.9 * X0)
        out[fused] = (cold, _run(s, _opts(capi, warm_start=1)))
    s.close()
    for k, name in enumerate(("cold", "warm")):
        _same(out[True][k], out[False][k], (case.id, name))
        assert np.all(out[True][k]["status"] == 0)
    _check_exact(case, ref, out[False][0], case.id + " tile (fusion off)")


@pytest.mark.parametrize("case", cc.tagged("no_glds"), ids=_ids)
def test_finish_through_l2_matches_the_finish_with_g_in_lds(capi, case, monkeypatch):
    """ALMPC_POLISH_NO_GLDS=1 (k_polish<false>) against the default (k_polish<true>, at nz 113 the one-kernel step)"""
    ref = cc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    env = NO_WAVE if case.route == "wave" else {}
    assert pick(case, env) in ("tile", "fused") and pick(case, dict(env, ALMPC_POLISH_NO_GLDS="1")) == "tile_l2"
    a = _step(capi, case, p, X0, env, monkeypatch)
    b = _step(capi, case, p, X0, dict(env, ALMPC_POLISH_NO_GLDS="1"), monkeypatch)
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["polish_iters"], b["polish_iters"])
    assert np.array_equal(a["iters"], b["iters"])
    _note("l2-vs-lds-u", case.id, float(np.abs(a["u"] - b["u"]).max()), 1e-12)
    assert np.abs(a["u"] - b["u"]).max() <= 1e-12 and np.abs(a["x"] - b["x"]).max() <= 1e-10
    assert np.all(b["status"] == 0)
    _check_outputs(p, X0, b, case.id + " tile_l2")
    _check_exact(case, ref, b, case.id + " tile_l2")


def pick(case, env):
    return cc.pick_route(*case.shape, no_shared_wave="ALMPC_NO_SHARED_WAVE" in env, no_glds="ALMPC_POLISH_NO_GLDS" in env,
                         stagewise="ALMPC_ROLLOUT_STAGEWISE" in env, sg_global="ALMPC_POLISH_SG_GLOBAL" in env)


@pytest.mark.parametrize("case", cc.tagged("stagewise"), ids=_ids)
def test_blocked_rollout_against_the_stage_by_stage_one(capi, case, monkeypatch):
    """ALMPC_ROLLOUT_STAGEWISE=1 changes the rollout only: u, e_u, status and the iteration counts bit for bit, x of both runs held to
    the dynamics and to the oracle.  Both runs on the tile kernels (without the blocked rollout n = 16 has no rollout in the finish's
    tail and with it no one-wave step); where both take the one-wave step, on that as well."""
    assert case.block[0] > 0 and cc.roll_block(*case.shape, stagewise=True) == (0, 0)
    ref = cc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    envs = [NO_WAVE] if case.route == "wave" else [{}]
    if case.route == "wave" and pick(case, {"ALMPC_ROLLOUT_STAGEWISE": "1"}) == "wave":
        envs.append({})
    for env in envs:
        who = "%s %s" % (case.id, pick(case, env))
        a = _step(capi, case, p, X0, env, monkeypatch)
        b = _step(capi, case, p, X0, dict(env, ALMPC_ROLLOUT_STAGEWISE="1"), monkeypatch)
        _same(a, b, who, keys=("u", "e_u", "status", "iters", "polish_iters"))
        assert np.all(a["status"] == 0)
        _note("blocked-vs-stagewise-x", who, float(np.abs(a["x"] - b["x"]).max()))
        for r, name in ((a, " blocked"), (b, " stage by stage")):
            _check_outputs(p, X0, r, who + name)
            _check_exact(case, ref, r, who + name)


@pytest.mark.parametrize("case", cc.tagged("sg_global"), ids=_ids)
def test_second_tier_in_the_global_scratch_equals_the_lds_slot(capi, case, monkeypatch):
    """ALMPC_POLISH_SG_GLOBAL=1: the same arithmetic in another home -- bit for bit, every instance solved and every one against the
    exact oracle.  Working sets of 33..48 rows take the LDS slot where the layout has one, 49..60 the global scratch in any case."""
    ref = cc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    lo_band, hi_band = cc.HEAVY_BANDS[case.id]
    na = ref["nact"]
    assert ((na >= 33) & (na <= 48)).any() == lo_band and ((na >= 49) & (na <= 60)).any() == hi_band and lo_band
    assert sorted(ref["exact"]) == list(range(cc.BATCH))
    env = NO_WAVE if case.route == "wave" else {}
    assert pick(case, env) == pick(case, dict(env, ALMPC_POLISH_SG_GLOBAL="1")) == "tile"
    a = _step(capi, case, p, X0, env, monkeypatch)
    b = _step(capi, case, p, X0, dict(env, ALMPC_POLISH_SG_GLOBAL="1"), monkeypatch)
    _same(a, b, case.id)
    for r, name in ((a, " slot" if case.slot else " no slot"), (b, " global scratch")):
        assert np.all(r["status"] == 0), (case.id, name, np.nonzero(r["status"])[0].tolist())
        _check_exact(case, ref, r, case.id + name)
    act = np.array([cc.active_rows(p, a["u"][i]) for i in range(cc.BATCH)])
    assert np.array_equal(act, na), "the device's working sets are the exact solution's"


# ---------------------------------------------------------------------------- f. batches
@pytest.mark.parametrize("case", [c for c in cc.CASES if len(c.batches) > 1], ids=_ids)
def test_smaller_batches_are_the_first_rows(capi, case, monkeypatch):
    """batch 16 (one full tile) and 1 against the batch of 37 on the same route: an instance's result does not depend on its tile"""
    ref = cc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    for route, env in _routes(case):
        full = _step(capi, case, p, X0, env, monkeypatch)
        for b in case.batches[1:]:
            assert cc.pick_route(*case.shape, batch=b, no_shared_wave=bool(env)) == route
            _same(full, _step(capi, case, p, X0[:b], env, monkeypatch), (case.id, route, b), rows=b)
