"""The per-instance design and step (almpc_design_batched -> almpc_calculate on a condensed handle) at every build and route: the
cases of tests/instance_step_cases.py against the oracles.  Run on an MI355X: pytest -m gpu.

Every handle is created with structured_fallback=False: the verdict is the condensed step's own, an instance its finish leaves
without a certificate stays at status 1 and no stage-wise solver runs.  The switches (ALMPC_*) are read by almpc_create: they are set
before the handle is made.  Tolerances are the project's: IT_TOL max(1, |v|) on ADMM iterates
(test_admm_iterate_matches_oracle_per_instance), U_TOL and 10 X_TOL against the exact oracle
(tests/test_gpu_condensed_step_shapes.py), 1e-9 / 1e-8 between two routes to the same optimum
(test_wave_per_instance_step_equals_the_two_launch_path), 1e-11 max|H| on H and F and 1e-12 on d
(test_design_batched_matches_oracle), the dynamics residual in long double with the instance's own model, and bit for bit where the
same device functions run on the same values.

Lines that start with `instance-step` print the measured maxima (pytest -s)."""
import functools

import numpy as np
import pytest

import condensed_step_cases as cc
import instance_step_cases as ic

pytestmark = pytest.mark.gpu

IT_TOL = 1e-9
U_TOL = 1e-6
X_TOL = 1e-5
KEYS = ("u", "e_u", "x", "e_x", "status", "iters", "polish_iters")
ITERATE_OPTS = [(1, 1), (2, 1), (7, 7)]
ALPHAS = (1.0, None)
WARM_OPTS = (dict(max_iter=7, check_every=7), dict(max_iter=3, check_every=1, alpha=1.0))
SPLIT_SCALE = {"ALMPC_DBG_SPLIT_SCALE": "1"}
_ids = lambda c: c.id


def _note(what, key, value, bound=None):
    print("instance-step %s %s %.3e%s" % (what, key, value, "" if bound is None else " of %.1e" % bound))


def _solver(capi, c, env, monkeypatch, batch=None, rho=0.1, profile="scalar"):
    """a designed handle of the first `batch` instances, made under the switches `env`"""
    b = c.batch if batch is None else batch
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        s = capi.Solver(c.n, c.m, c.N, b, structured_fallback=False)
    A, B = ic.models(c)
    t = ic.template(c)
    s.design_batched(A[:b], B[:b], t.Q, t.R, t.S, t.P, t.u_min, t.u_max, rho=rho, rho_profile=profile)
    s.set_reference(t.x_ref, t.u_ref)
    return s


def _run(s, X0=None, o=None):
    if X0 is not None:
        s.update_initialization(X0)
    s.calculate(o)
    return s.get_results()


def _step(capi, c, env, monkeypatch, X0, opts=None, **kw):
    s = _solver(capi, c, env, monkeypatch, batch=len(X0), **kw)
    r = _run(s, X0, opts)
    s.close()
    return r


def _same(a, b, what, keys=KEYS, rows=None):
    for k in keys:
        x, y = np.ascontiguousarray(a[k] if rows is None else a[k][:rows]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


def _check_outputs(c, X0, r, who):
    """what every step promises of its outputs: u inside the box, e_u = u - u_ref, e_x = x - x_ref, x[:, :, 0] = x0, and the
    deviation dynamics through the instance's OWN (A_i, B_i), the residual evaluated in long double"""
    t = ic.template(c)
    b = len(X0)
    A, B = (M[:b].astype(np.longdouble) for M in ic.models(c))
    assert np.isfinite(r["u"]).all() and np.isfinite(r["x"]).all(), who
    assert np.all(r["u"] <= t.u_max[None, :, None]) and np.all(r["u"] >= t.u_min[None, :, None]), who
    assert np.abs(r["e_u"] - (r["u"] - t.u_ref[None])).max() <= 1e-14, who
    assert np.abs(r["e_x"] - (r["x"] - t.x_ref[None])).max() <= 1e-12, who
    assert np.array_equal(r["x"][:, :, 0], X0), who
    ex, eu = r["e_x"].astype(np.longdouble), r["e_u"].astype(np.longdouble)
    res = float(np.abs(np.einsum("bij,bjk->bik", A, ex[:, :, :-1]) + np.einsum("bij,bjk->bik", B, eu) - ex[:, :, 1:]).max())
    bound = 1e-9 * max(1.0, float(np.abs(r["e_x"]).max()))
    _note("residual", who, res, bound)
    assert res <= bound, (who, res, bound)


def _check_exact(c, r, who):
    ref = ic.reference(c)
    err_u = err_x = 0.0
    for i in c.exact:
        if i >= len(r["u"]):
            continue
        e = ref["exact"][i]
        err_u = max(err_u, float(np.abs(r["u"][i] - e["u"]).max()))
        err_x = max(err_x, float(np.abs(r["x"][i] - e["x"]).max()))
    _note("exact-u", who, err_u, U_TOL)
    _note("exact-x", who, err_x, 10 * X_TOL)
    assert err_u <= U_TOL and err_x <= 10 * X_TOL, (who, err_u, err_x)


def _kernels(c, env, profile="scalar", polish=True):
    return " ".join("%s<%s>" % (k[0], k[1]) for k in ic.step_kernels(*c.shape, c.batch, profile, polish, env))


def _inverses(c, env, profile):
    f = ic.factor_plan(*c.shape, c.batch, profile, env)
    return " ".join(sorted({"inverse_%s<%s>" % (b[0], ",".join(str(v) for v in b[1:])) for b in f["inverses"]})) + \
        (" neg_gm<%d>" % f["neg_gm"] if f["neg_gm"] is not None else "") + (" design_rho" if f["rho_kernel"] else "") + \
        (" one-launch" if f["one_launch"] else "")


def _opt_kw(max_iter, check_every, alpha):
    return dict(max_iter=max_iter, check_every=check_every, **({} if alpha is None else dict(alpha=alpha)))


# ---------------------------------------------------------------------------- the oracle's iterates, once per case and profile
@functools.lru_cache(maxsize=None)
def _iterates(c, profile, rho):
    """{(max_iter, check_every, alpha): (u (batch, m, N), iters, status)} of cc.admm on mo.design_shared of every instance's problem"""
    X0 = ic.x0(c)
    des = ic.designs(c, profile, rho)
    out = {}
    for max_iter, check_every in ITERATE_OPTS:
        for alpha in ALPHAS:
            u, it, st = np.empty((c.batch, c.m, c.N)), np.empty(c.batch, dtype=np.int32), np.empty(c.batch, dtype=np.int32)
            for i in range(c.batch):
                p = ic.problem(c, i)
                o = cc.admm(des[i], cc.fs_of(p, des[i], X0[i]), **_opt_kw(max_iter, check_every, alpha))
                u[i], it[i], st[i] = cc.admm_u(p, des[i], o), o["iters"], o["status"]
            out[(max_iter, check_every, alpha)] = (u, it, st)
    return out


# ---------------------------------------------------------------------------- a. the design's outputs
@pytest.mark.parametrize("case", ic.CASES, ids=_ids)
def test_design_outputs_match_the_oracle(capi, mo, case, monkeypatch):
    """H_i, F_i and d_i of every instance against mo.condense / mo.jacobi_scaling of its own problem: by k_design_instance_t<NC, MC>
    with the scaling in its tail and by k_design_scale behind it (bit for bit the same), or on the dense route"""
    envs = [{}] + ([SPLIT_SCALE] if ic.scale_in_tail(*case.shape) else [])
    got = []
    for env in envs:
        s = _solver(capi, case, env, monkeypatch)
        got.append([s.get_design_instance(i) for i in range(case.batch)])
        s.close()
        eh = ef = ed = 0.0
        for i, (H, F, _) in enumerate(ic.condensed(case)):
            g = got[-1][i]
            d = mo.jacobi_scaling(H)
            eh = max(eh, float(np.abs(g["H"] - H).max() / np.abs(H).max()))
            ef = max(ef, float(np.abs(g["F"] - F).max() / np.abs(F).max()))
            ed = max(ed, float(np.abs(g["d"] - d).max() / np.abs(g["d"]).max()))
        who = "%s %s %s scaling %s" % (case.id, ic.design_route(*case.shape), "design_instance<%d,%d>" % ic.design_build(case.n, case.m)
                                       if ic.design_route(*case.shape) == "lds" else "blocks+gamma+hessian",
                                       "in the tail" if ic.scale_in_tail(*case.shape, env) else "by k_design_scale")
        _note("design-H", who, eh, 1e-11)
        _note("design-F", who, ef, 1e-11)
        _note("design-d", who, ed, 1e-12)
        assert eh <= 1e-11 and ef <= 1e-11 and ed <= 1e-12, (who, eh, ef, ed)
    if len(got) == 2:
        for a, b in zip(*got):
            assert all(np.array_equal(a[k], b[k]) for k in ("H", "F", "d"))


# ---------------------------------------------------------------------------- b. iterates, finish off
@pytest.mark.parametrize("profile,rho", ic.PROFILES)
@pytest.mark.parametrize("case", ic.CASES, ids=_ids)
def test_iterates_match_the_oracle(capi, case, profile, rho, monkeypatch):
    """k_admm_inst<PACKED> behind every inverse build the table names for the case, finish off: u, iteration counts and status of
    every instance after 1, 2 and 7 iterations, with and without relaxation -- this is what sees Minv_i, rho_i, F'_i, d_i and the
    packed layout; behind it k_rollout<1> with strides (x through the instance's own model)"""
    X0 = ic.x0(case)
    ref = _iterates(case, profile, rho)
    for env in [{}] + case.design_envs():
        s = _solver(capi, case, env, monkeypatch, rho=rho, profile=profile)
        s.update_initialization(X0)
        worst = 0.0
        for (max_iter, check_every, alpha), (u, it, st) in ref.items():
            r = _run(s, o=capi.default_opts(rho=rho, polish=0, **_opt_kw(max_iter, check_every, alpha)))
            what = (case.id, ic._env_id(env), profile, max_iter, check_every, alpha)
            assert np.array_equal(r["iters"], it) and np.array_equal(r["status"], st), what
            assert np.all(r["polish_iters"] == 0), what
            t = ic.template(case)
            err = float((np.abs(r["u"] - u) / np.maximum(1.0, np.abs(u - t.u_ref[None]).max(axis=(1, 2), keepdims=True))).max())
            worst = max(worst, err)
            assert err <= IT_TOL, what + (err,)
        who = "%s %s %s: %s %s" % (case.id, ic._env_id(env), profile, _kernels(case, env, profile, False), _inverses(case, env, profile))
        _check_outputs(case, X0, r, who)
        s.close()
        _note("iterate", who, worst, IT_TOL)


# ---------------------------------------------------------------------------- c. warm start
@pytest.mark.parametrize("profile,rho", ic.PROFILES)
@pytest.mark.parametrize("case", ic.CASES, ids=_ids)
def test_warm_start_continues_the_oracles_iteration(capi, case, profile, rho, monkeypatch):
    """k_admm_inst packed and full: a cold step that keeps its state, then a warm one from 0.9 x0, against the oracle's iteration
    chained the same way from the (x, z, y) of its own cold run"""
    X0 = ic.x0(case)
    des = ic.designs(case, profile, rho)
    t = ic.template(case)
    s = _solver(capi, case, {}, monkeypatch, rho=rho, profile=profile)
    worst = 0.0
    for kw in WARM_OPTS:
        cold = _run(s, X0, capi.default_opts(rho=rho, polish=0, **kw))
        warm = _run(s, 0.9 * X0, capi.default_opts(rho=rho, polish=0, warm_start=1, **kw))
        for i in range(case.batch):
            p = ic.problem(case, i)
            c0 = cc.admm(des[i], cc.fs_of(p, des[i], X0[i]), **kw)
            c1 = cc.admm(des[i], cc.fs_of(p, des[i], 0.9 * X0[i]), c0["x"], c0["z"], c0["y"], **kw)
            for r, o in ((cold, c0), (warm, c1)):
                assert r["iters"][i] == o["iters"] and r["status"][i] == o["status"], (case.id, i, kw)
                u = cc.admm_u(p, des[i], o)
                err = float(np.abs(r["u"][i] - u).max() / max(1.0, np.abs(u - t.u_ref).max()))
                worst = max(worst, err)
                assert err <= IT_TOL, (case.id, i, kw, err)
        assert np.abs(warm["u"] - cold["u"]).max() > 0.0
    s.close()
    _note("warm", "%s %s %s" % (case.id, profile, _kernels(case, {}, profile, False)), worst, IT_TOL)


@pytest.mark.parametrize("case", [c for c in ic.CASES if c.route == "wave"], ids=_ids)
def test_warm_one_wave_step_equals_the_two_launch_path(capi, case, monkeypatch):
    """k_step_inst_wave<NZC> keeps and takes up the ADMM state as k_admm_inst does: a cold step, then a warm one from 0.9 x0, finish
    on, on both routes -- equal status and iteration counts, the same optimum"""
    X0 = ic.x0(case)
    out = {}
    for env in ({}, ic.NO_WAVE):
        s = _solver(capi, case, env, monkeypatch)
        cold = _run(s, X0)
        out[ic._env_id(env)] = (cold, _run(s, 0.9 * X0, capi.default_opts(warm_start=1)))
        s.close()
    for k, name in enumerate(("cold", "warm")):
        w, t = out["default"][k], out[ic._env_id(ic.NO_WAVE)][k]
        who = "%s %s %s | %s" % (case.id, name, _kernels(case, {}), _kernels(case, ic.NO_WAVE))
        assert np.array_equal(w["iters"], t["iters"]) and np.array_equal(w["status"], t["status"]), who
        assert np.array_equal(w["polish_iters"], t["polish_iters"]), who
        assert np.all(w["status"] == 0), (who, np.nonzero(w["status"])[0].tolist())
        du, dx = float(np.abs(w["u"] - t["u"]).max()), float(np.abs(w["x"] - t["x"]).max())
        _note("wave-vs-two-u", who, du, 1e-9)
        assert du <= 1e-9 and dx <= 1e-8, (who, du, dx)
        _check_outputs(case, X0 if k == 0 else 0.9 * X0, w, who)


# ---------------------------------------------------------------------------- d. instances stop at different checks
@pytest.mark.parametrize("case", ic.tagged("freeze"), ids=_ids)
def test_instances_freeze_at_the_oracles_check(capi, case, monkeypatch):
    """amplitudes 0.01 and 3 alternate over the instances, 200 iterations with a check every 5: every instance stops at the oracle's
    check while its neighbours in the persistent grid of k_admm_inst go on (at batch 515: in the second round as well), and in the
    one-wave step (tests/test_instance_step_cases.py: no residual of any check lies within 1e-6 of its threshold)"""
    X0 = ic.freeze_x0(case)
    des = ic.designs(case, *ic.PROFILES[0])
    it = np.empty(case.batch, dtype=np.int32)
    u = np.empty((case.batch, case.m, case.N))
    for i in range(case.batch):
        p = ic.problem(case, i)
        o = cc.admm(des[i], cc.fs_of(p, des[i], X0[i]), **ic.FREEZE_OPTS)
        assert o["status"] == 0
        it[i], u[i] = o["iters"], cc.admm_u(p, des[i], o)
    r = _step(capi, case, {}, monkeypatch, X0, capi.default_opts(polish=0, **ic.FREEZE_OPTS))
    print("instance-step freeze", case.id, _kernels(case, {}, polish=False), sorted(set(r["iters"].tolist())), "max |u - u_oracle| %.3e" % np.abs(r["u"] - u).max())
    assert np.array_equal(r["iters"], it) and np.all(r["status"] == 0)
    assert len(set(it.tolist())) >= 2
    if case.route == "wave":    # the same counts from the one-wave step (the finish runs behind them)
        w = _step(capi, case, {}, monkeypatch, X0, capi.default_opts(**ic.FREEZE_OPTS))
        assert np.array_equal(w["iters"], it) and np.all(w["status"] == 0), _kernels(case, {})


# ---------------------------------------------------------------------------- e. finish on, on every route
@pytest.mark.parametrize("case", ic.CASES, ids=_ids)
def test_finish_on_every_route(capi, case, monkeypatch):
    """one cold step with default options on every route the table names: every instance solved by the condensed step itself, the
    compared ones against the exact oracle of their own problem, the outputs' promises, and the routes against each other"""
    X0 = ic.x0(case)
    out = {}
    for env in case.step_envs():
        who = "%s %s: %s" % (case.id, ic._env_id(env), _kernels(case, env))
        r = out[ic._env_id(env)] = _step(capi, case, env, monkeypatch, X0)
        assert np.all(r["status"] == 0), (who, np.nonzero(r["status"])[0].tolist())
        _check_outputs(case, X0, r, who)
        _check_exact(case, r, who)
    first = out.pop("default")
    for name, r in out.items():     # one-wave against two-launch, k_polish_sgl<0> against k_polish<false>
        assert np.array_equal(first["iters"], r["iters"]) and np.array_equal(first["status"], r["status"]), (case.id, name)
        du, dx = float(np.abs(first["u"] - r["u"]).max()), float(np.abs(first["x"] - r["x"]).max())
        _note("route-pair-u", "%s default | %s" % (case.id, name), du, 1e-9)
        assert du <= 1e-9 and dx <= 1e-8, (case.id, name, du, dx)
    if case.heavy:                  # the inputs do reach the second tier
        na = ic.active_counts(case)
        assert (((na >= 33) & (na <= 48)).any(), ((na >= 49) & (na <= 60)).any()) == ic.HEAVY_BANDS[case.id] and na.max() <= 60
        act = np.array([cc.active_rows(ic.template(case), first["u"][i]) for i in range(case.batch)])
        assert np.array_equal(act, na), "the device's working sets are the exact solution's"


# ---------------------------------------------------------------------------- f. inverse builds and split launches against the default
@pytest.mark.parametrize("profile,rho", ic.PROFILES)
@pytest.mark.parametrize("case", [c for c in ic.CASES if c.design_envs()], ids=_ids)
def test_design_switches_against_the_default(capi, case, profile, rho, monkeypatch):
    """ALMPC_INV_TILE, ALMPC_INV_CW, ALMPC_NO_RHO_FUSION, ALMPC_NO_PACKED_MINV and the ALMPC_DBG_SPLIT_* trio: d, H, F bit for bit
    the default's, the same status and iteration counts of ADMM and finish, and each within tolerance of the exact oracle on its own
    (its iterates: test_iterates_match_the_oracle)"""
    X0 = ic.x0(case)
    res = {}
    for env in [{}] + case.design_envs():
        s = _solver(capi, case, env, monkeypatch, rho=rho, profile=profile)
        r = _run(s, X0, capi.default_opts(rho=rho))
        res[ic._env_id(env)] = (r, [s.get_design_instance(i) for i in case.exact])
        s.close()
        who = "%s %s %s: %s %s" % (case.id, ic._env_id(env), profile, _kernels(case, env, profile), _inverses(case, env, profile))
        assert np.all(r["status"] == 0), (who, np.nonzero(r["status"])[0].tolist())
        _check_outputs(case, X0, r, who)
        _check_exact(case, r, who)
    r0, d0 = res.pop("default")
    for name, (r, d) in res.items():
        for a, b in zip(d0, d):
            assert all(np.array_equal(a[k], b[k]) for k in ("d", "H", "F")), (case.id, name)
        for k in ("status", "iters", "polish_iters"):
            assert np.array_equal(r0[k], r[k]), (case.id, name, profile, k)
        _note("switch-vs-default-u", "%s %s %s" % (case.id, name, profile), float(np.abs(r0["u"] - r["u"]).max()))


# ---------------------------------------------------------------------------- g. batches
@pytest.mark.parametrize("case", [c for c in ic.CASES if c.batches], ids=_ids)
def test_smaller_batches_are_the_first_rows(capi, case, monkeypatch):
    """batches 1, 3, 4 and 5 (k_design_inverse_wave packs four matrices, or the two inverses of two instances, per workgroup)
    against the batch of 37 on the same route, finish on and off: an instance's result does not depend on its neighbours"""
    X0 = ic.x0(case)
    for env in case.step_envs():
        for opts in (None, capi.default_opts(polish=0, max_iter=7, check_every=7)):
            full = _step(capi, case, env, monkeypatch, X0, opts)
            for b in case.batches:
                _same(full, _step(capi, case, env, monkeypatch, X0[:b], opts), (case.id, ic._env_id(env), b), rows=b)
