"""The places of the cold step's critical path that carry values through LDS: the row-constant table and the |f/d| partials of the
ADMM prologue, the pair-packed fragments of the KKT inverse, and the row-index look-ahead of the finish's G[W,:] sweeps (the same
inputs take the register Gauss-Jordan of the guessed set through guesses of every size).  None of them changes a floating-point
operation, so everything here is asked of the parent build as well.  Run on an MI355X: pytest -m gpu.

Bounds are those of tests/test_gpu_condensed_step_shapes.py for the same quantities: IT_TOL on iterates against the restatement,
U_TOL against the exact oracle, bit for bit between routes that run the same device functions.  The finish through L2
(k_polish<false>) is held to the finish with G in LDS bit for bit as well, as this change's specification asks ("u identical between
the three routes"), not to the 1e-12 of test_finish_through_l2_matches_the_finish_with_g_in_lds: on these inputs it is the guard that
the index look-ahead, which only the G-in-LDS builds have, leaves the sums alone -- both add the same products in the same ascending
order, 16 rows at a time or 8 (difference on the parent build: 0).  A change that reorders one of the two sweeps on purpose moves this
assertion to that bound.

Lines that start with `critical-path` print the measured maxima (pytest -s)."""
import functools

import numpy as np
import pytest

import bench
import condensed_step_cases as cc
import mpc_oracle as mo

pytestmark = pytest.mark.gpu

IT_TOL = 1e-9
U_TOL = 1e-6
PROFILES = [("scalar", 0.1), ("stiffness", 30.0)]
BATCH = cc.BATCH

# ---------------------------------------------------------------------------- finish: index look-ahead, guesses of every size
FINISH_AMPS = (1.0, 2.0, 3.0, 4.0, 6.0)
FINISH_K = (1, 2, 6)
FINISH_RHO = 45.0
# optimal active-set sizes that the inputs must reach: the chunks of 8 positions, the 16-column halves of the register inverse and
# the second tier (beyond 32 rows)
FINISH_BANDS = ((1, 8), (9, 16), (17, 24), (25, 32), (33, 48))


@functools.lru_cache(maxsize=None)
def finish_reference(amp):
    """dict(p, X0, exact {i: rollout dict}, nact) of the quadrotor batch of one amplitude; computed once, read-only"""
    p = mo.quadrotor()
    X0 = bench.make_x0(mo, 0, BATCH, amp)
    exact = cc.exact_batch(p, X0, range(BATCH))
    return dict(p=p, X0=X0, exact=exact, nact=np.array([cc.active_rows(p, exact[i]["u"]) for i in range(BATCH)]))


def _note(what, key, value, bound=None):
    print("critical-path %s %s %.3e%s" % (what, key, value, "" if bound is None else " of %.1e" % bound))


def _finish_solver(capi, p, env, monkeypatch):
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        s = capi.Solver(p.n, p.m, p.N, BATCH, structured_fallback=False)
    s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=FINISH_RHO, rho_profile="stiffness")
    s.set_reference(p.x_ref, p.u_ref)
    return s


def test_finish_inputs_cross_every_boundary():
    """the 185 instances' optimal active sets fall into every band (from the oracle alone)"""
    na = np.concatenate([finish_reference(a)["nact"] for a in FINISH_AMPS])
    for lo, hi in FINISH_BANDS:
        assert ((na >= lo) & (na <= hi)).any(), (lo, hi, sorted(set(na.tolist())))


@pytest.mark.parametrize("amp", FINISH_AMPS)
def test_finish_of_guesses_of_every_size(capi, amp, monkeypatch):
    """Stiffness rho 45, cold start, no redo, K = 1, 2 and 6 ADMM iterations (the guess shrinks and the adds grow as K falls), with
    and without the warm state: the one-kernel step, k_admm + k_polish<true> and k_admm + k_polish<false> (chunks of 16) certify every
    instance, reach the exact optimum and agree with each other."""
    ref = finish_reference(amp)
    p, X0 = ref["p"], ref["X0"]
    assert cc.pick_route(*cc.QUAD) == "fused" and cc.pick_route(*cc.QUAD, fuse_step=False) == "tile"
    assert cc.pick_route(*cc.QUAD, no_glds=True) == "tile_l2"
    fused = _finish_solver(capi, p, {}, monkeypatch)
    tile = _finish_solver(capi, p, {}, monkeypatch)
    tile.set_step_fusion(False)
    l2 = _finish_solver(capi, p, {"ALMPC_POLISH_NO_GLDS": "1"}, monkeypatch)
    worst_u = 0.0
    try:
        for K in FINISH_K:
            for keep in (True, False):
                out = {}
                for name, s in (("fused", fused), ("tile", tile), ("tile_l2", l2)):
                    s.update_initialization(X0)
                    s.calculate(capi.default_opts(rho=FINISH_RHO, max_iter=K, check_every=K, keep_warm_state=keep))
                    r = out[name] = s.get_results()
                    who = (amp, K, keep, name)
                    assert np.all(r["status"] == 0), (who, np.nonzero(r["status"])[0].tolist())
                    err = max(float(np.abs(r["u"][i] - ref["exact"][i]["u"]).max()) for i in range(BATCH))
                    worst_u = max(worst_u, err)
                    assert err <= U_TOL, (who, err)
                assert np.array_equal(out["fused"]["u"], out["tile"]["u"]), (amp, K, keep)
                assert np.array_equal(out["fused"]["polish_iters"], out["tile"]["polish_iters"]), (amp, K, keep)
                d = float(np.abs(out["tile"]["u"] - out["tile_l2"]["u"]).max())
                assert np.array_equal(out["tile"]["polish_iters"], out["tile_l2"]["polish_iters"]), (amp, K, keep)
                assert np.array_equal(out["tile"]["u"], out["tile_l2"]["u"]), (amp, K, keep, d)
    finally:
        for s in (fused, tile, l2):
            s.close()
    _note("finish exact-u", "amplitude %g" % amp, worst_u, U_TOL)


# ---------------------------------------------------------------------------- ADMM phase: table through LDS, |f/d| at the first check, pair-packed M^-1
ADMM_CASES = tuple(cc.CASE_BY_ID[i] for i in ("3-2-6", "6-1-41", "12-4-30", "11-11-11", "56-2-1"))
ADMM_BUILDS = {"3-2-6": (1, 3), "6-1-41": (3, 12), "12-4-30": (8, 30), "11-11-11": (8, 32), "56-2-1": (1, 3)}
# (max_iter, check_every): |f/d| is first read at iteration 1, 2 or 7, and at (7, 1) and (7, 2) it is kept over repeated checks
ITERATE_OPTS = ((1, 1), (2, 1), (7, 1), (7, 2), (7, 7))
# a loose tolerance that stops instances at different early checks: on the restatement every residual of every check stays at least
# 7e-4 (relative) away from its threshold at these shapes, far above IT_TOL
LOOSE = dict(eps_abs=0.1, eps_rel=0.1, max_iter=12, check_every=1)
_ids = lambda c: c.id


def _admm_solver(capi, p, batch, rho, profile, refs=None):
    s = capi.Solver(p.n, p.m, p.N, batch, structured_fallback=False)
    s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=rho, rho_profile=profile)
    if refs is None:
        s.set_reference(p.x_ref, p.u_ref)
    else:
        s.set_reference(refs[0], refs[1], per_instance=True)
    return s


def _run(s, o):
    s.calculate(o)
    return s.get_results()


@pytest.mark.parametrize("profile,rho", PROFILES)
@pytest.mark.parametrize("batch", (BATCH, 1))
@pytest.mark.parametrize("case", ADMM_CASES, ids=_ids)
def test_admm_iterates_and_stops(capi, co, case, batch, profile, rho):
    """k_admm with the finish off at an odd KS (3-2-6, and 56-2-1 without the affine first iterate: fragments one by one), at three
    waves and at eight (pair-packed fragments), batch 37 and 1: the restatement's iterates after 1, 2 and 7 iterations with the first
    check at iteration 1, 2 and 7; its iteration counts and status under a loose tolerance; and a warm start chained on its own cold run."""
    assert case.build == ADMM_BUILDS[case.id]
    ref = cc.reference(case)
    p, X0 = ref["p"], ref["X0"][:batch]
    des = mo.design_shared(p, rho=rho, rho_profile=profile)
    s = _admm_solver(capi, p, batch, rho, profile)
    worst = 0.0
    try:
        s.update_initialization(X0)
        for max_iter, check_every in ITERATE_OPTS:
            kw = dict(max_iter=max_iter, check_every=check_every)
            r = _run(s, capi.default_opts(rho=rho, polish=0, **kw))
            o = co.step_batch(p, des, X0, polish=False, **kw)
            what = (case.id, batch, profile, kw)
            assert np.array_equal(r["iters"], o["iters"]) and np.array_equal(r["status"], o["status"]), what
            err = float(np.abs(r["u"] - o["u"]).max())
            worst = max(worst, err)
            assert err <= IT_TOL, (what, err)
        # early convergence
        r = _run(s, capi.default_opts(rho=rho, polish=0, **LOOSE))
        for i in range(batch):
            o = cc.admm(des, cc.fs_of(p, des, X0[i]), **LOOSE)
            assert r["iters"][i] == o["iters"] and r["status"][i] == o["status"], (case.id, batch, profile, i)
            err = float(np.abs(r["u"][i] - cc.admm_u(p, des, o)).max())
            worst = max(worst, err)
            assert err <= IT_TOL, (case.id, batch, profile, i, err)
        # warm start
        kw = dict(max_iter=7, check_every=2)
        cold = _run(s, capi.default_opts(rho=rho, polish=0, **kw))
        s.update_initialization(0.9 * X0)
        warm = _run(s, capi.default_opts(rho=rho, polish=0, warm_start=1, **kw))
        for i in range(batch):
            c0 = cc.admm(des, cc.fs_of(p, des, X0[i]), **kw)
            c1 = cc.admm(des, cc.fs_of(p, des, 0.9 * X0[i]), c0["x"], c0["z"], c0["y"], **kw)
            for rr, o in ((cold, c0), (warm, c1)):
                assert rr["iters"][i] == o["iters"] and rr["status"][i] == o["status"], (case.id, batch, profile, i)
                err = float(np.abs(rr["u"][i] - cc.admm_u(p, des, o)).max())
                worst = max(worst, err)
                assert err <= IT_TOL, (case.id, batch, profile, i, err)
    finally:
        s.close()
    _note("iterate", "k_admm<%d,%d> %s batch %d %s" % (case.build + (case.id, batch, profile)), worst, IT_TOL)


@pytest.mark.parametrize("profile,rho", PROFILES)
@pytest.mark.parametrize("batch", (BATCH, 1))
@pytest.mark.parametrize("case", ADMM_CASES, ids=_ids)
def test_table_equals_per_row_loads(capi, case, batch, profile, rho):
    """shared references (the row-constant table) against the same references given per instance (per-row loads, no table), both from
    the full first product: the same operations on the same values -- u, iters and status of the iterate bit for bit"""
    ref = cc.reference(case)
    p, X0 = ref["p"], ref["X0"][:batch]
    xr = np.ascontiguousarray(np.broadcast_to(p.x_ref[None], (batch,) + p.x_ref.shape))
    ur = np.ascontiguousarray(np.broadcast_to(p.u_ref[None], (batch,) + p.u_ref.shape))
    a = _admm_solver(capi, p, batch, rho, profile)
    b = _admm_solver(capi, p, batch, rho, profile, refs=(xr, ur))
    try:
        for kw in (dict(polish=0, max_iter=7, check_every=2), dict(polish=0, **LOOSE)):
            out = []
            for s in (a, b):
                s.update_initialization(X0)
                o = capi.default_opts(rho=rho, **kw)
                o.reserved[0] |= capi.OPT_FULL_FIRST_PRODUCT
                out.append(_run(s, o))
            for k in ("u", "iters", "status"):
                assert np.array_equal(out[0][k], out[1][k]), (case.id, batch, profile, kw, k)
    finally:
        a.close()
        b.close()
