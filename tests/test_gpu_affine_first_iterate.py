"""The cold start's first ADMM iterate from an n-column product (xt1 = W e0 + wS, W = -Minv F', wS = -Minv fS) against the full
nz x nz product (ALMPC_OPT_FULL_FIRST_PRODUCT in opts.reserved[0]) and against the oracle.  Run on an MI355X: pytest -m gpu.

With x = z = y = 0 the first right-hand side is -f' = -(F' e0 + fS), so the two forms are the same iteration summed in another order:
the iterates agree to 1e-9 (the tolerance test_admm_only_matches_oracle_iterate holds the device to against the oracle).  W belongs
to the design and wS to a shared reference of almpc_set_reference.  Per-instance references, and shapes whose design workspace has no
room behind W (N = 1 with large n), take the full product: the tests assert which form ran (the two forms differ in the last bits, the
same form twice does not).  The tests at the end change design and references on a live handle and compare with a fresh one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U_TOL = 1e-6
IT_TOL = 1e-9
# 8-wave tiles on the fused path with odd / padded nz, the benchmark's shape, a small tile, and two shapes with n > 16 (the general
# fragment path of the prologue: ksf = 5 and 16)
SHAPES = [(3, 1, 117), (2, 1, 113), (4, 4, 31), (12, 4, 30), (3, 2, 7), (20, 1, 40), (64, 2, 3)]
SMALL_BATCH_MAX = 500   # shapes with n*m*N up to this also run a batch below one tile


def _problem(mo, n, m, N):
    """The benchmark's quadrotor for (12, 4, 30); else a random stable plant with an input-rate weight and a time-varying u_ref, so
    that fS (and with it wS) is not zero."""
    if (n, m, N) == (12, 4, 30):
        return mo.quadrotor()
    rng = np.random.default_rng(7000 * n + 10 * m + N)
    A = rng.standard_normal((n, n))
    A *= 0.97 / np.max(np.abs(np.linalg.eigvals(A)))
    B = rng.standard_normal((n, m))
    u_ref = 0.05 * rng.standard_normal((m, 1)) + 0.03 * rng.standard_normal((m, N))
    return mo.make_problem(A, B, N, -0.5 * np.ones(m), 0.7 * np.ones(m), x_ref=0.1 * rng.standard_normal(n), u_ref=u_ref,
                           q=10.0, r=1.0, s=0.5 if N > 2 else 0.0)


def _x0(mo, p, batch):
    if (p.n, p.m, p.N) == (12, 4, 30):
        return mo.quadrotor_x0_batch(batch, 3.0, first_instance=77)
    return 3.0 * np.random.default_rng(p.n + p.N).standard_normal((batch, p.n))


def _solver(capi, p, batch, rho=0.1, rho_profile="scalar", reference=True):
    s = capi.Solver(p.n, p.m, p.N, batch)
    s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=rho, rho_profile=rho_profile)
    if reference:
        s.set_reference(p.x_ref, p.u_ref)
    return s


def _opts(capi, full_first=False, **kw):
    o = capi.default_opts(**kw)
    if full_first:
        o.reserved[0] |= capi.OPT_FULL_FIRST_PRODUCT
    return o


def _run(s, o):
    s.calculate(o)
    return s.get_results()


def _batches(n, m, N):
    return (37, 5) if n * m * N <= SMALL_BATCH_MAX else (37,)


def _iterate_cases():
    for max_iter in (1, 2, 6):
        for check_every in sorted({1, max_iter}):
            for alpha in (1.0, None):
                yield max_iter, check_every, alpha


# ---------------------------------------------------------------------------- iterates, finish off
@pytest.mark.parametrize("profile,rho", [("scalar", 0.1), ("stiffness", 30.0)])
@pytest.mark.parametrize("n,m,N", SHAPES)
def test_first_iterates_match_full_product_and_oracle(capi, mo, co, n, m, N, profile, rho):
    p = _problem(mo, n, m, N)
    des = mo.design_shared(p, rho=rho, rho_profile=profile)
    for batch in _batches(n, m, N):
        X0 = _x0(mo, p, batch)
        s = _solver(capi, p, batch, rho, profile)
        s.update_initialization(X0)
        for max_iter, check_every, alpha in _iterate_cases():
            kw = dict(rho=rho, polish=0, max_iter=max_iter, check_every=check_every)
            if alpha is not None:
                kw["alpha"] = alpha
            a = _run(s, _opts(capi, **kw))
            f = _run(s, _opts(capi, full_first=True, **kw))
            ckw = dict(max_iter=max_iter, check_every=check_every, polish=False)
            if alpha is not None:
                ckw["alpha"] = alpha
            c = co.step_batch(p, des, X0, **ckw)
            case = (batch, max_iter, check_every, alpha)
            print(case, "affine vs full", np.abs(a["u"] - f["u"]).max(), "affine vs oracle", np.abs(a["u"] - c["u"]).max(),
                  "full vs oracle", np.abs(f["u"] - c["u"]).max())
            assert np.array_equal(a["iters"], f["iters"]) and np.array_equal(a["status"], f["status"]), case
            assert np.abs(a["u"] - f["u"]).max() <= IT_TOL, case
            assert np.abs(a["u"] - c["u"]).max() <= IT_TOL, case
            assert np.all(a["polish_iters"] == 0)
            if max_iter == 6 and batch == 37:   # the affine form did run: a re-associated sum leaves other last bits somewhere
                assert not np.array_equal(a["u"], f["u"]), case
        s.close()


def test_shape_without_workspace_room_keeps_the_full_product(capi, mo, co):
    """n = 64, N = 1: the design's workspace (kr = 64 rows) has no room for wS and the table behind W (n + 9 rows): the step takes the
    full first product and the per-row loads, with or without the bit, and still gives the oracle's iterate."""
    p = _problem(mo, 64, 2, 1)
    des = mo.design_shared(p)
    X0 = _x0(mo, p, 37)
    s = _solver(capi, p, 37)
    s.update_initialization(X0)
    kw = dict(polish=0, max_iter=6, check_every=6)
    a = _run(s, _opts(capi, **kw))
    f = _run(s, _opts(capi, full_first=True, **kw))
    s.close()
    c = co.step_batch(p, des, X0, polish=False, max_iter=6, check_every=6)
    for k in ("u", "iters", "status"):
        assert np.array_equal(a[k], f[k]), k
    assert np.abs(a["u"] - c["u"]).max() <= IT_TOL


# ---------------------------------------------------------------------------- finish on, the benchmark's operating point
@pytest.fixture(scope="module")
def bench_point(mo):
    p = mo.quadrotor()
    X0 = np.concatenate([mo.quadrotor_x0_batch(48, a, first_instance=48 * k) for k, a in enumerate((0.3, 1.0, 3.0))])
    sample = list(range(0, len(X0), 16))
    exact = {i: mo.solve_mpc_exact(p, X0[i])["u"] for i in sample}
    return p, X0, exact


def test_finish_on_at_the_benchmark_point(capi, bench_point):
    p, X0, exact = bench_point
    s = _solver(capi, p, len(X0), 45.0, "stiffness")
    s.update_initialization(X0)
    res = {}
    for keep in (False, True):
        for full in (False, True):
            res[keep, full] = _run(s, _opts(capi, full_first=full, rho=45.0, max_iter=6, check_every=6, keep_warm_state=keep))
    s.close()
    for key, r in res.items():
        assert np.all(r["status"] == 0), key
        for i, u in exact.items():
            assert np.abs(r["u"][i] - u).max() <= U_TOL, (key, i)
    for keep in (False, True):
        assert np.array_equal(res[keep, False]["status"], res[keep, True]["status"])
    for full in (False, True):
        for k in ("u", "x", "status", "iters", "polish_iters"):
            assert np.array_equal(res[False, full][k], res[True, full][k]), (full, k)


# ---------------------------------------------------------------------------- paths that must not change
@pytest.mark.parametrize("n,m,N,polish", [(12, 4, 30, 1), (3, 2, 7, 0)])   # (finish off on the small shape: with it the batch goes to
def test_warm_start_steps_do_not_take_the_affine_form(capi, mo, n, m, N, polish):   # the one-wave-per-instance step, not the tile kernel)
    p = _problem(mo, n, m, N)
    X0 = _x0(mo, p, 37)
    s = _solver(capi, p, 37)
    s.update_initialization(X0)
    out = []
    for full in (False, True):
        _run(s, _opts(capi, max_iter=6, check_every=6, polish=polish))        # cold, state kept: the same state both times
        s.update_initialization(0.9 * X0)
        out.append(_run(s, _opts(capi, full_first=full, max_iter=6, check_every=6, warm_start=1, polish=polish)))
        s.update_initialization(X0)
    s.close()
    for k in ("u", "x", "iters"):
        assert np.array_equal(out[0][k], out[1][k]), k


# ---------------------------------------------------------------------------- per-instance references, and the lifetime of W / wS
def _refs(p, batch, seed):
    rng = np.random.default_rng(seed)
    xr = p.x_ref[None] + 0.05 * rng.standard_normal((batch, p.n, 1)) * np.ones((1, 1, p.N + 1))
    ur = p.u_ref[None] + 0.04 * rng.standard_normal((batch, p.m, p.N))     # time-varying per instance: fS_i != 0 with S != 0
    return xr, ur


@pytest.mark.parametrize("n,m,N", [(4, 4, 31), (3, 2, 7)])
def test_per_instance_references_and_stale_constants(capi, mo, n, m, N):
    p = _problem(mo, n, m, N)
    assert p.S[0, 0] != 0.0
    batch = 37
    X0 = _x0(mo, p, batch)
    kw = dict(polish=0, max_iter=6, check_every=6)
    keys = ("u", "iters", "status")

    def fresh(rho, refs):
        t = _solver(capi, p, batch, rho, reference=False)
        if refs is not None:
            t.set_reference(*refs, per_instance=True)
        t.update_initialization(X0)
        r = _run(t, _opts(capi, rho=rho, **kw))
        t.close()
        return r

    def same(a, b, what):
        for k in keys:
            assert np.array_equal(a[k], b[k]), (what, k)

    r1, r2 = _refs(p, batch, 1), _refs(p, batch, 2)
    s = _solver(capi, p, batch)                    # shared reference first: the per-instance one below replaces the buffers
    s.update_initialization(X0)
    s.set_reference(*r1, per_instance=True)
    a = _run(s, _opts(capi, **kw))
    f = _run(s, _opts(capi, full_first=True, **kw))
    same(a, f, "per-instance references take the full first product: the bit changes nothing")
    same(a, fresh(0.1, r1), "first per-instance reference")
    # a second reference with other values
    s.set_reference(*r2, per_instance=True)
    a2 = _run(s, _opts(capi, **kw))
    same(a2, _run(s, _opts(capi, full_first=True, **kw)), "second per-instance reference, bit set")
    assert np.abs(a2["u"] - a["u"]).max() > 1e-6, "the second reference does not move the iterate: the test shows nothing"
    same(a2, fresh(0.1, r2), "second per-instance reference")
    # a re-design with another rho replaces Minv: W and wS are made again (the design leaves the default reference, zeros, shared)
    s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=0.7)
    s.update_initialization(X0)
    same(_run(s, _opts(capi, rho=0.7, **kw)), fresh(0.7, None), "re-design, default reference")
    s.set_reference(*r2, per_instance=True)
    a3 = _run(s, _opts(capi, rho=0.7, **kw))
    same(a3, _run(s, _opts(capi, full_first=True, rho=0.7, **kw)), "re-design, per-instance reference, bit set")
    same(a3, fresh(0.7, r2), "re-design, then the per-instance reference")
    # back to a shared reference with fS != 0 (wS is made again, for the new Minv), then another one
    for scale in (1.0, -0.5):
        s.set_reference(p.x_ref, scale * p.u_ref)
        a4 = _run(s, _opts(capi, rho=0.7, **kw))
        f4 = _run(s, _opts(capi, full_first=True, rho=0.7, **kw))
        assert np.abs(a4["u"] - f4["u"]).max() <= IT_TOL and np.array_equal(a4["iters"], f4["iters"])
        assert not np.array_equal(a4["u"], f4["u"]), "the affine form did not run on the shared reference"
        t = _solver(capi, p, batch, 0.7, reference=False)
        t.set_reference(p.x_ref, scale * p.u_ref)
        t.update_initialization(X0)
        same(a4, _run(t, _opts(capi, rho=0.7, **kw)), "shared reference after the per-instance one")
        t.close()
    s.close()


# ---------------------------------------------------------------------------- the row-constant table of shared references
@pytest.mark.parametrize("n,m,N", [(12, 4, 30), (4, 4, 31), (6, 3, 30)])   # fused step, and the k_admm + k_polish pair of 8 waves (nz 124: past the fused step) and of 6
def test_row_constant_table_gives_the_bounds_of_the_per_instance_loads(capi, mo, n, m, N):
    """Shared references read d, 1/d, lo, hi, rho, fS, v0S, wS from a table made at set_reference; per-instance references load and
    derive them in the step as before.  The finish forms lo / hi itself and tests ADMM's clipped z against them, so the table must
    hold the same bits: the same references given once (table) and broadcast per instance (loads) must give the same instances
    without a finish iteration and the same u, bit for bit."""
    p = _problem(mo, n, m, N)
    batch = 37
    X0 = _x0(mo, p, batch)
    quad = (n, m, N) == (12, 4, 30)
    # (the quadrotor's own u_ref is zero: shift it by a tenth of the box, differently per input and stage)
    u_ref = p.u_ref + (0.1 * (p.u_max - p.u_min)[:, None] * np.cos(np.arange(N) + np.arange(m)[:, None]) if quad else 0.0)
    assert np.abs(u_ref).max() > 0.0
    rho, profile = (45.0, "stiffness") if quad else (0.1, "scalar")
    o = dict(rho=rho, max_iter=6, check_every=6) if quad else dict(rho=rho)
    res = []
    for per_instance in (False, True):
        s = _solver(capi, p, batch, rho, profile, reference=False)
        if per_instance:
            s.set_reference(np.broadcast_to(p.x_ref, (batch,) + p.x_ref.shape), np.broadcast_to(u_ref, (batch,) + u_ref.shape), per_instance=True)
        else:
            s.set_reference(p.x_ref, u_ref)
        s.update_initialization(X0)
        res.append(_run(s, _opts(capi, full_first=True, **o)))   # (the full first product on both: only the constants differ)
        if not per_instance:   # the table is made again by a second set_reference and by a re-design
            s.set_reference(p.x_ref, 0.5 * u_ref)
            s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=rho, rho_profile=profile)
            s.set_reference(p.x_ref, u_ref)
            s.update_initialization(X0)
            res.append(_run(s, _opts(capi, full_first=True, **o)))
        s.close()
    tab, tab2, loads = res
    assert np.all(loads["status"] == 0)
    at_bound = np.isclose(loads["u"], p.u_min[None, :, None]) | np.isclose(loads["u"], p.u_max[None, :, None])
    assert at_bound.any(), "no active bound: the test shows nothing"
    d = mo.design_shared(p, rho=rho, rho_profile=profile)["d"]
    assert np.ptp(d) > 0.0
    for r in (tab, tab2):
        assert np.array_equal(r["polish_iters"] == 0, loads["polish_iters"] == 0)
        for k in ("u", "status", "iters", "polish_iters"):
            assert np.array_equal(r[k], loads[k]), k
