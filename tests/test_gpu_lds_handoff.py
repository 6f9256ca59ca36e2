"""The one-kernel step's hand-off of the ADMM results (z, v0, the signs of y, the status, the processing order) to its finish through
LDS against the round trip through global memory (ALMPC_OPT_HBM_HANDOFF in opts.reserved[0]), against the two-kernel path and
against the exact oracle.  Run on an MI355X: pytest -m gpu.

A step takes the LDS hand-off when it runs as one kernel (k_step_fused: nz 113..128), keeps no warm state
(ALMPC_OPT_NO_WARM_STATE) and its finish has the workgroup-shared second-tier slot.  The same device functions then run on the same
values, so every comparison between the three paths is BIT FOR BIT (NaNs included: the byte images are compared).  Ranks 0..7 of a
tile wait in the buffers of the waves 0..7, ranks 8..15 in the second-tier slot: the batches are one partial tile without a rank
beyond 7 (5), one full tile (16), a partial tile behind two full ones (37) and, on the quadrotor, 200.  The exact solutions are
computed once per shape for the largest batch (the smaller batches are its first instances)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U_TOL = 1e-6
KEYS = ("u", "e_u", "x", "e_x", "status", "iters", "polish_iters")
SHAPES = [(12, 4, 30), (3, 1, 117), (4, 2, 59)]   # the quadrotor; odd nz (the last row pair half empty); nz 118
QUAD = (12, 4, 30)


def _problem(mo, n, m, N):
    """The benchmark's quadrotor for (12, 4, 30); else a random stable plant with an input-rate weight and a time-varying u_ref."""
    if (n, m, N) == QUAD:
        return mo.quadrotor()
    rng = np.random.default_rng(7000 * n + 10 * m + N)
    A = rng.standard_normal((n, n))
    A *= 0.97 / np.max(np.abs(np.linalg.eigvals(A)))
    B = rng.standard_normal((n, m))
    u_ref = 0.05 * rng.standard_normal((m, 1)) + 0.03 * rng.standard_normal((m, N))
    return mo.make_problem(A, B, N, -0.5 * np.ones(m), 0.7 * np.ones(m), x_ref=0.1 * rng.standard_normal(n), u_ref=u_ref,
                           q=10.0, r=1.0, s=0.5)


def _x0(mo, p, batch):
    if (p.n, p.m, p.N) == QUAD:   # the benchmark's three amplitudes, interleaved so that every tile holds easy and hard instances
        parts = [mo.quadrotor_x0_batch((batch + 2) // 3, a, first_instance=300 * k) for k, a in enumerate((0.3, 1.0, 3.0))]
        return np.stack(parts, axis=1).reshape(-1, p.n)[:batch]
    return 3.0 * np.random.default_rng(p.n + p.N).standard_normal((batch, p.n))


_CASES = {}


def _case(mo, shape):
    """(problem, X0 of the largest batch, exact u of every instance), once per shape"""
    if shape not in _CASES:
        p = _problem(mo, *shape)
        X0 = _x0(mo, p, 200 if shape == QUAD else 37)
        _, _, H, F = mo.condense(p)   # (solve_mpc_exact's box-only branch with the condensing done once)
        fS = mo.s_rate_gradient(p)
        lo = (p.u_min[:, None] - p.u_ref).T.reshape(-1)
        hi = (p.u_max[:, None] - p.u_ref).T.reshape(-1)
        U = np.stack([mo.rollout(p, x, mo.solve_box_qp_exact(H, F @ (x - p.x_ref[:, 0]) + fS, lo, hi))["u"] for x in X0])
        _CASES[shape] = (p, X0, U)
    return _CASES[shape]


def _solver(capi, p, batch, rho, profile):
    s = capi.Solver(p.n, p.m, p.N, batch)
    s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=rho, rho_profile=profile)
    s.set_reference(p.x_ref, p.u_ref)
    return s


def _opts(capi, hbm=False, **kw):
    o = capi.default_opts(**kw)
    if hbm:
        o.reserved[0] |= capi.OPT_HBM_HANDOFF
    return o


def _run(s, o):
    s.calculate(o)
    return s.get_results()


def _same(a, b, what):
    for k in KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


def _three(capi, s, **kw):
    """(a) the LDS hand-off, (b) the same kernel with the round trip through global memory, (c) the two-kernel path"""
    a = _run(s, _opts(capi, keep_warm_state=False, **kw))
    b = _run(s, _opts(capi, hbm=True, keep_warm_state=False, **kw))
    s.set_step_fusion(False)
    c = _run(s, _opts(capi, keep_warm_state=False, **kw))
    s.set_step_fusion(True)
    return a, b, c


# ---------------------------------------------------------------------------- the three paths and the oracle
@pytest.mark.parametrize("max_iter", [6, 1])
@pytest.mark.parametrize("profile,rho", [("scalar", 0.1), ("stiffness", 45.0)])
@pytest.mark.parametrize("n,m,N", SHAPES)
def test_lds_handoff_equals_hbm_handoff_two_kernel_path_and_oracle(capi, mo, n, m, N, profile, rho, max_iter):
    p, X0, U = _case(mo, (n, m, N))
    solved = 0
    for batch in (5, 16, 37) + ((200,) if (n, m, N) == QUAD else ()):
        s = _solver(capi, p, batch, rho, profile)
        s.update_initialization(X0[:batch])
        a, b, c = _three(capi, s, rho=rho, max_iter=max_iter, check_every=max_iter)
        s.close()
        _same(a, b, (batch, "LDS hand-off against the hand-off through global memory"))
        _same(a, c, (batch, "LDS hand-off against the two-kernel path"))
        ok = a["status"] == 0
        err = np.abs(a["u"] - U[:batch]).reshape(batch, -1).max(axis=1)
        print((n, m, N), profile, max_iter, batch, "solved", int(ok.sum()), "max |u - u*| on them", float(err[ok].max(initial=0.0)))
        assert np.all(err[ok] <= U_TOL), (batch, np.flatnonzero(ok & (err > U_TOL)))
        solved += int(ok.sum())
    assert solved > 0, "no instance was solved: the comparison with the oracle shows nothing"


# ---------------------------------------------------------------------------- the gate of the second-tier slot
GATE_AMPLITUDE, GATE_FIRST = 10.0, 500   # (found with the loop below: five of the first tile's instances guess 36 .. 59 rows)


def test_second_tier_waits_for_the_staged_records(capi, mo):
    """Instances whose guessed working set has more than 32 rows enter the second tier at once.  They are the first ranks of their
    tile, so the records of the ranks 8..15 still wait in the shared second-tier slot: the slot must not be claimed, the wave takes
    the global scratch (with ALMPC_OPT_HBM_HANDOFF the first of them gets the slot).  The arithmetic is the same in both homes.

    Every path runs on a handle of its own, two steps each, and first steps are compared with first steps, second with second: at
    this amplitude the finish gives up on some instances (more than 64 active rows) and the handle re-solves them stage by stage,
    and that re-solve depends on what the handle's previous step left (measured on the parent commit as well, with the tier in
    either home: the first step of a handle differs from its later ones on the re-solved instances by 1e-11, the later ones agree
    with each other)."""
    p = mo.quadrotor()
    rho = 45.0
    des = mo.design_shared(p, rho=rho, rho_profile="stiffness")
    X0 = mo.quadrotor_x0_batch(32, GATE_AMPLITUDE, first_instance=GATE_FIRST)
    guess = []
    for x0 in X0:
        fs = des["Fs"] @ (x0 - p.x_ref[:, 0]) + des["fS"]
        r = mo.admm_box(des["Hs"], fs, des["lo"], des["hi"], rho=des["rho_vec"], sigma=des["sigma"], max_iter=6, check_every=6,
                        Minv=des["Minv"], unscale=des["d"])
        # (no active-set change allowed: n_active is the size of the guessed set)
        guess.append(mo.polish_active_set(des["G"], -des["G"] @ fs, des["lo"], des["hi"], r["z"], r["y"], max_iter=0)["n_active"])
    big = (np.array(guess) > 32).reshape(2, 16).sum(axis=1)
    print("guessed rows", guess, "instances beyond 32 per tile", big)
    assert big.max() >= 2, "no tile with two instances that start in the second tier: the test shows nothing"

    def two_steps(hbm, fused):
        s = _solver(capi, p, 32, rho, "stiffness")
        s.set_step_fusion(fused)
        s.update_initialization(X0)
        out = [_run(s, _opts(capi, hbm=hbm, keep_warm_state=False, rho=rho, max_iter=6, check_every=6)) for _ in range(2)]
        s.close()
        return out

    a, b, c = two_steps(False, True), two_steps(True, True), two_steps(False, False)
    for k, step in enumerate(("first step", "second step")):
        _same(a[k], b[k], "second tier at the start, %s: LDS hand-off against the hand-off through global memory" % step)
        _same(a[k], c[k], "second tier at the start, %s: LDS hand-off against the two-kernel path" % step)


# ---------------------------------------------------------------------------- paths that must not change
def test_state_keeping_and_warm_steps_ignore_the_bit(capi, mo):
    p, X0, _ = _case(mo, QUAD)
    s = _solver(capi, p, 37, 45.0, "stiffness")
    out = []
    for hbm in (False, True):
        s.update_initialization(X0[:37])
        cold = _run(s, _opts(capi, hbm=hbm, rho=45.0, max_iter=6, check_every=6))              # keeps x, z, y
        s.update_initialization(0.9 * X0[:37])
        out.append((cold, _run(s, _opts(capi, hbm=hbm, rho=45.0, max_iter=6, check_every=6, warm_start=1))))
    s.close()
    _same(out[0][0], out[1][0], "state-keeping step")
    _same(out[0][1], out[1][1], "warm step")


def test_per_instance_references(capi, mo):
    p, X0, _ = _case(mo, QUAD)
    batch = 37
    rng = np.random.default_rng(11)
    xr = p.x_ref[None] + 0.05 * rng.standard_normal((batch, p.n, 1)) * np.ones((1, 1, p.N + 1))
    ur = p.u_ref[None] + 0.04 * rng.standard_normal((batch, p.m, p.N))
    s = _solver(capi, p, batch, 45.0, "stiffness")
    s.set_reference(xr, ur, per_instance=True)
    s.update_initialization(X0[:batch])
    kw = dict(rho=45.0, max_iter=6, check_every=6)
    a, b, c = _three(capi, s, **kw)
    k = _run(s, _opts(capi, **kw))            # the state-keeping step: the parent's path
    kb = _run(s, _opts(capi, hbm=True, **kw))
    s.close()
    _same(a, b, "per-instance references, no warm state")
    _same(a, c, "per-instance references, two-kernel path")
    _same(a, k, "per-instance references, state-keeping step")
    _same(k, kb, "per-instance references, state-keeping step, bit set")


# ---------------------------------------------------------------------------- a live handle
def test_hand_off_step_leaves_nothing_stale_for_later_steps(capi, mo):
    """After a hand-off step the z / v0 / sign buffers in global memory hold whatever an earlier step left.  A state-keeping step
    and a warm step behind it must equal the same two steps on a fresh handle."""
    p, X0, _ = _case(mo, QUAD)
    kw = dict(rho=45.0, max_iter=6, check_every=6)

    def keep_then_warm(s):
        s.update_initialization(X0[:37])
        k = _run(s, _opts(capi, **kw))
        s.update_initialization(0.9 * X0[:37])
        return k, _run(s, _opts(capi, warm_start=1, **kw))

    s = _solver(capi, p, 37, 45.0, "stiffness")
    s.update_initialization(X0[37:74])                     # other instances: what they leave behind must not matter
    _run(s, _opts(capi, keep_warm_state=False, **kw))
    live = keep_then_warm(s)
    s.close()
    t = _solver(capi, p, 37, 45.0, "stiffness")
    fresh = keep_then_warm(t)
    t.close()
    _same(live[0], fresh[0], "state-keeping step behind a hand-off step")
    _same(live[1], fresh[1], "warm step behind them")


# ---------------------------------------------------------------------------- a non-finite x0
def test_non_finite_x0_is_handed_on(capi, mo):
    p, X0, U = _case(mo, QUAD)
    batch, bad = 37, 21
    X = X0[:batch].copy()
    X[bad, 2] = np.nan
    s = _solver(capi, p, batch, 45.0, "stiffness")
    s.update_initialization(X)
    a, b, c = _three(capi, s, rho=45.0, max_iter=6, check_every=6)
    s.update_initialization(X0[:batch])
    clean = _run(s, _opts(capi, keep_warm_state=False, rho=45.0, max_iter=6, check_every=6))
    s.close()
    _same(a, b, "non-finite x0: LDS hand-off against the hand-off through global memory")
    _same(a, c, "non-finite x0: LDS hand-off against the two-kernel path")
    assert a["status"][bad] == 2
    others = np.arange(batch) != bad
    for k in KEYS:
        assert np.array_equal(a[k][others], clean[k][others]), k
    assert np.all(a["status"][others] == 0)
    assert np.abs(a["u"][others] - U[:batch][others]).max() <= U_TOL
