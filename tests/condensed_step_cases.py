"""The shapes at which the condensed shared-model step (almpc_design_shared -> almpc_calculate) is tested: one table for
tests/test_condensed_step_cases.py (CPU: the table reaches every instantiated build and route, and its inputs are well posed) and
tests/test_gpu_condensed_step_shapes.py (GPU: the step against the oracles, on the route the table names).

The selection rules of csrc/almpc_api.hip are restated here in Python (pick_ks, roll_geom, build_rollout_table's block size,
polish_layout, pick_route, step_rollout); the CPU test holds the constants against the source."""
import functools

import numpy as np

import mpc_oracle as mo

# ---------------------------------------------------------------------------- constants of the source (checked by the CPU test)
ADMM_BUILDS = ((1, 3), (1, 4), (2, 8), (3, 10), (3, 12), (4, 16), (5, 20), (6, 24), (7, 28), (8, 30), (8, 32))   # k_admm<NRB, KS>
FUSED_BUILDS = ((8, 30), (8, 32))                                                                                # k_step_fused<NRB, KS>
WAVE_BUILDS = (16, 32, 48, 64)                                                                                   # k_step_inst_wave<NZC>
ROLL_SMX, ROLL_NX = 24, 16
ROLL_EXACT = (20, 12)               # roll_run<20, 12>: s*m <= 20 && n <= 12
POLISH_SG_SHARED_CAP = 48
POLISH_LDS_MIN_PER_WAVE = 128 + 64 + 64 + 32
POLISH_WAVES_GLDS = 8
TILE = 16
LDS_MAX = 160 * 1024
NUM_CUS = 256                       # MI355X; pick_route sends up to two instances per CU to the one-wave step
QUAD = (12, 4, 30)
BATCH = 37                          # two full tiles and a partial one of 5
EXACT_STEP = 3                      # every third instance against the exact oracle (heavy cases: every instance)


# ---------------------------------------------------------------------------- the selection rules
def nrb_of(nz):
    return (nz + 15) // 16


def pick_ks(nz, nrb):
    exact = (nz + 3) // 4
    if nrb == 8 and exact <= 30:
        return 30
    if nrb == 3 and exact <= 10:
        return 10
    if nrb == 1 and exact <= 3:
        return 3
    return 4 * nrb


def roll_geom(n, m, N):
    """(g, cpl, fits) of the stage-by-stage rollout in a finish's tail"""
    g = 1
    while 2 * g * n <= 64:
        g *= 2
    C = n + m
    cpl = (C + g - 1) // g
    fits = (N + 1) * C <= 32 * 32 and cpl <= 8
    cpl = 1 if cpl <= 1 else 2 if cpl <= 2 else 4 if cpl <= 4 else 8
    return g, cpl, fits


def roll_block(n, m, N, stagewise=False):
    """(s, nb) of the blocked rollout, (0, 0) where build_rollout_table leaves the shape to the stage-by-stage one"""
    s = min(N, 64 // n, ROLL_SMX // m)
    if not (s >= 1 and n <= ROLL_NX and not stagewise):
        return 0, 0
    return s, (N + s - 1) // s


def roll_exact(n, m, s):
    return s * m <= ROLL_EXACT[0] and n <= ROLL_EXACT[1]


def polish_shared_total(n, m, N, nz, nzs, fused):
    off_ab = nzs + 2 * m + nz
    off_xref = off_ab + (n * (n + m) if fused and fused != 3 else 0)
    return (off_xref + ((N + 1) * n if fused else 0) + 1) & ~1


def admm_lds_bytes(n, nz):
    nrb = nrb_of(nz)
    return (2 * 16 * nrb * TILE + nrb * 8 * TILE + 4 * ((n + 3) // 4) * TILE) * 8


def polish_layout(n, m, N, stagewise=False, sg_global=False):
    """polish_layout of a shared model: dict(fused, fuse_rollout, per_wave, total, slot, l_glds, l_step) (bytes)"""
    nz = m * N
    nzs = 16 * nrb_of(nz)
    s, _ = roll_block(n, m, N, stagewise)
    blocked = s > 0
    fused = roll_geom(n, m, N)[2] or blocked
    fr = (3 if blocked else 1) if fused else 0
    per_wave = POLISH_LDS_MIN_PER_WAVE
    if fused and not blocked and (N + 1) * (n + m) > per_wave:
        per_wave = (N + 1) * (n + m)
    per_wave = (per_wave + 1) & ~1
    total = polish_shared_total(n, m, N, nz, nzs, fr)
    g_lds = nz * ((nz + 1) & ~1)
    l_glds = (g_lds + total + POLISH_WAVES_GLDS * per_wave + 2) * 8
    slot_bytes = POLISH_SG_SHARED_CAP * 64 * 8
    slot = l_glds + slot_bytes <= LDS_MAX and not sg_global
    if slot:
        l_glds += slot_bytes
    l_step = max(l_glds - g_lds * 8, admm_lds_bytes(n, nz)) + g_lds * 8
    return dict(fused=fused, fuse_rollout=fr, per_wave=per_wave, total=total, slot=slot, l_glds=l_glds, l_step=l_step)


def pick_route(n, m, N, batch=BATCH, polish=True, fuse_step=True, no_glds=False, no_shared_wave=False, stagewise=False, sg_global=False):
    """fused (k_step_fused) | wave (k_step_inst_wave on shared operands) | tile (k_admm + k_polish<true>) | tile_l2 (k_admm +
    k_polish<false>) | nopolish (k_admm + the separate rollout)"""
    if not polish:
        return "nopolish"
    nz = m * N
    nrb = nrb_of(nz)
    L = polish_layout(n, m, N, stagewise, sg_global)
    if fuse_step and not no_glds and nrb == 8 and L["fused"] and L["l_step"] <= LDS_MAX:
        return "fused"
    if 16 * nrb <= 64 and L["fused"] and not no_shared_wave and batch <= 2 * NUM_CUS and (L["total"] + L["per_wave"]) * 8 <= 64 * 1024:
        return "wave"
    return "tile" if L["l_glds"] <= LDS_MAX and not no_glds else "tile_l2"


def separate_rollout(n, m, N):
    """(k_rollout build, LDS bytes, beyond the 64 KiB default) of step_rollout"""
    per_wave, shared = n * (N + 1) + m * N, n * n + n * m
    if (shared + 4 * per_wave) * 8 <= 60 * 1024:
        return 4, (shared + 4 * per_wave) * 8, False
    l = (shared + per_wave) * 8
    return 1, l, l > 64 * 1024


def rollout_kind(n, m, N, polish=True, stagewise=False):
    """blocked_exact | blocked_general | stagewise_tail | separate4 | separate1, and the dynamic-LDS flag"""
    L = polish_layout(n, m, N, stagewise)
    if polish and L["fused"]:
        s, _ = roll_block(n, m, N, stagewise)
        if s > 0:
            return ("blocked_exact" if roll_exact(n, m, s) else "blocked_general"), False
        return "stagewise_tail", False
    k, _, dyn = separate_rollout(n, m, N)
    return "separate%d" % k, dyn


# ---------------------------------------------------------------------------- the cases
class Case:
    def __init__(self, n, m, N, amp=3.0, seed=0, heavy=False, batches=(BATCH,), tags=(), xref_glb=False):
        self.n, self.m, self.N, self.amp, self.seed, self.heavy = n, m, N, amp, seed, heavy
        self.batches = tuple(batches)   # batches beyond the first: bit for bit the first rows of the batch-37 run
        self.tags = frozenset(tags)
        self.xref_glb = xref_glb        # per-instance references as well: the finish reads them from global memory
        self.exact = tuple(range(BATCH)) if heavy else tuple(range(0, BATCH, EXACT_STEP))

    nz = property(lambda s: s.m * s.N)
    nrb = property(lambda s: nrb_of(s.nz))
    nzs = property(lambda s: 16 * s.nrb)
    ks = property(lambda s: pick_ks(s.nz, s.nrb))
    build = property(lambda s: (s.nrb, s.ks))
    ksf = property(lambda s: (s.n + 3) // 4)
    shape = property(lambda s: (s.n, s.m, s.N))
    id = property(lambda s: "%d-%d-%d%s" % (s.n, s.m, s.N, "-heavy" if s.heavy else ""))
    route = property(lambda s: pick_route(*s.shape))                                   # the default route, finish on
    tile_route = property(lambda s: pick_route(*s.shape, no_shared_wave=True))        # ... with ALMPC_NO_SHARED_WAVE=1
    rollout = property(lambda s: rollout_kind(*s.shape))
    slot = property(lambda s: polish_layout(*s.shape)["slot"])
    block = property(lambda s: roll_block(*s.shape))

    def __repr__(self):
        return self.id


_B = (BATCH, 16, 1)
CASES = (
    # k_admm<1, 3>: nz 1 and 12 (one block, s = N)
    Case(1, 1, 1, batches=_B), Case(3, 2, 6, batches=_B, tags=("stagewise",)),
    # <1, 4>: nz 13 (m = 13: s = 1, exact fit) and 16 (n = 16: s = 4, every lane busy, N a multiple of s; ksf = 4)
    Case(2, 13, 1), Case(16, 2, 8, batches=_B, tags=("stagewise",)),
    # <2, 8>: nz 17 (n = 17: ksf = 5, k_rollout<4>; n = 64: k_rollout<1> below 64 KiB), 25 (m > 24: stage-wise tail), 32 (n = 1: s = 24)
    Case(17, 1, 17, tags=("separate", "freeze")), Case(64, 1, 17, tags=("separate",)), Case(2, 25, 1, batches=_B),
    Case(1, 1, 32, batches=_B, tags=("no_glds",)),
    # <3, 10>: nz 33 (n = 13: general fit) and 40 (n = 33: ksf = 9, k_rollout<4>)
    Case(13, 3, 11, batches=_B), Case(33, 2, 20, tags=("separate",)),
    # <3, 12>: nz 41 (N = 1 mod s, s = 10) and 48 (m = 24: s = 1, general fit)
    Case(6, 1, 41, tags=("stagewise",)), Case(3, 24, 2, batches=_B),
    # <4, 16>: nz 49 (N = 1 mod s, s = 3, general fit) and 64 (n = 16), and the heavy (4, 2, 32)
    Case(5, 7, 7, batches=_B), Case(16, 4, 16, batches=_B, tags=("no_glds",), xref_glb=True),
    Case(4, 2, 32, amp=10.0, heavy=True, tags=("sg_global",)),
    # <5, 20>: nz 65 (m = 13: s = 1, five blocks, exact fit) and 80
    Case(5, 13, 5, tags=("stagewise",)), Case(10, 2, 40, tags=("freeze",)),
    # <6, 24>: nz 81 and 96 (N a multiple of s = 8), and the heavy (6, 3, 30)
    Case(2, 9, 9), Case(7, 3, 32, tags=("no_glds",)), Case(6, 3, 30, amp=10.0, heavy=True, tags=("sg_global", "no_glds")),
    # <7, 28>: nz 97 (s = 21) and 112
    Case(3, 1, 97), Case(5, 4, 28),
    # <8, 30>: nz 113 (s * n = 64, N = 1 mod s) and 120 (the quadrotor: exact fit, s = 5, 60 lanes; n = 64: k_rollout<1>, dynamic LDS)
    Case(4, 1, 113, batches=_B, tags=("unfused", "freeze", "no_glds")), Case(12, 4, 30, batches=_B), Case(64, 2, 60, tags=("separate",)),
    # <8, 30> again: nz 116, m > 24 (the stage-by-stage rollout in the tail of the one-kernel step)
    Case(3, 29, 4, tags=("unfused",)),
    # (the shapes with m > 24 need amplitude 6 for active rows)
    # <8, 32>: nz 121 (no second-tier slot) and 123 (m > 24) in one kernel -- beyond nz 123 G beside the ADMM buffers outgrows the
    # 160 KB and the step is k_admm + k_polish<true> --, 125 (m > 24; heavy: no slot), 128 (m > 24; n = 16, N = 128: G and the
    # references outgrow LDS, k_polish<false> by default)
    Case(11, 11, 11, tags=("unfused",)), Case(3, 41, 3, amp=6.0, tags=("unfused",)), Case(2, 25, 5, amp=6.0), Case(7, 5, 25, amp=10.0, heavy=True, tags=("sg_global",)),
    Case(3, 32, 4, amp=6.0), Case(16, 1, 128),
    # the kr >= n + 9 boundary of the affine first iterate (N = 1: kr = 64)
    Case(55, 2, 1, tags=("affine",)), Case(56, 2, 1, tags=("full_first",)),
)
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)
REGULAR = tuple(c for c in CASES if not c.heavy)
HEAVY = tuple(c for c in CASES if c.heavy)
HEAVY_BANDS = {"4-2-32-heavy": (True, True), "6-3-30-heavy": (True, False), "7-5-25-heavy": (True, True)}   # 33..48, 49..60 populated
FREEZE_AMPS = (0.01, 3.0)           # alternate within each tile
FREEZE_OPTS = dict(max_iter=200, check_every=5)


def tagged(tag):
    return tuple(c for c in CASES if tag in c.tags)


def reached():
    """What the table claims to run: builds of k_admm, k_step_fused, k_step_inst_wave, k_polish (GLDS true / false), k_rollout"""
    out = dict(admm=set(), fused=set(), wave=set(), polish=set(), rollout=set())
    for c in CASES:
        routes = {c.route, c.tile_route}
        if "no_glds" in c.tags:
            routes.add(pick_route(*c.shape, no_glds=True, no_shared_wave=True))
        for r in routes:
            if r == "fused":
                out["fused"].add(c.build)   # (tests a, b and the unfused pairs run k_admm of the same build)
            elif r == "wave":
                out["wave"].add(next(z for z in WAVE_BUILDS if c.nzs <= z))
            else:
                out["polish"].add(r == "tile")
        out["admm"].add(c.build)            # finish off: every case runs k_admm (tests a and b)
        out["rollout"].add(separate_rollout(*c.shape)[0])   # ... and the separate rollout behind it
    return out


# ---------------------------------------------------------------------------- inputs and references
def problem(c):
    """The recipe of test_gpu_affine_first_iterate._problem: the quadrotor for (12, 4, 30); else a random plant of spectral radius
    0.97, bounds -0.5 / 0.7, an input-rate weight and a time-varying u_ref, so that fS and wS are not zero"""
    n, m, N = c.shape
    if c.shape == QUAD:
        return mo.quadrotor()
    rng = np.random.default_rng(7000 * n + 10 * m + N + 100000 * c.seed)
    A = rng.standard_normal((n, n))
    A *= 0.97 / np.max(np.abs(np.linalg.eigvals(A)))
    B = rng.standard_normal((n, m))
    u_ref = 0.05 * rng.standard_normal((m, 1)) + 0.03 * rng.standard_normal((m, N))
    u_min, u_max = -0.5 * np.ones(m), 0.7 * np.ones(m)
    if m > ROLL_SMX:   # the stage-by-stage tail reads the box per row of a pair: neighbouring inputs get different bounds
        u_min, u_max = u_min - 0.04 * (np.arange(m) % 3), u_max + 0.05 * (np.arange(m) % 3)
    return mo.make_problem(A, B, N, u_min, u_max, x_ref=0.1 * rng.standard_normal(n), u_ref=u_ref, q=10.0, r=1.0, s=0.5 if N > 2 else 0.0)


def x0(c, amp=None):
    amp = c.amp if amp is None else amp
    if c.shape == QUAD:
        return mo.quadrotor_x0_batch(BATCH, amp, first_instance=77)
    return amp * np.random.default_rng(c.n + c.N + 100000 * c.seed).standard_normal((BATCH, c.n))


def freeze_x0(c):
    """amplitudes 0.01 and 3 alternate within each tile: easy and hard instances freeze at different checks"""
    X0 = x0(c, 1.0)
    return X0 * np.where(np.arange(BATCH) % 2 == 0, FREEZE_AMPS[0], FREEZE_AMPS[1])[:, None]


def instance_refs(c, p):
    """per-instance references around the shared ones (xref_glb cases): x_ref constant over the horizon, u_ref time-varying"""
    rng = np.random.default_rng(31 * c.n + c.N)
    xr = p.x_ref[None] + 0.05 * rng.standard_normal((BATCH, c.n, 1)) * np.ones((1, 1, c.N + 1))
    ur = p.u_ref[None] + 0.04 * rng.standard_normal((BATCH, c.m, c.N))
    return xr, ur


def with_refs(p, x_ref, u_ref):
    """the problem with other references (same weights and bounds)"""
    import copy
    q = copy.copy(p)
    q.x_ref, q.u_ref = np.array(x_ref), np.array(u_ref)
    return q


def exact_batch(p, X0, which):
    """{i: rollout of the exact solution} (solve_mpc_exact's box-only branch with the condensing done once)"""
    _, _, H, F = mo.condense(p)
    fS = mo.s_rate_gradient(p)
    lo = (p.u_min[:, None] - p.u_ref).T.reshape(-1)
    hi = (p.u_max[:, None] - p.u_ref).T.reshape(-1)
    return {i: mo.rollout(p, X0[i], mo.solve_box_qp_exact(H, F @ (X0[i] - p.x_ref[:, 0]) + fS, lo, hi)) for i in which}


def active_rows(p, u):
    return int((np.isclose(u, p.u_min[:, None], rtol=0, atol=1e-12) | np.isclose(u, p.u_max[:, None], rtol=0, atol=1e-12)).sum())


@functools.lru_cache(maxsize=None)
def reference(c):
    """dict(p, X0, exact {i: rollout dict} of the compared instances, nact: active rows of the exact solution of EVERY instance) of a
    case, computed once per process and read-only for every test that uses it"""
    p, X0 = problem(c), x0(c)
    every = exact_batch(p, X0, range(BATCH))
    return dict(p=p, X0=X0, exact={i: every[i] for i in c.exact}, nact=np.array([active_rows(p, every[i]["u"]) for i in range(BATCH)]))


@functools.lru_cache(maxsize=None)
def reference_glb(c):
    """the same with per-instance references: dict(p, X0, refs (xr, ur), exact {i: rollout dict})"""
    p, X0 = problem(c), x0(c)
    xr, ur = instance_refs(c, p)
    exact = {}
    for i in c.exact:
        exact.update(exact_batch(with_refs(p, xr[i], ur[i]), X0, (i,)))
    return dict(p=p, X0=X0, refs=(xr, ur), exact=exact)


# ---------------------------------------------------------------------------- the ADMM iteration, chained (warm start) and traced
def admm(des, fs, x=None, z=None, y=None, alpha=1.6, eps_abs=1e-3, eps_rel=1e-3, max_iter=25, check_every=25, trace=None):
    """mpc_oracle.admm_box on a design of mpc_oracle.design_shared, from a given (x, z, y): z is clipped to the bounds as admm_body
    does with a stored state.  trace (a list): (primal residual, its threshold, dual residual, its threshold) of every check."""
    Hs, Minv, lo, hi, d, rho, sigma = des["Hs"], des["Minv"], des["lo"], des["hi"], des["d"], des["rho_vec"], des["sigma"]
    nz = fs.size
    x = np.zeros(nz) if x is None else x.copy()
    y = np.zeros(nz) if y is None else y.copy()
    z = np.zeros(nz) if z is None else np.clip(z, lo, hi)
    status, it = 1, 0
    for it in range(1, max_iter + 1):
        xt = Minv @ (sigma * x - fs + rho * z - y)
        x = alpha * xt + (1 - alpha) * x
        w = alpha * xt + (1 - alpha) * z + y / rho
        zn = np.clip(w, lo, hi)
        y = rho * (w - zn)
        z = zn
        if it % check_every == 0 or it == max_iter:
            Hx = Hs @ x
            rp, rd = np.max(np.abs(d * (x - z))), np.max(np.abs((Hx + fs + y) / d))
            tp = eps_abs + eps_rel * max(np.max(np.abs(d * x)), np.max(np.abs(d * z)))
            td = eps_abs + eps_rel * max(np.max(np.abs(Hx / d)), np.max(np.abs(y / d)), np.max(np.abs(fs / d)))
            if trace is not None:
                trace.append((rp, tp, rd, td))
            if rp <= tp and rd <= td:
                status = 0
                break
    return dict(x=x, z=z, y=y, iters=it, status=status)


def admm_u(p, des, r):
    """the inputs of an iterate: u = clip(d z + u_ref), (m, N)"""
    v = (r["z"] * des["d"]).reshape(p.N, p.m).T
    return np.clip(v + p.u_ref, p.u_min[:, None], p.u_max[:, None])


def fs_of(p, des, x0_):
    return des["Fs"] @ (np.asarray(x0_, dtype=np.float64) - p.x_ref[:, 0]) + des["fS"]
