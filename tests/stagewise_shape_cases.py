"""The shapes at which the stage-wise solvers are tested: one table for tests/test_stagewise_shape_cases.py (CPU: the table covers every
instantiated build and its inputs are well posed) and tests/test_gpu_stagewise_shapes.py (GPU: k_sdual and k_riccati against the oracles).

k_sdual (csrc/almpc_sdual.hip.h) is instantiated once per pair of SD_SHAPES (csrc/almpc_api.hip); sdual_pick_shape(nt, m) takes the
first pair that covers (nt, m), nt = n, or n + m with an input-rate weight S.  A lane owns one slot of a stage for every G-th stage,
G = 64 / (NT + MC); the working-set mask has one bit per lane and slot, so the horizon ends at N = 64 G - 1 (sdual_shape_ok)."""
import functools

import numpy as np

import mpc_oracle as mo
import stagewise_oracle as so

SD_SHAPES = ((2, 2), (4, 2), (6, 2), (8, 4), (12, 4), (16, 4), (16, 8), (32, 16), (48, 16))
RICCATI_SHAPES = ((12, 4), (4, 2), (2, 1))     # the specialised builds of k_riccati; every other shape takes the generic one
FEATURES = ("ubox", "xbox", "eq", "xbox_eq")   # input box alone / + state box / + terminal equality / + both
BATCH = 37                                     # no multiple of the waves per workgroup
EXACT_STEP = 3                                 # every third instance against the exact oracle ...
RESTATED = (1, 12, 23, 36)                     # ... and these four against the restatement of the kernel's algorithm
XBOX = 2.0


def pick_build(nt, m):
    for NT, MC in SD_SHAPES:
        if nt <= NT and m <= MC:
            return (NT, MC)
    return None


def G_of(build):
    return 64 // (build[0] + build[1])


def n_max(build):
    return 64 * G_of(build) - 1


class Case:
    def __init__(self, n, m, N, S, feat, amp, seed=0, xbox=XBOX, batch=BATCH, exact=None, pull=False):
        self.pull = pull   # the references of the last stage lie outside the bounds: rows of the last stage are active
        self.n, self.m, self.N, self.S, self.feat, self.amp, self.seed, self.xbox, self.batch = n, m, N, bool(S), feat, amp, seed, xbox, batch
        self.exact = tuple(range(0, batch, EXACT_STEP)) if exact is None else tuple(exact)   # instances held against the exact oracle
        self.restated = tuple(i for i in RESTATED if i < batch)                              # ... against the restatement

    @property
    def nt(self):
        return self.n + self.m if self.S else self.n

    @property
    def build(self):
        return pick_build(self.nt, self.m)

    @property
    def exact_fit(self):
        return (self.nt, self.m) == self.build

    @property
    def padded(self):
        return self.nt < self.build[0] and self.m < self.build[1]

    @property
    def has_xbox(self):
        return self.feat in ("xbox", "xbox_eq")

    @property
    def has_eq(self):
        return self.feat in ("eq", "xbox_eq")

    @property
    def id(self):
        return f"{self.n}-{self.m}-{self.N}{'-S' if self.S else ''}-{self.feat}"

    @property
    def compared(self):
        return sorted(set(self.exact) | set(self.restated))


def plant(n, m, N, S, feat="ubox", seed=0, xbox=XBOX, pull=False):
    """A random plant with spectral radius 0.97 (as test_random_stable_plants_of_many_shapes), bounds tight enough to be active,
    non-zero references.  pull: the input reference of the last stage and the state reference of the terminal stage lie outside
    the bounds, so that the last input and (with a state box) the terminal state end on a bound -- the rows with the highest
    coordinates of the trajectory.  Returns the problem and the generator, which the caller draws the initial states from."""
    rng = np.random.default_rng(1000 * n + 10 * m + N + 100000 * seed)
    A = rng.standard_normal((n, n))
    A *= 0.97 / np.max(np.abs(np.linalg.eigvals(A)))
    B = rng.standard_normal((n, m))
    kw = {}
    if feat in ("xbox", "xbox_eq"):
        kw.update(x_min=-xbox * np.ones(n), x_max=xbox * np.ones(n))
    if feat in ("eq", "xbox_eq"):
        kw.update(terminal="equality")
    x_ref, u_ref = 0.1 * rng.standard_normal(n), 0.05 * rng.standard_normal(m)
    if pull:
        x_ref, u_ref = np.tile(x_ref[:, None], (1, N + 1)), np.tile(u_ref[:, None], (1, N))
        if feat == "xbox":
            x_ref[0, N] = 1.5 * xbox
        u_ref[0, N - 1] = 0.75 if feat == "eq" else 1.0   # (u_max = 0.7; the terminal equality leaves the last inputs little room)
    p = mo.make_problem(A, B, N, -0.5 * np.ones(m), 0.7 * np.ones(m), x_ref=x_ref, u_ref=u_ref, q=10.0, r=1.0, s=0.5 if S else 0.0, **kw)
    return p, rng


def inputs(c):
    """(problem, X0) of a case; with a state box the initial states lie inside it, so that an infeasible instance is the solver's
    verdict and not the first stage's"""
    p, rng = plant(c.n, c.m, c.N, c.S, c.feat, c.seed, c.xbox, c.pull)
    X0 = c.amp * rng.standard_normal((c.batch, c.n))
    if c.has_xbox:
        X0 = np.clip(X0, -0.99 * c.xbox, 0.99 * c.xbox)
    return p, X0


def _c(n, m, N, S, feats, amp=3.0, eq_amp=1.0, **kw):
    return [Case(n, m, N, S, f, eq_amp if f in ("eq", "xbox_eq") else amp, **kw) for f in feats]


ALL = FEATURES
REST = ("ubox", "eq", "xbox_eq")
# Seeds, amplitudes and boxes other than the defaults: chosen on the CPU so that the state-box cases hold both a solved instance with
# an active state bound and an infeasible one (test_stagewise_shape_cases.py); a plant with n = 1 and spectral radius 0.97 cannot
# leave a box it starts in, so the n = 1 shapes carry no state box.
CASES = (
    # (2, 2): G = 16
    _c(1, 1, 1, 0, ("ubox",)) + _c(2, 2, 9, 0, REST) + _c(2, 2, 9, 0, ("xbox",), amp=6.0, seed=1) + _c(1, 1, 5, 1, ("ubox",))
    # (4, 2): G = 10
    + _c(4, 1, 11, 0, ("ubox",)) + _c(4, 1, 11, 0, ("xbox",), amp=6.0, xbox=1.0)
    + _c(2, 1, 7, 1, ("ubox",)) + _c(2, 1, 7, 1, ("xbox",), amp=1.0, xbox=0.5) + _c(4, 2, 9, 0, ("eq", "xbox_eq"))
    # (6, 2): G = 8
    + _c(6, 1, 10, 0, ("ubox",)) + _c(4, 1, 7, 1, ("ubox",)) + _c(4, 1, 7, 1, ("xbox",), amp=6.0)
    + _c(4, 2, 9, 1, REST) + _c(4, 2, 9, 1, ("xbox",), amp=6.0, xbox=1.0)
    # (8, 4): G = 5
    + _c(7, 3, 10, 0, ALL) + _c(5, 3, 9, 1, ("ubox", "xbox")) + _c(4, 4, 6, 1, ("ubox", "xbox_eq"))
    # (12, 4): G = 4
    + _c(9, 3, 12, 0, ALL) + _c(9, 4, 12, 0, ("ubox",)) + _c(8, 4, 8, 1, ALL)
    # (16, 4): G = 3, the first build whose sweep goes through LDS (NT + MC > 16)
    + _c(13, 3, 9, 0, ALL) + _c(16, 4, 8, 0, ("ubox", "eq")) + _c(12, 4, 8, 1, ("ubox", "xbox", "xbox_eq"))
    # (16, 8): G = 2
    + _c(11, 5, 8, 0, ALL) + _c(16, 8, 6, 0, ("ubox", "xbox", "eq")) + _c(8, 8, 6, 1, ("ubox", "xbox_eq"))
    # (32, 16): G = 1, lanes 48..63 idle
    + _c(17, 3, 8, 0, ("ubox",)) + _c(17, 3, 8, 0, ("xbox",), amp=1.0) + _c(20, 9, 6, 0, ALL) + _c(32, 16, 5, 0, REST)
    + _c(16, 16, 5, 1, ("ubox",)) + _c(16, 16, 5, 1, ("xbox",), amp=6.0, xbox=4.0) + _c(24, 8, 6, 1, ("eq", "xbox_eq"))
    # (48, 16): G = 1, a stage fills the wave; on a structured handle (n <= 32) only with S
    + _c(30, 7, 6, 1, ("ubox", "xbox")) + _c(32, 16, 4, 1, REST) + _c(32, 16, 4, 1, ("xbox",), amp=6.0, xbox=0.5)
    + _c(30, 12, 5, 1, ("eq", "xbox_eq"))
)

# the horizon edge N = 64 G - 1 at G = 1 and G = 2, four instances each.  Bit 63 of the working-set mask belongs to the stages
# 64 G - G .. N: at G = 1 to the terminal state alone (a terminal equality, or a state bound that is active there), at G = 2 to
# the last input as well -- hence `pull`
_E = dict(exact=RESTATED, pull=True)
EDGE_CASES = (
    _c(17, 1, 63, 0, ("ubox",), **_E) + _c(17, 1, 63, 0, ("xbox",), amp=1.0, **_E) + _c(20, 4, 63, 0, ("eq",), **_E)
    + _c(30, 2, 63, 1, ("ubox",), **_E) + _c(13, 5, 127, 0, ("ubox",), **_E) + _c(13, 5, 127, 0, ("xbox",), amp=1.0, **_E)
    + _c(13, 5, 127, 0, ("eq",), **_E)
)
# k_riccati as the first solver (input box only): the specialised builds, each also through the generic one, and generic-only shapes
RICCATI_CASES = (Case(12, 4, 30, 0, "ubox", 3.0), Case(4, 2, 20, 0, "ubox", 3.0), Case(2, 1, 10, 0, "ubox", 3.0),
                 Case(7, 3, 10, 0, "ubox", 3.0), Case(20, 9, 6, 0, "ubox", 3.0), Case(32, 16, 8, 0, "ubox", 3.0))
# one case per build for the kernel variant without cached responses (the records stay resident in registers): the richest feature
# set.  The two G = 1 builds are NOT in these lists: k_sdual<32, 16, 1, false, false> solving 20-9-6-xbox_eq under ALMPC_SDUAL_NO_GHAT
# ended with a GPU memory fault ("an illegal memory access was encountered") whose cause is not found; neither
# that build nor the (48, 16) one (more registers still) is run as a solver again before it is -- that also keeps per-instance models
# with n + m > 24, whose solves take the same build, out of the GPU tests.
VARIANT_CASES = ("2-2-9-xbox_eq", "4-2-9-xbox_eq", "4-2-9-S-xbox_eq", "7-3-10-xbox_eq", "9-3-12-xbox_eq", "13-3-9-xbox_eq", "11-5-8-xbox_eq",
                 "8-8-6-S-xbox_eq")
WIDE_CASES = ("11-5-8-xbox_eq",)                                           # (16, 8): the table built but not used (ALMPC_SDUAL_NO_GH)
SCREEN_CASES = ("11-5-8-xbox", "20-9-6-xbox", "30-7-6-S-xbox")             # G = 2 and G = 1: infeasible instances among them
# capacity tiers (32 / 64 / 128 rows) at the wide builds: (case, a working set above `above` rows exists, one within 32 exists)
TIER_CASES = ((Case(32, 16, 5, 0, "ubox", 10.0, exact=range(BATCH)), 32, True), (Case(16, 8, 12, 0, "ubox", 10.0, exact=range(BATCH)), 32, True),
              (Case(32, 16, 5, 0, "ubox", 40.0, exact=range(BATCH)), 64, False), (Case(16, 8, 12, 0, "ubox", 40.0, exact=range(BATCH)), 64, False),
              (Case(32, 16, 7, 1, "ubox", 40.0, exact=range(BATCH)), 96, False))
CASE_BY_ID = {c.id: c for c in CASES}


def active_inputs(p, u):
    return int(((u >= p.u_max[:, None] - 1e-12) | (u <= p.u_min[:, None] + 1e-12)).sum())


def active_states(p, x):
    if p.x_min is None:
        return 0
    return int(((x[:, 1:] >= p.x_max[:, None] - 1e-9) | (x[:, 1:] <= p.x_min[:, None] + 1e-9)).sum())


def exact_or_none(p, x0):
    """the exact oracle's solution, None for an infeasible problem (ValueError); a RuntimeError (no certificate) is the caller's failure"""
    try:
        return mo.solve_mpc_exact(p, x0)
    except ValueError:
        return None


def restate(p, x0):
    """solve_mpc_stagewise + first_tier: the working set never outgrew the 32 rows of k_sdual's first launch, so the kernel decides
    in one launch and its count of working-set changes equals the restatement's"""
    r = so.solve_mpc_stagewise(p, x0, wcap=32)
    first_tier = r["status"] != 1
    if not first_tier:
        r = so.solve_mpc_stagewise(p, x0)
    return dict(r, first_tier=first_tier)


@functools.lru_cache(maxsize=None)
def reference(c):
    """Both oracles on the compared instances of a case, computed once per process and read-only for every test that uses it:
    dict(p, X0, exact {i: solution | None}, restated {i: solve_mpc_stagewise's output + first_tier})."""
    p, X0 = inputs(c)
    exact = {i: exact_or_none(p, X0[i]) for i in c.exact}
    restated = {i: restate(p, X0[i]) for i in c.restated}
    return dict(p=p, X0=X0, exact=exact, restated=restated)
