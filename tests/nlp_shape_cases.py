"""The shapes at which the black-box (NLP) family is tested beyond the 4-2-16x2 model: the network linearisation (k_fnn_jacobian_w,
k_fnn_jacobian), the time-varying design (k_design_ltv_reg, k_design_ltv), the SQP loop and its glue (k_fnn_rollout, k_sqp_prepare,
k_sqp_step, k_sqp_kkt), the exact-Hessian mode (k_fnn_lag_hessian, k_sqp_exact_qp) and the re-linearisation pipeline with the Jacobian as
the head of k_design_instance_t.  One table for tests/test_nlp_shape_cases.py (CPU: the table reaches every build, the restated
dispatch is the source's, the references are well posed) and tests/test_gpu_nlp_shapes.py (GPU: the kernels against the references).

The host's decisions -- launch_fnn_jacobian, ltv_reg_path, launch_design_ltv, design_fuses_fnn, sqp_exact_check (csrc/almpc_api.hip),
fnn_weights_doubles, fnn_wave_scratch_doubles, fnn_w_lds_doubles (csrc/almpc_fnn.hip.h), sqp_step_chunk, sqp_step_lds_doubles,
fnn_hess_wave_doubles, sqp_exact_lds_doubles (csrc/almpc_sqp.hip.h), design_ltv_lds_doubles, design_ltv_reg_lds_doubles
(csrc/almpc_instance.hip.h) -- are restated here in Python; the CPU test holds them against the source text.
A set of switches is a dict {ALMPC_*: value} as a handle's (or a linearisation call's) environment holds it."""
import functools

import numpy as np

import densenet_ref as dr
import instance_step_cases as ic
import mpc_oracle as mo
import net_ref as nr
import sqp_exact_ref as ex
import sqp_solve_ref as sref

# ---------------------------------------------------------------------------- constants of the source (checked by the CPU test)
KINDS = ("fnn", "resnet", "polynet", "densenet")
NET = {"fnn": 0, "resnet": 1, "polynet": 2, "densenet": 3}           # NET_* of csrc/almpc_fnn.hip.h
ACTS = ("tanh", "relu")
FNN_W_WAVES = 4
FNN_W_BUILDS = tuple((lw, net) for lw in (32, 64) for net in range(4))   # k_fnn_jacobian_w<LW, NET>
LTV_REG_BUILDS = (0, 2, 4, 6, 12)                                     # k_design_ltv_reg<NC, 4>
LTV_REG_NZ = 128
LDS_MAX = 160 * 1024
LDS_STATIC = 64 * 1024                                                # above it: ensure_dyn_lds
PPW2_MAX = 192                                                        # H (n + m) <= 192: two points per wave
WG_CAP_PER_CU = 8                                                     # k_fnn_jacobian_w: at most num_cus * 8 workgroups
NUM_CUS = ic.NUM_CUS                                                  # what the CPU test assumes; the GPU test asks the device
STEP_LDS_DOUBLES = 12288                                              # sqp_step_chunk: 96 KB of doubles
MARGIN = 1e-6                                                         # strict complementarity of every QP of a reference
SQP_ITERS = 4

ONE_POINT = {"ALMPC_FNN_ONE_POINT_PER_WAVE": "1"}
FNN_WG = {"ALMPC_FNN_WG": "1"}
LTV_LDS = {"ALMPC_LTV_LDS": "1"}
SPLIT_PREPARE = {"ALMPC_DBG_SPLIT_PREPARE": "1"}
SPLIT_SCALE = {"ALMPC_DBG_SPLIT_SCALE": "1"}
SPLIT_JACOBIAN = {"ALMPC_DBG_SPLIT_JACOBIAN": "1"}
on = ic.on


# ---------------------------------------------------------------------------- the linearisation
def densenet_wh_offset(H, l):
    return H * H * l * (l + 1) // 2


def fnn_weights_doubles(n, m, H, L, kind="fnn"):
    if kind == "densenet":
        return H * (n + m) + densenet_wh_offset(H, L) + L * H + n * (L + 1) * H
    return H * (n + m) + L * H * H + L * H + n * H


def fnn_wave_scratch_doubles(n, m, H, L, kind="fnn"):
    if kind == "densenet":
        return (L + 1) * H * (1 + n + m) + H + (n + m)
    return 2 * H + 2 * H * (n + m) + (n + m) + (H if kind == "polynet" else 0)


def fnn_w_lds_doubles(n, m, H, L, ppw=1, kind="fnn"):
    return fnn_weights_doubles(n, m, H, L, kind) + FNN_W_WAVES * ppw * fnn_wave_scratch_doubles(n, m, H, L, kind)


def lin_ppw(n, m, H, env=()):
    return 2 if H * (n + m) <= PPW2_MAX and not on(env, "ALMPC_FNN_ONE_POINT_PER_WAVE") else 1


def lin_supported(n, m, H, L, kind="fnn"):
    return fnn_wave_scratch_doubles(n, m, H, L, kind) * 8 <= LDS_MAX


def lin_build(n, m, H, L, kind="fnn", env=()):
    """launch_fnn_jacobian: ("w", LW, NET) the wave build | ("wg", NET, dyn) one workgroup per point, dyn: LDS above 64 KB"""
    ppw = lin_ppw(n, m, H, env)
    if fnn_w_lds_doubles(n, m, H, L, ppw, kind) * 8 <= LDS_STATIC and not on(env, "ALMPC_FNN_WG"):
        return ("w", 64 // ppw, NET[kind])
    return ("wg", NET[kind], fnn_wave_scratch_doubles(n, m, H, L, kind) * 8 > LDS_STATIC)


def lin_grid(points, ppw, num_cus=NUM_CUS):
    """(workgroups, passes of the grid-stride loop of the busiest wave, lanes of the last pass that store nothing)"""
    per_wg = FNN_W_WAVES * ppw
    wgs = min((points + per_wg - 1) // per_wg, num_cus * WG_CAP_PER_CU)
    stride = wgs * per_wg
    return wgs, (points + stride - 1) // stride, (-points) % ppw


def big_count(ppw, num_cus=NUM_CUS):
    """a full pass of the capped grid and five points of a second"""
    return num_cus * WG_CAP_PER_CU * FNN_W_WAVES * ppw + 5


# ---------------------------------------------------------------------------- the time-varying design
def design_ltv_lds_doubles(n, m, N):
    nz = m * N
    return nz * nz + 3 * n * nz + 4 * n * n + n * m + 3 * n + nz


def design_ltv_reg_lds_doubles(n, m, N):
    return 4 * n * LTV_REG_NZ + 4 * n * n + 2 * n * m + 4 * n + 2 * N * n + 2 * m * m


def ltv_reg_path(n, m, N, env=()):
    return (m * N <= LTV_REG_NZ and n * n + n * m <= 1024 - n and design_ltv_reg_lds_doubles(n, m, N) * 8 <= LDS_MAX
            and not on(env, "ALMPC_LTV_LDS"))


def ltv_build(n, m, N, env=()):
    """launch_design_ltv: ("reg", NC) | ("lds",) | None (ltv_supported fails)"""
    if ltv_reg_path(n, m, N, env):
        return ("reg", n if n in LTV_REG_BUILDS[1:] else 0)
    return ("lds",) if design_ltv_lds_doubles(n, m, N) * 8 <= LDS_MAX else None


def ltv_fused(n, m, N, env=(), exact=False):
    """sqp_plan: (the scaling as the tail of k_design_ltv_reg, k_sqp_prepare as its head)"""
    scales = not exact and ltv_reg_path(n, m, N, env) and m * N <= 128 and not on(env, "ALMPC_DBG_SPLIT_SCALE")
    return scales, scales and not on(env, "ALMPC_DBG_SPLIT_PREPARE")


# ---------------------------------------------------------------------------- the SQP glue and the exact mode
def sqp_step_chunk(n, m, N):
    E, fixed = n * n + n * m + n, (N + 1) * n + m * N + 16
    ch = (STEP_LDS_DOUBLES - fixed) // E
    return 1 if ch < 1 else min(ch, N)


def sqp_step_lds_doubles(n, m, N):
    return sqp_step_chunk(n, m, N) * (n * n + n * m + n) + (N + 1) * n + m * N + 16


def sqp_chunks(n, m, N):
    """the chunk lengths k_sqp_step / k_sqp_kkt walk"""
    ch = sqp_step_chunk(n, m, N)
    return [min(ch, N - k0) for k0 in range(0, N, ch)]


def sqp_supported(n, m, N, env=()):
    """what sqp_fnn_setup accepts"""
    return n <= 64 and sqp_step_lds_doubles(n, m, N) * 8 <= LDS_MAX and ltv_build(n, m, N, env) is not None


def step_supported(n, m, N):
    """what the step behind a per-instance QP (almpc_design_ltv -> almpc_calculate, every SQP iteration) accepts: the rollout in the
    finish's tail (polish_layout: L.fused)"""
    return ic.polish_layout(n, m, N)["fused"]


def fnn_hess_wave_doubles(n, m, H, L, kind="fnn"):
    nin, S = n + m, (2 * L if kind == "polynet" else L)
    if kind == "densenet":
        return nin + (2 * (L + 1) + 1) * H + (L + 1) * H * nin + 2 * S * H + S * H * nin
    return nin + 3 * H + H * nin + 2 * S * H + S * H * nin


def sqp_exact_lds_doubles(n, m, nz):
    nin = n + m
    return 2 * n * nz + 2 * n + nin * nz + nin + nin * nin + n * n + n * m + n + 8


def exact_supported(kind, n, m, H, L, N, act="tanh"):
    """sqp_exact_check on a condensed handle without state rows"""
    return (act != "relu" and m * N <= 128 and 4 * fnn_hess_wave_doubles(n, m, H, L, kind) * 8 <= LDS_STATIC
            and sqp_exact_lds_doubles(n, m, m * N) * 8 <= LDS_STATIC)


# ---------------------------------------------------------------------------- the re-linearisation
def design_fuses_fnn(n, m, N, H, L, kind="fnn", env=()):
    if kind != "fnn":
        return False
    lds = ic.design_instance_lds_doubles(n, m, N) + fnn_weights_doubles(n, m, H, L) + fnn_wave_scratch_doubles(n, m, H, L)
    return lds * 8 <= LDS_MAX and not on(env, "ALMPC_DBG_SPLIT_JACOBIAN")


design_build = ic.design_build


# ---------------------------------------------------------------------------- the cases
class Case:
    """One row: family (lin | ltv | sqp | exact | relin), the network (kind, n, m, H, L, act), the horizon N, the batch (lin: the number
    of points; None: big_count of the device), the sets of switches it runs under beside none, and what was chosen for its inputs
    (seed, amp: the spread of x0 / xbar, ub: the half-width of the input box) so that its reference meets the conditions of
    tests/test_nlp_shape_cases.py."""

    def __init__(self, family, n, m, N=0, kind="fnn", H=0, L=0, act="tanh", batch=3, envs=(), seed=0, amp=0.5, ub=0.3, tags=(), big=0):
        self.family, self.kind, self.n, self.m, self.H, self.L, self.N, self.act = family, kind, n, m, H, L, N, act
        self.batch, self.seed, self.amp, self.ub, self.big = batch, seed, amp, ub, big
        self.envs = tuple(dict(e) for e in envs)
        self.tags = frozenset(tags)

    nz = property(lambda s: s.m * s.N)
    shape = property(lambda s: (s.n, s.m, s.N))
    net = property(lambda s: (s.n, s.m, s.H, s.L))

    @property
    def id(self):
        out = self.family
        if self.family != "ltv":
            out += "-%s-%d-%d-%dx%d-%s" % (self.kind, self.n, self.m, self.H, self.L, self.act)
        else:
            out += "-%d-%d" % (self.n, self.m)
        if self.N:
            out += "-N%d" % self.N
        out += "-big%d" % self.big if self.big else "-b%d" % self.batch
        return out + "".join("-" + t for t in sorted(self.tags))

    def __repr__(self):
        return self.id

    def points(self, num_cus=NUM_CUS):
        return big_count(self.big, num_cus) if self.big else self.batch

    def all_envs(self):
        return [{}] + [e for e in self.envs]


def env_id(env):
    return ic._env_id(env)


# ---- linearisation: (n, m, H, L), points, the measured gap of the float64 restatement to long double (largest over the four kinds and
# both activations, relative to the largest entry of A, B, f; tests/test_nlp_shape_cases.py re-measures it) -- the tolerance of a row is
# max(1e-12, 16 gap)
LIN_SHAPES = (
    # (n, m, H, L), points, gap        what the row is for
    ((1, 1, 4, 3), 4, 6e-16),        # w<32>, three layers
    ((3, 1, 5, 1), 1, 2e-16),        # w<32>, one point: the other half-wave stores nothing
    ((3, 1, 5, 1), 3, 1.1e-15),
    ((3, 1, 5, 1), 7, 2.6e-16),
    ((2, 3, 70, 1), 4, 7e-16),       # weights + 4 scratches above 64 KB: the workgroup build, H > 64
    ((6, 2, 33, 2), 5, 4.2e-16),     # w<64>, H no multiple of the lanes, five points on four waves
    ((12, 4, 16, 1), 4, 3.5e-16),    # w<64>, H (n + m) = 256
    ((5, 2, 8, 0), 4, 2.6e-16),      # no hidden layer
    ((30, 6, 5, 1), 3, 2.6e-16),     # w<32>, n + m = 36 > 32 lanes
    ((2, 1, 260, 1), 2, 1.8e-15),    # workgroup build, H > 256 threads
    ((2, 1, 70, 1), 5, 1.6e-15),     # w<64> with H > 64: a second trip with a partial tail
    ((1, 1, 40, 1), 3, 7e-16),       # w<32> with H > 32: the same on a half-wave
    ((12, 4, 300, 0), 2, 8e-16),     # workgroup build above 64 KB of LDS (ensure_dyn_lds)
)
LIN_GAP = {(s, p): g for s, p, g in LIN_SHAPES}
LIN_ENVS = (ONE_POINT, FNN_WG)
LIN = tuple(Case("lin", n, m, kind=k, H=H, L=L, act=a, batch=p, envs=LIN_ENVS)
            for (n, m, H, L), p, _ in LIN_SHAPES for k in KINDS for a in ACTS)
# the grid-stride loop's second, partial pass: a (2, 1, 4, 1) network, two points per wave and (ALMPC_FNN_ONE_POINT_PER_WAVE) one
LIN_BIG = tuple(Case("lin", 2, 1, kind=k, H=4, L=1, act="tanh", big=ppw, envs=(ONE_POINT,) if ppw == 1 else ()) for k in KINDS for ppw in (2, 1))
LIN_BIG_GAP = 5.1e-16


def lin_tol(c):
    return max(1e-12, 16 * (LIN_BIG_GAP if c.big else LIN_GAP[(c.net, c.batch)]))


# ---- time-varying design: c_all, S and a non-diagonal P; seed, amp chosen so that every QP has an input on a bound and is strictly
# complementary with margin (smallest multiplier / slack recorded by tests/test_nlp_shape_cases.py)
def _ltv(n, m, N, **kw):
    envs = (LTV_LDS,) if design_ltv_lds_doubles(n, m, N) * 8 <= LDS_MAX else ()
    return Case("ltv", n, m, N, batch=4, envs=envs, **kw)


LTV = (
    _ltv(2, 1, 1, amp=3.0), _ltv(2, 1, 2, amp=3.0), _ltv(2, 1, 3, amp=3.0),      # <2, 4>: the N > 1, N > 2, k + 3 < N edges of the prefetch
    _ltv(2, 4, 32),                                                # <2, 4>, nz 128
    _ltv(4, 2, 3, amp=2.0),                                        # <4, 4>, nz 6: ni = 1
    _ltv(4, 4, 32),                                                # <4, 4>, nz 128
    _ltv(4, 3, 7),                                                 # <4, 4>, m does not divide 32
    _ltv(6, 8, 16),                                                # <6, 4>, nz 128
    _ltv(6, 1, 5, amp=2.0),                                        # <6, 4>, nz 5
    _ltv(12, 4, 1, amp=1.5), _ltv(12, 4, 2, amp=1.5), _ltv(12, 4, 3, amp=1.5),               # <12, 4>: the prefetch edges
    _ltv(5, 3, 42),                                                # <0, 4>, nz 126
    _ltv(7, 2, 64),                                                # <0, 4>, nz 128
    _ltv(4, 3, 7, tags=("plain",)),                                # c_all = None, S = None
    _ltv(6, 1, 5, amp=2.0, tags=("pinst",)),                       # one P per instance
)


# ---- the SQP loop (Gauss-Newton, four iterations; the strided-group linearisation with ppi = N)
SQP_ENVS = (SPLIT_PREPARE, SPLIT_SCALE, LTV_LDS)


def _sqp(kind, n, m, H, L, N, **kw):
    return Case("sqp", n, m, N, kind=kind, H=H, L=L, batch=3, envs=SQP_ENVS, **kw)


SQP = (
    _sqp("fnn", 16, 1, 8, 1, 59, tags=("chunked",)),       # k_sqp_step in chunks of 39 + 20, above 64 KB of LDS; <0, 4>
    _sqp("resnet", 16, 1, 8, 1, 59, ub=0.5, tags=("chunked",)),
    _sqp("fnn", 2, 4, 12, 1, 32),                          # <2, 4> at nz 128
    _sqp("polynet", 6, 8, 20, 2, 16),                      # <6, 4> at nz 128
    _sqp("densenet", 12, 4, 16, 1, 8),                     # <12, 4>
    _sqp("fnn", 3, 1, 5, 1, 12, amp=1.0, ub=0.05),                        # <0, 4>, nz 12
    _sqp("resnet", 1, 1, 4, 3, 7, amp=1.0, ub=0.03),                      # n = m = 1
)
SOLVE_ITERS, SOLVE_TOL = 30, 1e-6
# (24, 1, 8, 1, 30) -- a chunk of 18 inside every limit of sqp_fnn_setup -- and (17, 1, 8, 1, 12) are set up and then refused by the first
# iteration: the finish of a per-instance QP rolls the stages out with n + m <= 8 g lanes, g the largest power of two with g n <= 64,
# which no n above 16 meets (step_supported).  With n <= 16 and m N <= 128 no walk is chunked up to N = 36 ((16, 3, 37) walks 36 + 1): hence (16, 1, 59), 39 + 20, above.
SQP_REFUSED = (_sqp("fnn", 24, 1, 8, 1, 30, tags=("refused",)), _sqp("fnn", 17, 1, 8, 1, 12, tags=("refused",)))

# ---- the exact Hessian's first QP; the last row is refused (the PolyNet's 2 L activation sites do not fit 16 KB per wave)
EXACT = tuple(Case("exact", n, m, N, kind=k, H=H, L=L, batch=3)
              for (n, m, H, L, N) in ((2, 3, 70, 1, 9), (6, 2, 33, 2, 16), (16, 1, 8, 1, 59)) for k in KINDS) + (
    Case("exact", 6, 2, 16, kind="fnn", H=33, L=3, batch=3), Case("exact", 6, 2, 16, kind="polynet", H=33, L=3, batch=3, tags=("refused",)))

# ---- the re-linearisation pipeline (Fnn): the Jacobian as the head of k_design_instance_t, and in front of it
RELIN = tuple(Case("relin", n, m, N, kind="fnn", H=H, L=L, batch=6, envs=(SPLIT_JACOBIAN,), ub=0.15)
              for (n, m, H, L, N) in ((12, 4, 16, 1, 10), (2, 1, 8, 2, 12), (3, 2, 33, 1, 9), (4, 2, 16, 2, 10)))

CASES = LIN + LIN_BIG + LTV + SQP + SQP_REFUSED + EXACT + RELIN
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


def reached():
    """What the table claims to run, derived from the rules above"""
    out = dict(lin_w=set(), lin_wg=set(), lin_passes=set(), lin_idle_half=set(), ltv_reg=set(), ltv_lds=set(), ltv_fused=set(),
               rollout=set(), step_chunks=set(), step_dyn=set(), lag_hessian=set(), relin=set())
    for c in CASES:
        for env in c.all_envs():
            if c.family in ("lin", "sqp", "exact") or (c.family == "relin" and not design_fuses_fnn(*c.shape, c.H, c.L, c.kind, env)):
                b = lin_build(*c.net, c.kind, env)
                if b[0] == "w":
                    out["lin_w"].add(b[1:])
                    pts = c.points() if c.family == "lin" else c.batch * (c.N if c.family != "relin" else 1)
                    g = lin_grid(pts, 64 // b[1])
                    out["lin_passes"].add((b[1], g[1]))
                    out["lin_idle_half"].add((b[1], g[2]))
                else:
                    out["lin_wg"].add(b[1:])
            if c.family in ("ltv", "sqp", "exact"):
                b = ltv_build(*c.shape, env)
                if b[0] == "reg":
                    out["ltv_reg"].add(b[1])
                    if c.family == "sqp":
                        out["ltv_fused"].add((b[1],) + ltv_fused(*c.shape, env))
                else:
                    out["ltv_lds"].add(c.family)
            if "refused" in c.tags and c.family == "sqp":
                continue
            if c.family in ("sqp", "exact"):
                out["rollout"].add(NET[c.kind])
                out["step_chunks"].add(len(sqp_chunks(*c.shape)) > 1)
                out["step_dyn"].add(sqp_step_lds_doubles(*c.shape) * 8 > LDS_STATIC)
            if c.family == "exact" and "refused" not in c.tags:
                out["lag_hessian"].add(NET[c.kind])
            if c.family == "relin":
                out["relin"].add((design_build(c.n, c.m), design_fuses_fnn(*c.shape, c.H, c.L, c.kind, env)))
    return out


# ---------------------------------------------------------------------------- networks and inputs
@functools.lru_cache(maxsize=None)
def _weights(n, m, H, L):
    return mo.synthetic_fnn(n=n, m=m, H=H, L=L, act="tanh")


@functools.lru_cache(maxsize=None)
def network(kind, n, m, H, L, act):
    """the model of a case: mo.synthetic_fnn's weights for the shape in the kind's recurrence (dr.synthetic_densenet's for a DenseNet),
    W_out rescaled to a spectral radius of 0.95 of A at the origin"""
    if kind == "densenet":
        return dr.synthetic_densenet(n=n, m=m, H=H, L=L, seed=0x5EED0004 + 64 * H + L, act=act)
    f = nr.as_kind(_weights(n, m, H, L), kind)
    f.act = act
    A0, _ = f.jacobian(np.zeros(n), np.zeros(m))
    f.W_out = f.W_out * (0.95 / max(1e-12, float(np.max(np.abs(np.linalg.eigvals(A0))))))
    return f


def model(c):
    return network(c.kind, c.n, c.m, c.H, c.L, c.act)


def lin_points(c, num_cus=NUM_CUS):
    """x (p, n), u (p, m): pre-activations on both sides of the relu kinks"""
    p = c.points(num_cus)
    r = np.random.default_rng(1000 * c.n + 10 * c.H + c.L + p)
    return 1.5 * r.standard_normal((p, c.n)), 1.5 * r.standard_normal((p, c.m))


def lin_reference(c, num_cus=NUM_CUS, dtype=np.float64):
    """(A, B, f) of every point: the float64 restatement over all points at once (dtype: long double for its yardstick)"""
    x, u = lin_points(c, num_cus)
    return dr.evaluate_points(model(c), x, u, dtype)


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- time-varying design
@functools.lru_cache(maxsize=None)
def ltv_inputs(c):
    """dict of design_ltv's arguments (as test_ltv_design_kernels_both_builds makes them), read-only"""
    n, m, N = c.shape
    b = c.batch
    rng = np.random.default_rng(n * 100 + N + 7919 * m + 100000 * c.seed)
    A_all = np.stack([[0.85 * np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n) for _ in range(N)] for _ in range(b)])
    B_all = rng.standard_normal((b, N, n, m))
    c_all = 0.05 * rng.standard_normal((b, N, n))
    xbar = c.amp * 2.0 * rng.standard_normal((b, n, N + 1)); ubar = 0.2 * rng.standard_normal((b, m, N))
    x_ref = 0.2 * rng.standard_normal((n, N + 1)); u_ref = 0.1 * rng.standard_normal((m, N))
    Q, R, S, P = 10.0 * np.eye(n), 1.0 * np.eye(m), 0.3 * np.eye(m), 25.0 * np.eye(n) + 0.2 * np.ones((n, n))
    if "plain" in c.tags:
        c_all, S = None, None
    if "pinst" in c.tags:
        P = np.stack([(20.0 + 3.0 * i) * np.eye(n) + 0.1 * (i + 1) * np.ones((n, n)) for i in range(b)])
    out = dict(A_all=A_all, B_all=B_all, c_all=c_all, xbar=xbar, ubar=ubar, x_ref=x_ref, u_ref=u_ref, Q=Q, R=R, S=S, P=P,
               umin=-0.5 * np.ones(m), umax=0.6 * np.ones(m))
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def qp_margins(H, q, lo, hi, v):
    """(inputs on a bound, smallest multiplier of an active bound, smallest slack of an inactive one) in the Jacobi-scaled coordinates
    of mo.solve_box_qp_exact"""
    d = 1.0 / np.sqrt(np.diag(H))
    w, los, his = v / d, lo / d, hi / d
    g = (H * d[:, None] * d[None, :]) @ w + q * d
    at_lo, at_hi = v <= lo + 1e-13 * np.maximum(1.0, np.abs(lo)), v >= hi - 1e-13 * np.maximum(1.0, np.abs(hi))
    act = at_lo | at_hi
    mult = np.where(at_lo, g, np.where(at_hi, -g, np.inf))
    slack = np.where(act, np.inf, np.minimum(w - los, his - w))
    return int(act.sum()), float(mult.min()), float(slack.min())


@functools.lru_cache(maxsize=None)
def ltv_reference(c):
    """[dict(H, q, lo, hi, v, margins)] of every instance (mo.ltv_qp, mo.solve_box_qp_exact)"""
    a = ltv_inputs(c)
    out = []
    for i in range(c.batch):
        P = a["P"][i] if a["P"].ndim == 3 else a["P"]
        S = np.zeros((c.m, c.m)) if a["S"] is None else a["S"]
        H, q, lo, hi = mo.ltv_qp(a["A_all"][i], a["B_all"][i], None if a["c_all"] is None else a["c_all"][i], a["xbar"][i], a["ubar"][i],
                                 a["x_ref"], a["u_ref"], a["Q"], a["R"], S, P, a["umin"], a["umax"])
        v = mo.solve_box_qp_exact(H, q, lo, hi)
        out.append(dict(H=H, q=q, lo=lo, hi=hi, v=v, margins=qp_margins(H, q, lo, hi, v)))
    return out


# ---- the SQP loop, the exact mode, the re-linearisation: one problem per case
@functools.lru_cache(maxsize=None)
def nlp_problem(c):
    """dict(x_ref, u_ref, Q, R, S, P, u_min, u_max) and X0 (batch, n) of an sqp / exact / relin case"""
    n, m, N = c.shape
    rng = np.random.default_rng(31 * n + 7 * m + N + 1000 * c.H + 100000 * c.seed)
    x_ref = np.tile(0.1 * rng.standard_normal(n)[:, None], (1, N + 1))
    u_ref = np.tile(0.05 * rng.standard_normal(m)[:, None], (1, N))
    kw = dict(x_ref=x_ref, u_ref=u_ref, Q=10.0 * np.eye(n), R=1.0 * np.eye(m), S=(0.3 if c.family != "relin" else 0.0) * np.eye(m),
              P=25.0 * np.eye(n) + 0.2 * np.ones((n, n)), u_min=-c.ub * np.ones(m), u_max=c.ub * np.ones(m))
    X0 = x_ref[:, 0][None, :] + c.amp * rng.standard_normal((c.batch, n))
    return kw, X0


def _args(kw):
    return (kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"])


def traced(fn, *a, **k):
    """fn(*a, **k) with every QP it hands to mo.solve_box_qp_exact recorded: (result, [(H, q, lo, hi, v)])"""
    qps, solve = [], mo.solve_box_qp_exact

    def rec(H, f, lo, hi, *aa, **kk):
        v = solve(H, f, lo, hi, *aa, **kk)
        qps.append((H, f, lo, hi, v))
        return v
    mo.solve_box_qp_exact = rec
    try:
        return fn(*a, **k), qps
    finally:
        mo.solve_box_qp_exact = solve


@functools.lru_cache(maxsize=None)
def sqp_reference(c, adaptive=False):
    """per instance: dict(X [iters], U [iters]: the iterate after 1 .. SQP_ITERS iterations of mo.sqp_fnn, margins: qp_margins of every
    QP of the longest run)"""
    kw, X0 = nlp_problem(c)
    f = model(c)
    out = []
    for i in range(c.batch):
        Xs, Us = [], []
        for it in range(1, SQP_ITERS + 1):
            (X, U, hist), qps = traced(mo.sqp_fnn, f, X0[i], *_args(kw), it, adaptive=adaptive)
            Xs.append(X); Us.append(U)
        out.append(dict(X=Xs, U=Us, margins=[qp_margins(*q) for q in qps], hist=hist))
    return out


@functools.lru_cache(maxsize=None)
def solve_reference(c):
    """sqp_solve_ref.sqp_solve of every instance (merit rule), with the margins of its QPs"""
    kw, X0 = nlp_problem(c)
    out = []
    for i in range(c.batch):
        r, qps = traced(sref.sqp_solve, model(c), X0[i], *_args(kw), SOLVE_ITERS, SOLVE_TOL)
        out.append(dict(r, margins=[qp_margins(*q) for q in qps]))
    return out


def start_rollout(c, i):
    """(X, U) of sqp_fnn_start: the rollout of the clipped u_ref"""
    kw, X0 = nlp_problem(c)
    U = np.clip(kw["u_ref"], kw["u_min"][:, None], kw["u_max"][:, None])
    return mo.fnn_rollout(model(c), X0[i], U), U


def stage_hessian_of(kind):
    """the stage Hessian sqp_exact_ref.exact_qp must look up for a kind: its own for an Fnn (net_ref's falls back to it: patching it in
    would recurse), net_ref's for a ResNet / PolyNet, densenet_ref's for a DenseNet"""
    return {"fnn": ex.stage_hessian, "resnet": nr.stage_hessian, "polynet": nr.stage_hessian, "densenet": dr.stage_hessian}[kind]


_EX_STAGE_HESSIAN = ex.stage_hessian


@functools.lru_cache(maxsize=None)
def exact_reference(c):
    """[(H, q)] of the first QP of the exact mode of every instance (sqp_exact_ref.exact_qp)"""
    kw, X0 = nlp_problem(c)
    f = model(c)
    out = []
    ex.stage_hessian = _EX_STAGE_HESSIAN if c.kind == "fnn" else stage_hessian_of(c.kind)
    try:
        for i in range(c.batch):
            X, U = start_rollout(c, i)
            A, B, cc = [], [], []
            for k in range(c.N):
                Ak, Bk = f.jacobian(X[:, k], U[:, k])
                A.append(Ak); B.append(Bk); cc.append(f.forward(X[:, k], U[:, k]) - X[:, k + 1])
            He, qe, *_ = ex.exact_qp(f, X, U, A, B, cc, *_args(kw))
            out.append((He, qe))
    finally:
        ex.stage_hessian = _EX_STAGE_HESSIAN
    return out


@functools.lru_cache(maxsize=None)
def relin_reference(c):
    """dict(P, per instance: A, B at (x0, u_ref[:, 0]), the exact solution of the linearised problem)"""
    kw, X0 = nlp_problem(c)
    f = model(c)
    Al, Bl = f.jacobian(kw["x_ref"][:, -1], kw["u_ref"][:, -1])
    P = mo.dare(Al, Bl, kw["Q"], kw["R"])
    inst = []
    for i in range(c.batch):
        A, B = f.jacobian(X0[i], kw["u_ref"][:, 0])
        p = mo.make_problem(A, B, c.N, kw["u_min"], kw["u_max"], x_ref=kw["x_ref"], u_ref=kw["u_ref"], q=10.0, r=1.0, P=P)
        inst.append(dict(A=A, B=B, exact=mo.solve_mpc_exact(p, X0[i])))
    return dict(P=P, inst=inst)
