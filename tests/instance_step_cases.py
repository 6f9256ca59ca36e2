"""The shapes at which the per-instance design and step (almpc_design_batched -> almpc_calculate on a condensed handle) are tested:
one table for tests/test_instance_step_cases.py (CPU: the table reaches every instantiated build and route, and its inputs are well
posed) and tests/test_gpu_instance_step_shapes.py (GPU: design and step against the oracles, on the builds the table names).

The selection rules of csrc/almpc_api.hip (launch_batched_design, launch_batched_factor, polish_layout, pick_route, step_two_launch,
step_admm_or_guess, step_rollout), csrc/almpc_design.hip.h (design_inverse_*, launch_design_inverse, launch_neg_gm_batched) and
csrc/almpc_instance.hip.h (design_instance_lds_doubles) are restated here in Python; the CPU test holds them against the source.
A set of switches is a dict {ALMPC_*: value} as a handle's environment holds it."""
import copy
import functools

import numpy as np

import condensed_step_cases as cc
import mpc_oracle as mo

# ---------------------------------------------------------------------------- constants of the source (checked by the CPU test)
DESIGN_BUILDS = ((12, 4), (4, 2), (2, 1), (0, 0))                     # k_design_instance_t<NC, MC>, in the launcher's order
INV_WAVE_BUILDS = (16, 32, 48, 64)                                    # k_design_inverse_wave<NC>
INV_C32_BUILDS = tuple((cw, h) for h in (True, False) for cw in (8, 16, 32))   # k_design_inverse_c32<CW, H>
INV_TILE_BUILDS = ((2, 8, 8), (4, 16, 8))                             # k_design_inverse_t<AR, KC, NG = 8>
NEG_GM_BUILDS = (4, 8, 16)                                            # k_neg_gm_cols<NC>
ADMM_INST_BUILDS = (True, False)                                      # k_admm_inst<PACKED>
WAVE_BUILDS = cc.WAVE_BUILDS                                          # k_step_inst_wave<NZC>
LDS_MAX = cc.LDS_MAX
NUM_CUS = cc.NUM_CUS
POLISH_GLB_PER_INST = 64 * 64
POLISH_WAVES = 4
INV_WAVES_PER_WG = 4                # k_design_inverse_wave: 256 threads, one wave per matrix (two per instance in its two-inverse mode)
C32_THROUGHPUT_ABOVE = 256          # the column-split inverse: <CW, true> up to 256 matrices, <CW, false> beyond
BATCH = cc.BATCH
BIG = 2 * NUM_CUS + 3               # 515: one more round of the persistent grid for three instances, k_polish<false> with strides
EXACT_STEP = cc.EXACT_STEP
QUAD = cc.QUAD
PROFILES = (("scalar", 0.1), ("stiffness", 30.0))


def on(env, name):
    """ON_IF_SET switches (csrc/almpc_switches.h)"""
    return name in env


def on1(env, name):
    """ON_IF_1 switches"""
    return dict(env).get(name, "")[:1] == "1"


# ---------------------------------------------------------------------------- the design
def design_instance_lds_doubles(n, m, N):
    return 4 * n * n + n * m + (N + 1) * n * n + 5 * N * n * m


def design_route(n, m, N):
    """lds (k_design_instance_t) | dense (k_design_blocks + k_design_gamma + k_design_hessian, blockIdx.y = instance)"""
    return "lds" if design_instance_lds_doubles(n, m, N) * 8 <= LDS_MAX else "dense"


def design_build(n, m):
    return (n, m) if (n, m) in DESIGN_BUILDS[:3] else (0, 0)


def scale_in_tail(n, m, N, env=()):
    """the Jacobi scaling as the tail of k_design_instance_t; else k_design_scale"""
    return design_route(n, m, N) == "lds" and m * N <= 128 and design_instance_lds_doubles(n, m, N) >= 128 and not on(env, "ALMPC_DBG_SPLIT_SCALE")


def inverse_makes_rho(nz, nzs, env):
    return nz <= 64 and nzs <= 64 and not on(env, "ALMPC_INV_TILE") and not on(env, "ALMPC_NO_RHO_FUSION")


def inverse_can_pack(nz, env):
    return nz > 64 and nz <= 128 and (nz & 1) == 0 and not on(env, "ALMPC_INV_TILE") and not on(env, "ALMPC_NO_PACKED_MINV")


def inverse_makes_v(nz, env):
    return nz <= 128 and not on(env, "ALMPC_INV_TILE") and not on(env, "ALMPC_DBG_SPLIT_NEGGM")


def inverse_build(nz, matrices, env):
    """launch_design_inverse: ("wave", NC) | ("c32", CW, H) | ("tile", AR, KC, NG)"""
    tile = on(env, "ALMPC_INV_TILE")
    if nz <= 64 and not tile:
        return ("wave", next(z for z in INV_WAVE_BUILDS if nz <= z))
    if nz <= 64:
        return ("tile",) + INV_TILE_BUILDS[0]
    if not tile:
        cw = int(env["ALMPC_INV_CW"]) if "ALMPC_INV_CW" in env else (16 if matrices <= C32_THROUGHPUT_ABOVE else 32)
        return ("c32", cw if cw in (8, 16) else 32, matrices <= C32_THROUGHPUT_ABOVE)
    return ("tile",) + INV_TILE_BUILDS[1]


def neg_gm_build(n, nz):
    """launch_neg_gm_batched: k_neg_gm_cols<4 | 8 | 16>, 0 for the generic k_neg_gm"""
    lds = n * nz * 8
    for nc in NEG_GM_BUILDS:
        if nz <= 128 and n <= nc and lds <= 48 * 1024:
            return nc
    return 0


def wave_inverse_grid(batch, two):
    """(workgroups, waves of the last one that have a job) of k_design_inverse_wave"""
    jobs = 2 * batch if two else batch
    return (jobs + INV_WAVES_PER_WG - 1) // INV_WAVES_PER_WG, (jobs - 1) % INV_WAVES_PER_WG + 1


def factor_plan(n, m, N, batch=BATCH, profile="scalar", env=()):
    """launch_batched_factor behind a per-instance design (with_v, an ADMM phase follows): dict(scale: k_design_scale runs,
    one_launch, inverses: the builds launched, v_in_inverse, neg_gm: build or None, rho_kernel: k_design_rho runs, packed)"""
    env = dict(env)
    nz = m * N
    nzs = 16 * cc.nrb_of(nz)
    inv = inverse_build(nz, batch, env)
    out = dict(scale=not scale_in_tail(n, m, N, env), one_launch=False, inverses=[inv], v_in_inverse=False, neg_gm=None, rho_kernel=False,
               packed=False)
    if (profile == "scalar" and inverse_makes_rho(nz, nzs, env) and nz <= 64 and inverse_makes_v(nz, env)
            and not on(env, "ALMPC_DBG_SPLIT_INVERSES")):
        out.update(one_launch=True, v_in_inverse=True)
        return out
    if nz <= 64 and inverse_makes_v(nz, env):
        out["v_in_inverse"] = True
    else:
        out["neg_gm"] = neg_gm_build(n, nz)
    out["packed"] = inverse_can_pack(nz, env)
    out["rho_kernel"] = not inverse_makes_rho(nz, nzs, env)
    out["inverses"].append(inv)
    return out


# ---------------------------------------------------------------------------- the step
def polish_layout(n, m, N):
    """polish_layout of per-instance models: dict(fused, per_wave, wave_const_off, total) (doubles) -- no blocked rollout (that is
    the shared model's), no second-tier slot in the workgroup's LDS"""
    nz = m * N
    nzs = 16 * cc.nrb_of(nz)
    fused = cc.roll_geom(n, m, N)[2]
    per_wave = cc.POLISH_LDS_MIN_PER_WAVE
    if fused and (N + 1) * (n + m) > per_wave:
        per_wave = (N + 1) * (n + m)
    per_wave = (per_wave + 1) & ~1
    off = per_wave
    per_wave += (nzs + n * (n + m) + 1) & ~1
    return dict(fused=fused, per_wave=per_wave, wave_const_off=off, total=cc.polish_shared_total(n, m, N, nz, nzs, 1 if fused else 0), slot=False)


def wave_step_lds_bytes(n, m, N):
    L = polish_layout(n, m, N)
    nz = m * N
    return (L["total"] + L["per_wave"] + nz * 16 * cc.nrb_of(nz)) * 8


def pick_route(n, m, N, polish=True, env=()):
    """wave (k_step_inst_wave) | two (k_admm_inst + a finish) | nopolish (k_admm_inst + k_rollout<1>)"""
    if not polish:
        return "nopolish"
    nzs = 16 * cc.nrb_of(m * N)
    if nzs <= 64 and polish_layout(n, m, N)["fused"] and not on1(env, "ALMPC_NO_INST_WAVE") and wave_step_lds_bytes(n, m, N) <= 64 * 1024:
        return "wave"
    return "two"


def sgl_lds_bytes(n, m, N):
    L = polish_layout(n, m, N)
    nz = m * N
    return (L["total"] + L["per_wave"] + POLISH_GLB_PER_INST + nz * 16 * cc.nrb_of(nz)) * 8


def finish(n, m, N, batch=BATCH, env=()):
    """the finish of step_two_launch: sgl (k_polish_sgl<0>: G_i and the second-tier inverse in LDS) | l2 (k_polish<false> with strides)
    | unsupported (no rollout in the finish's tail)"""
    if not polish_layout(n, m, N)["fused"]:
        return "unsupported"
    if batch <= 2 * NUM_CUS and sgl_lds_bytes(n, m, N) <= LDS_MAX and not on(env, "ALMPC_POLISH_SG_GLOBAL"):
        return "sgl"
    return "l2"


def admm_inst_grid(batch):
    """workgroups of the persistent grid of k_admm_inst: workgroup b solves instances b, b + grid, ..."""
    return batch if NUM_CUS * 2 > batch else NUM_CUS * 2


def step_kernels(n, m, N, batch=BATCH, profile="scalar", polish=True, env=()):
    """the kernels of one step as a tuple of names"""
    r = pick_route(n, m, N, polish, env)
    nzs = 16 * cc.nrb_of(m * N)
    if r == "wave":
        return (("step_inst_wave", next(z for z in WAVE_BUILDS if nzs <= z)),)
    admm = ("admm_inst", factor_plan(n, m, N, batch, profile, env)["packed"])
    if r == "nopolish":
        return (admm, ("rollout", 1))
    return (admm, ("polish", finish(n, m, N, batch, env)))


# ---------------------------------------------------------------------------- the cases
NO_WAVE = {"ALMPC_NO_INST_WAVE": "1"}
SG_GLOBAL = {"ALMPC_POLISH_SG_GLOBAL": "1"}
SPLIT = {"ALMPC_DBG_SPLIT_SCALE": "1", "ALMPC_DBG_SPLIT_NEGGM": "1", "ALMPC_DBG_SPLIT_INVERSES": "1"}


def _env_id(env):
    return "+".join(k[len("ALMPC_"):].lower() + ("" if v == "1" else v) for k, v in sorted(env.items())) or "default"


class Case:
    """One row: a shape, a batch, and the sets of switches (`envs`) it is run under beside none.  Every set that changes the design
    (the inverse builds, the penalty profile's kernel, the packed layout, the split launches) is compared with the default handle
    bit for bit in d, H, F and in status and iteration counts (test f); NO_WAVE and SG_GLOBAL are routes of the step (tests b - e)."""

    def __init__(self, n, m, N, amp=3.0, batch=BATCH, heavy=False, envs=(), batches=(), tags=(), seed=0):
        self.n, self.m, self.N, self.amp, self.batch, self.heavy, self.seed = n, m, N, amp, batch, heavy, seed
        self.envs = tuple(dict(e) for e in envs)
        self.batches = tuple(batches)       # smaller batches: bit for bit the first rows of the full run
        self.tags = frozenset(tags)
        if batch > BATCH:
            self.exact = tuple(range(0, batch, 20)) + tuple(range(2 * NUM_CUS, batch))
        else:
            self.exact = tuple(range(batch)) if heavy else tuple(range(0, batch, EXACT_STEP))

    nz = property(lambda s: s.m * s.N)
    nzs = property(lambda s: 16 * cc.nrb_of(s.nz))
    shape = property(lambda s: (s.n, s.m, s.N))
    id = property(lambda s: "%d-%d-%d%s%s" % (s.n, s.m, s.N, "-heavy" if s.heavy else "", "" if s.batch == BATCH else "-b%d" % s.batch))
    route = property(lambda s: pick_route(*s.shape))

    def __repr__(self):
        return self.id

    def step_envs(self):
        """the sets of switches that choose the step's kernels: none; NO_WAVE where the default is the one-wave step; SG_GLOBAL where
        the table asks for it (on top of NO_WAVE where needed to reach a finish of its own)"""
        out = [{}]
        if self.route == "wave":
            out.append(NO_WAVE)
        for e in self.envs:
            if on(e, "ALMPC_POLISH_SG_GLOBAL"):
                out.append(e)
        return out

    def design_envs(self):
        """the sets of switches that change the design's launches"""
        return [e for e in self.envs if not on(e, "ALMPC_POLISH_SG_GLOBAL") and e != NO_WAVE]

    def all_envs(self):
        out = []
        for e in self.step_envs() + self.design_envs():
            if e not in out:
                out.append(e)
        return out


def _cw(v):
    return {"ALMPC_INV_CW": str(v)}


_TILE, _NORHO, _NOPACK = {"ALMPC_INV_TILE": "1"}, {"ALMPC_NO_RHO_FUSION": "1"}, {"ALMPC_NO_PACKED_MINV": "1"}
_SGW = dict(NO_WAVE, **SG_GLOBAL)
CASES = (
    # ---- every wave build (k_design_inverse_wave, k_step_inst_wave) at exact fit and one past it: nz 1, 12, 16, 17, 32, 33, 48, 49, 59, 64
    Case(1, 1, 1),                                          # 12 doubles of design LDS: the scaling by k_design_scale
    Case(3, 2, 6, envs=(_NORHO, SPLIT), batches=(1, 3, 4, 5)),
    Case(16, 1, 16, envs=(SPLIT,)),                         # n = 16: k_neg_gm_cols<16> under the split launches
    Case(2, 1, 17, tags=("freeze",)),                       # k_design_instance_t<2, 1>, m N < 64
    Case(4, 2, 16, envs=(_TILE,)),                          # <4, 2>, m N < 64; k_design_inverse_t<2, 8, 8>
    Case(13, 3, 11),
    Case(12, 4, 12, envs=(_NORHO,)),                        # <12, 4>, m N < 64
    Case(3, 24, 2),
    Case(5, 7, 7, amp=2.0, envs=(SPLIT, _SGW)),             # n = 5: k_neg_gm_cols<8> under the split launches
    Case(16, 1, 59),                                        # 21 120 doubles: the dense design route in front of the one-wave step
    Case(16, 4, 16, envs=(_SGW,)),
    Case(4, 2, 32, amp=20.0, heavy=True, envs=(_SGW,)),     # one-wave step, k_polish_sgl<0> and k_polish<false> on 33 .. 60 active rows
    # ---- nz above 64: the column-split inverse, k_neg_gm_cols, k_admm_inst packed and full, both finishes
    Case(5, 13, 5),                                         # nz 65, odd: full Minv
    Case(2, 2, 33, envs=(_NOPACK, _cw(8), _cw(32))),        # nz 66, even: packed; n = 2: k_neg_gm_cols<4>
    Case(3, 23, 3, envs=(_cw(16),)),                        # nz 69
    Case(4, 2, 40, envs=(SG_GLOBAL,), tags=("freeze",)),    # <4, 2>, m N > 64
    Case(6, 3, 30, amp=13.5, heavy=True, envs=(SG_GLOBAL,)),  # nz 90: Sinv in LDS (k_polish_sgl<0>) and in the global scratch
    Case(2, 1, 97),                                         # <2, 1>, m N > 64; odd
    Case(16, 2, 50, envs=(_TILE,)),                         # nz 100, 22 112 doubles: the dense route; n = 16: k_neg_gm_cols<16>; <4, 16, 8>
    Case(6, 4, 30),                                         # nz 120, n = 6: k_neg_gm_cols<8>
    Case(12, 4, 30),                                        # the quadrotor family: <12, 4>, m N > 64; k_polish<false> by default
    Case(3, 1, 127, amp=1.0),                               # (amplitude 3 would put up to 55 rows on a bound)
    Case(16, 8, 16),                                        # nz 128
    # ---- large batches at small shapes
    Case(2, 2, 5, batch=BIG, envs=(_NORHO,), tags=("freeze",)),         # nz 10: the wave inverse's partial last workgroup in both modes
    Case(4, 2, 36, batch=BIG, envs=(_cw(16), _cw(8)), tags=("freeze",)),  # nz 72: c32<32 | 16 | 8, false>, packed k_admm_inst persistent
)
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)
REGULAR = tuple(c for c in CASES if not c.heavy)
HEAVY = tuple(c for c in CASES if c.heavy)
HEAVY_BANDS = {"4-2-32-heavy": (True, True), "6-3-30-heavy": (True, True)}   # 33..48, 49..60 populated
FREEZE_AMPS = cc.FREEZE_AMPS
FREEZE_OPTS = cc.FREEZE_OPTS


def tagged(tag):
    return tuple(c for c in CASES if tag in c.tags)


def reached():
    """What the table claims to run, derived from the rules above"""
    out = dict(design=set(), design_route=set(), scale_in_tail=set(), inv_wave=set(), inv_c32=set(), inv_tile=set(), neg_gm=set(),
               rho_kernel=set(), one_launch=set(), packed=set(), admm_inst=set(), step_wave=set(), finish=set(), rollout=set(),
               wave_inverse_partial=set(), admm_inst_rounds=set())
    for c in CASES:
        out["design_route"].add(design_route(*c.shape))
        if design_route(*c.shape) == "lds":
            out["design"].add(design_build(c.n, c.m))
        for env in c.all_envs():
            out["scale_in_tail"].add(scale_in_tail(*c.shape, env))
            for profile, _ in PROFILES:
                f = factor_plan(*c.shape, c.batch, profile, env)
                for b in f["inverses"]:
                    out["inv_" + b[0]].add(b[1:] if len(b) > 2 else b[1])
                    if b[0] == "wave":
                        out["wave_inverse_partial"].add((f["one_launch"], wave_inverse_grid(c.batch, f["one_launch"])[1] < INV_WAVES_PER_WG))
                if f["neg_gm"] is not None:
                    out["neg_gm"].add(f["neg_gm"])
                out["rho_kernel"].add((f["rho_kernel"], c.nz <= 64))
                out["one_launch"].add(f["one_launch"])
                out["packed"].add(f["packed"])
                for polish in (True, False):
                    for k in step_kernels(*c.shape, c.batch, profile, polish, env):
                        if k[0] == "admm_inst":
                            out["admm_inst"].add(k[1])
                            out["admm_inst_rounds"].add(c.batch > admm_inst_grid(c.batch))
                        elif k[0] == "step_inst_wave":
                            out["step_wave"].add(k[1])
                        elif k[0] == "polish":
                            out["finish"].add(k[1])
                        else:
                            out["rollout"].add(k[1])
    return out


# ---------------------------------------------------------------------------- inputs and references
def _base(c):
    """the shared part of a case's problems: weights q = 10, r = 1, s = 0.5 (N > 2), P = 20 I given, bounds -0.5 / 0.7, a non-zero
    x_ref and a time-varying u_ref (cc.problem's)"""
    n, m, N = c.shape
    rng = np.random.default_rng(9000 * n + 10 * m + N + 100000 * c.seed)
    A0, B0 = rng.standard_normal((n, n)), rng.standard_normal((n, m))
    u_ref = 0.05 * rng.standard_normal((m, 1)) + 0.03 * rng.standard_normal((m, N))
    return rng, A0, B0, 0.1 * rng.standard_normal(n), u_ref


@functools.lru_cache(maxsize=None)
def models(c):
    """(A (batch, n, n), B (batch, n, m)), read-only: the quadrotor family for (12, 4, 30); else A_i = A0 + 0.1 N(0, 1) rescaled to a
    spectral radius drawn from [0.85, 0.99], B_i = B0 (1 + 0.1 N(0, 1)) elementwise"""
    n, m, N = c.shape
    if c.shape == QUAD:
        from test_gpu_batched_models import quad_family
        A, B = quad_family(mo, c.batch)
    else:
        rng, A0, B0, _, _ = _base(c)
        A = A0[None] + 0.1 * rng.standard_normal((c.batch, n, n))
        for i in range(c.batch):
            A[i] *= rng.uniform(0.85, 0.99) / np.max(np.abs(np.linalg.eigvals(A[i])))
        B = B0[None] * (1.0 + 0.1 * rng.standard_normal((c.batch, n, m)))
    A.setflags(write=False); B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def template(c):
    """the problem of a case with the base model: weights, P, bounds and references of every instance"""
    n, m, N = c.shape
    if c.shape == QUAD:
        return mo.quadrotor()           # (P: the nominal model's DARE solution, GIVEN to the design of every instance)
    _, A0, B0, x_ref, u_ref = _base(c)
    return mo.make_problem(A0, B0, N, -0.5 * np.ones(m), 0.7 * np.ones(m), x_ref=x_ref, u_ref=u_ref, q=10.0, r=1.0, s=0.5 if N > 2 else 0.0,
                           P=20.0 * np.eye(n))


def problem(c, i):
    """the problem of instance i"""
    p = copy.copy(template(c))
    p.A, p.B = models(c)[0][i], models(c)[1][i]
    return p


def x0(c, amp=None):
    amp = c.amp if amp is None else amp
    if c.shape == QUAD:
        return mo.quadrotor_x0_batch(c.batch, amp, first_instance=77)
    return amp * np.random.default_rng(c.n + c.N + 100000 * c.seed + 17).standard_normal((c.batch, c.n))


def freeze_x0(c):
    X0 = x0(c, 1.0)
    return X0 * np.where(np.arange(c.batch) % 2 == 0, FREEZE_AMPS[0], FREEZE_AMPS[1])[:, None]


@functools.lru_cache(maxsize=None)
def condensed(c):
    """[(H_i, F_i, fS_i)] of every instance (mo.condense, mo.s_rate_gradient)"""
    out = []
    for i in range(c.batch):
        p = problem(c, i)
        _, _, H, F = mo.condense(p)
        out.append((H, F, mo.s_rate_gradient(p)))
    return out


@functools.lru_cache(maxsize=None)
def designs(c, profile, rho):
    """[mo.design_shared of instance i's problem]"""
    return [mo.design_shared(problem(c, i), rho=rho, rho_profile=profile) for i in range(c.batch)]


def _exact(c, which):
    X0 = x0(c)
    t = template(c)
    lo = (t.u_min[:, None] - t.u_ref).T.reshape(-1)
    hi = (t.u_max[:, None] - t.u_ref).T.reshape(-1)
    out = {}
    for i in which:
        p = problem(c, i)
        _, _, H, F = mo.condense(p)
        out[i] = mo.rollout(p, X0[i], mo.solve_box_qp_exact(H, F @ (X0[i] - p.x_ref[:, 0]) + mo.s_rate_gradient(p), lo, hi))
    return out


@functools.lru_cache(maxsize=None)
def reference(c):
    """dict(X0, exact {i: rollout dict of the exact solution of instance i's own problem} for the compared instances), computed
    once per process and read-only"""
    return dict(X0=x0(c), exact=_exact(c, c.exact))


@functools.lru_cache(maxsize=None)
def active_counts(c):
    """active rows of the exact solution of EVERY instance"""
    e = dict(reference(c)["exact"])
    e.update(_exact(c, [i for i in range(c.batch) if i not in e]))
    return np.array([cc.active_rows(problem(c, i), e[i]["u"]) for i in range(c.batch)])
