"""CPU tests of the case table behind tests/test_gpu_condensed_step_shapes.py (tests/condensed_step_cases.py): the Python restatement of
the step's selection rules uses the constants and the build lists of the source, the table reaches every build of k_admm, k_polish,
k_rollout, k_step_fused and k_step_inst_wave that csrc/instances/*.inc instantiate -- a build added later without a case fails
here --, it holds the rows the geometry of the kernels asks for, and every instance the GPU tests compare is one the finish can decide
(at most 32 active rows, the heavy cases at most 60 with the second-tier bands populated)."""
import os
import re

import numpy as np
import pytest

import condensed_step_cases as cc
import mpc_oracle as mo
from conftest import ROOT

CSRC = os.path.join(ROOT, "automationlabsmodelpredictivecontrol.jl_amd", "csrc")


def _read(*parts):
    with open(os.path.join(CSRC, *parts)) as f:
        return f.read()


def _const(src, name):
    """the value of `constexpr int NAME = <sum of integers>`"""
    m = re.search(r"\b%s\s*=\s*([0-9+ ]+)[;,]" % name, src)
    assert m, name
    return sum(int(t) for t in m.group(1).split("+"))


def _ints(pattern, src):
    return sorted(tuple(int(g) for g in m) if isinstance(m, tuple) else int(m) for m in re.findall(pattern, src))


# ---------------------------------------------------------------------------- the restatement against the source
def test_the_restatement_uses_the_constants_and_builds_of_the_source():
    api, ker = _read("almpc_api.hip"), _read("almpc_kernels.hip.h")
    step, inst = _read("instances", "step.inc"), _read("instances", "instance.inc")
    body = api[api.index("hipError_t launch_admm(int nrb"):]
    body = body[:body.index("#undef CASE")]
    launched = tuple((int(a), int(b)) for a, b in re.findall(r"\bCASE\(\s*(\d+)\s*,\s*(\d+)\s*\)", body))
    assert launched == cc.ADMM_BUILDS
    assert _ints(r"k_admm<(\d+), (\d+)>", step) == sorted(cc.ADMM_BUILDS)
    assert _ints(r"k_step_fused<(\d+), (\d+)>", step) == sorted(cc.FUSED_BUILDS)
    assert _ints(r"k_rollout<(\d+)>", step) == [1, 4]
    assert sorted(re.findall(r"k_polish<(\w+)>", step)) == ["false", "true"]
    assert _ints(r"k_step_inst_wave<(\d+)>", inst) == sorted(cc.WAVE_BUILDS)
    for name in ("ROLL_SMX", "ROLL_NX", "POLISH_SG_SHARED_CAP", "POLISH_LDS_MIN_PER_WAVE", "TILE"):
        assert _const(ker, name) == getattr(cc, name), name
    assert "#define ALMPC_EXP_POLISH_WAVES %d\n" % cc.POLISH_WAVES_GLDS in ker
    # pick_ks
    ks = api[api.index("int pick_ks(int nz, int nrb) {"):]
    ks = ks[:ks.index("\n}\n")]
    for line in ("const int exact = (nz + 3) / 4;", "if (nrb == 8 && exact <= 30) return 30;", "if (nrb == 3 && exact <= 10) return 10;",
                 "if (nrb == 1 && exact <= 3) return 3;", "return 4 * nrb;"):
        assert line in ks, line
    assert ks.count("return") == 4
    # the rules of the rollout, the layout and the routes as the source states them
    for text in ("int sblk = std::min(N, std::min(64 / n, ROLL_SMX / m));",
                 "if (!(sblk >= 1 && n <= ROLL_NX && !h->sw.rollout_stagewise)) return ALMPC_OK;",
                 "h->roll_s = sblk; h->roll_nb = (N + sblk - 1) / sblk;",
                 "while (2 * r.g * h->n <= 64) r.g *= 2;",
                 "r.fits = (size_t)(h->N + 1) * C <= 32 * 32 && r.cpl <= 8;",
                 "L.fuse_rollout = L.fused ? (h->ltv ? 2 : (blocked ? 3 : 1)) : 0;",
                 "L.g_lds = (size_t)h->nz * ((h->nz + 1) & ~1);",
                 "L.l_glds = (L.g_lds + L.SL.total + (size_t)POLISH_WAVES_GLDS * per_wave + 2) * sizeof(double);",
                 "if (L.l_glds + slot <= 160 * 1024 && !h->batched && !h->sw.polish_sg_global) {",
                 "return ((size_t)2 * h->nzs * TILE + (size_t)h->nrb * 8 * TILE + (size_t)4 * h->ksf * TILE) * sizeof(double);",
                 "h->nrb == 8 && (h->ks == 30 || h->ks == 32) && L.fused &&",
                 "L.l_step <= 160 * 1024)",
                 "if (!h->batched && h->nzs <= 64 && L.fused && h->dPlain && !h->ltv && !h->sw.no_shared_wave &&",
                 "h->sw.shared_wave_max_batch.value_or((long)2 * h->num_cus)",
                 "if (L.l_glds <= 160 * 1024 && !h->sw.polish_no_glds && !h->batched) {",
                 "if (!h->batched && (shared + 4 * per_wave) * sizeof(double) <= 60 * 1024) {",
                 "const size_t per_wave = (size_t)h->n * (h->N + 1) + h->nz, shared = (size_t)h->n * h->n + (size_t)h->n * h->m;"):
        assert text in api, text
    for text in ("const bool exact = p.roll_s * m <= %d && n <= %d;" % cc.ROLL_EXACT, "roll_run<%d, %d>(cu2, cx2," % cc.ROLL_EXACT,
                 "roll_run<ROLL_SMX, ROLL_NX>(cu, cx,",
                 "L.off_xref = L.off_ab + ((fused && fused != 3) ? n * (n + m) : 0);",
                 "L.total = (L.off_xref + (fused ? (N + 1) * n : 0) + 1) & ~1;"):
        assert text in ker, text


def test_the_restated_rules_at_known_shapes():
    assert [cc.pick_ks(nz, cc.nrb_of(nz)) for nz in (1, 12, 13, 16, 17, 40, 41, 112, 113, 120, 121, 128)] == [3, 3, 4, 4, 8, 10, 12, 28, 30, 30, 32, 32]
    assert cc.roll_block(12, 4, 30) == (5, 6) and cc.roll_exact(12, 4, 5) and cc.roll_block(16, 2, 8) == (4, 2) and not cc.roll_exact(16, 2, 4)
    assert cc.roll_block(1, 1, 32) == (24, 2) and cc.roll_block(3, 24, 2) == (1, 2) and cc.roll_block(2, 25, 5) == (0, 0) and cc.roll_block(17, 1, 17) == (0, 0)
    assert cc.roll_block(12, 4, 30, stagewise=True) == (0, 0)
    assert cc.roll_geom(12, 4, 30) == (4, 4, True) and cc.roll_geom(17, 1, 17)[2] is False and cc.roll_geom(2, 25, 5) == (32, 1, True)
    # the quadrotor: one kernel, the second-tier slot beside G in 160 KB; without the fused step two launches, without G in LDS k_polish<false>
    assert cc.pick_route(12, 4, 30) == "fused" and cc.polish_layout(12, 4, 30)["slot"] and cc.polish_layout(12, 4, 30)["l_step"] <= cc.LDS_MAX
    assert cc.pick_route(12, 4, 30, fuse_step=False) == "tile" and cc.pick_route(12, 4, 30, no_glds=True) == "tile_l2"
    assert cc.pick_route(12, 4, 30, polish=False) == "nopolish"
    # the one-wave step: nzs <= 64, up to two instances per CU
    assert cc.pick_route(3, 2, 7) == "wave" and cc.pick_route(3, 2, 7, batch=2 * cc.NUM_CUS + 1) == "tile" and cc.pick_route(3, 2, 7, no_shared_wave=True) == "tile"
    assert cc.pick_route(17, 1, 17) == "tile"       # (no rollout in the finish's tail: no one-wave step)
    # the one-kernel step ends at nz 123: beyond, G beside the ADMM buffers (2 x 128 x 16 + ... doubles) outgrows the 160 KB
    assert cc.pick_route(3, 1, 123) == "fused" and cc.pick_route(4, 4, 31) == "tile" and cc.pick_route(2, 1, 128) == "tile"
    assert cc.separate_rollout(20, 1, 40)[0] == 4 and cc.separate_rollout(64, 1, 17) == (1, 42632, False) and cc.separate_rollout(64, 1, 12)[0] == 4 and cc.separate_rollout(64, 1, 13)[0] == 1
    assert cc.separate_rollout(64, 2, 60) == (1, 65984, True)


# ---------------------------------------------------------------------------- the table against the builds
def test_the_table_reaches_every_instantiated_build_and_route():
    r = cc.reached()
    assert r["admm"] == set(cc.ADMM_BUILDS)
    assert r["fused"] == set(cc.FUSED_BUILDS)
    assert r["wave"] == set(cc.WAVE_BUILDS)
    assert r["polish"] == {True, False}
    assert r["rollout"] == {1, 4}
    assert {c.route for c in cc.CASES} | {c.tile_route for c in cc.CASES} == {"fused", "wave", "tile", "tile_l2"}
    kinds = {c.rollout[0] for c in cc.CASES}
    assert kinds == {"blocked_exact", "blocked_general", "stagewise_tail", "separate4", "separate1"}
    assert any(c.rollout[1] for c in cc.CASES)                       # k_rollout<1> beyond the 64 KiB of LDS a kernel has by default
    assert {c.slot for c in cc.CASES if c.nrb == 8} == {True, False}
    for c in cc.CASES:
        assert c.n <= 64 and c.nz <= 128 and c.batches[0] == cc.BATCH, c.id


def test_the_table_holds_the_required_rows():
    by_nz = {}
    for c in cc.REGULAR + cc.HEAVY:
        by_nz.setdefault(c.nz, []).append(c)
    largest, smallest = (12, 16, 32, 40, 48, 64, 80, 96, 112, 120, 128), (1, 13, 17, 33, 41, 49, 65, 81, 97, 113, 121)
    for b, hi, lo in zip(cc.ADMM_BUILDS, largest, smallest):
        assert any(c.build == b for c in by_nz.get(hi, ())) and any(c.build == b for c in by_nz.get(lo, ())), b
        assert cc.pick_ks(hi + 1, cc.nrb_of(hi + 1)) != b[1] or cc.nrb_of(hi + 1) != b[0] or hi == 128
        assert lo == 1 or (cc.nrb_of(lo - 1), cc.pick_ks(lo - 1, cc.nrb_of(lo - 1))) != b
    rows = [c for c in cc.REGULAR if c.nz in largest + smallest]
    assert {16, 17, 33, 64, 1} <= {c.n for c in rows}
    assert {4, 5, 9, 16} <= {c.ksf for c in rows}
    # k_step_inst_wave on shared operands: every NZC on the default route, at batches 37 and 1, and again on the tile route
    for nzs in cc.WAVE_BUILDS:
        cs = [c for c in cc.REGULAR if c.nzs == nzs and c.route == "wave" and c.tile_route == "tile"]
        assert any({37, 1} <= set(c.batches) for c in cs), nzs
    # rollout geometry
    geo = {c.id: (c.block, c.rollout[0]) for c in cc.CASES}
    assert geo["12-4-30"] == ((5, 6), "blocked_exact")                                                      # 60 lanes, N a multiple of s
    assert any(c.n == 16 and c.block[0] == 4 for c in cc.CASES)                                             # 64 lanes
    assert any(c.n == 13 and c.block[0] > 0 for c in cc.CASES)
    assert any(c.m == 24 and c.block[0] == 1 and c.rollout[0] == "blocked_general" for c in cc.CASES)
    assert any(c.m == 13 and c.block[0] == 1 and c.rollout[0] == "blocked_exact" and c.block[1] > 1 for c in cc.CASES)
    assert any(c.shape[:2] == (1, 1) and c.N >= 24 and c.block[0] == 24 for c in cc.CASES)
    assert any(c.block == (c.N, 1) and c.N < min(64 // c.n, 24 // c.m) and c.N > 1 for c in cc.CASES)      # one block
    assert any(c.block[0] > 1 and c.N % c.block[0] == 0 and c.block[1] > 1 for c in cc.CASES)
    assert any(c.block[0] > 1 and c.N % c.block[0] == 1 and c.block[1] > 1 for c in cc.CASES)
    assert any(c.block[0] * c.n == 64 and c.n < 16 for c in cc.CASES)
    assert any(c.xref_glb and c.block[0] > 0 for c in cc.CASES)
    # m > 24: the rows the kernels' geometry asks for, and two that the one-kernel step takes (nz <= 123)
    for shape, route in (((2, 25, 5), "tile"), ((3, 32, 4), "tile"), ((2, 25, 1), "wave"), ((3, 29, 4), "fused"), ((3, 41, 3), "fused")):
        c = cc.CASE_BY_ID["%d-%d-%d" % shape]
        assert c.rollout[0] == "stagewise_tail" and c.route == route, c.id
    assert {cc.CASE_BY_ID["3-29-4"].ks, cc.CASE_BY_ID["3-41-3"].ks} == {30, 32}
    # separate rollout
    sep = {c.id: c.rollout for c in cc.tagged("separate")}
    assert sep["64-1-17"] == ("separate1", False) and sep["64-2-60"] == ("separate1", True)
    assert any(17 <= c.n <= 32 and c.rollout == ("separate4", False) for c in cc.tagged("separate"))
    # heavy saturation
    assert {c.id: (c.route, c.nz, c.amp) for c in cc.HEAVY} == {"4-2-32-heavy": ("wave", 64, 10.0), "6-3-30-heavy": ("tile", 90, 10.0),
                                                                "7-5-25-heavy": ("tile", 125, 10.0)}
    assert cc.CASE_BY_ID["4-2-32-heavy"].tile_route == "tile" and cc.CASE_BY_ID["4-2-32-heavy"].slot and cc.CASE_BY_ID["6-3-30-heavy"].slot
    assert not cc.CASE_BY_ID["7-5-25-heavy"].slot       # nz 125: the slot does not fit beside G
    assert set(cc.HEAVY_BANDS) == {c.id for c in cc.HEAVY} == {c.id for c in cc.tagged("sg_global")}
    # the boundary of the affine first iterate
    assert [c.shape for c in cc.tagged("affine")] == [(55, 2, 1)] and [c.shape for c in cc.tagged("full_first")] == [(56, 2, 1)]
    # the route pairs
    unf = cc.tagged("unfused")
    assert all(c.route == "fused" and c.shape != cc.QUAD for c in unf) and {c.ks for c in unf} == {30, 32}
    assert sum(c.m > 24 for c in unf) == 2
    ng = cc.tagged("no_glds")
    assert {2, 4, 6, 8} <= {c.nrb for c in ng} and any(c.heavy for c in ng)
    sw = cc.tagged("stagewise")
    assert any(c.block[0] == 1 and c.block[1] > 1 for c in sw) and any(c.block == (c.N, 1) for c in sw)
    assert any(c.N % c.block[0] and c.block[1] > 1 for c in sw) and any(c.n == 16 for c in sw)
    assert {c.nrb for c in cc.tagged("freeze")} == {2, 5, 8}


# ---------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.id)
def test_compared_instances_are_within_the_finish_capacity(case):
    ref = cc.reference(case)
    p = ref["p"]
    assert sorted(ref["exact"]) == list(case.exact)
    na = np.array([cc.active_rows(p, ref["exact"][i]["u"]) for i in case.exact])
    for i in case.exact:   # the exact solutions are exact: solve_box_qp_exact's certificate, and solve_mpc_exact on the first one
        assert np.all(ref["exact"][i]["u"] <= p.u_max[:, None] + 1e-12) and np.all(ref["exact"][i]["u"] >= p.u_min[:, None] - 1e-12)
    assert np.abs(mo.solve_mpc_exact(p, ref["X0"][case.exact[0]])["u"] - ref["exact"][case.exact[0]]["u"]).max() <= 1e-12
    if case.heavy:
        lo_band, hi_band = cc.HEAVY_BANDS[case.id]
        assert na.max() <= 60
        assert ((na >= 33) & (na <= 48)).sum() >= 1
        assert (((na >= 49) & (na <= 60)).sum() >= 1) == hi_band and lo_band
    else:
        assert na.max() <= 32 and na.sum() >= 1
    assert ref["nact"].max() <= 60          # every instance, compared or not, is one the finish decides: status 0 can be asked of all
    if case.m > cc.ROLL_SMX:                # the stage-by-stage tail: the second row of a pair ends on its upper bound somewhere
        up = [np.isclose(ref["exact"][i]["u"], p.u_max[:, None], rtol=0, atol=1e-12).T.reshape(-1)[1::2].sum() for i in case.exact]
        assert sum(up) >= 1 and np.ptp(p.u_max) > 0 and np.all(p.u_max[1:] != p.u_max[:-1])
    if case.xref_glb:
        g = cc.reference_glb(case)
        xr, ur = g["refs"]
        ng = np.array([cc.active_rows(p, g["exact"][i]["u"]) for i in case.exact])
        assert ng.max() <= 32 and ng.sum() >= 1
        assert np.abs(g["exact"][case.exact[1]]["u"] - ref["exact"][case.exact[1]]["u"]).max() > 1e-6   # the references do move the solution


@pytest.mark.parametrize("case", cc.tagged("freeze"), ids=lambda c: c.id)
def test_freeze_inputs_stop_at_different_checks_and_far_from_the_threshold(case):
    """Equal iteration counts can be asked of the device without an allowance: no residual of any check lies within 1e-6 (relative)
    of its threshold, and every tile holds instances that stop at different checks."""
    p = cc.problem(case)
    des = mo.design_shared(p)
    X0 = cc.freeze_x0(case)
    iters = []
    for i in range(cc.BATCH):
        trace = []
        r = cc.admm(des, cc.fs_of(p, des, X0[i]), trace=trace, **cc.FREEZE_OPTS)
        iters.append(r["iters"])
        assert r["status"] == 0 and len(trace) == r["iters"] // cc.FREEZE_OPTS["check_every"]
        for rp, tp, rd, td in trace:
            assert abs(rp - tp) > 1e-6 * tp and abs(rd - td) > 1e-6 * td, i
    for t0 in range(0, cc.BATCH, cc.TILE):
        assert len(set(iters[t0:t0 + cc.TILE])) >= 2, t0


def test_the_chained_iteration_is_the_oracles():
    """cc.admm from zero is mpc_oracle.admm_box; from a kept state it continues it: 3 + 4 iterations without a check are 7"""
    c = cc.CASE_BY_ID["5-7-7"]
    p = cc.problem(c)
    des = mo.design_shared(p, rho=30.0, rho_profile="stiffness")
    fs = cc.fs_of(p, des, cc.x0(c)[3])
    kw = dict(alpha=1.6, eps_abs=0.0, eps_rel=0.0)
    a = mo.admm_box(des["Hs"], fs, des["lo"], des["hi"], rho=des["rho_vec"], sigma=des["sigma"], max_iter=7, check_every=7, Minv=des["Minv"],
                    unscale=des["d"], **kw)
    b = cc.admm(des, fs, max_iter=7, check_every=7, **kw)
    c3 = cc.admm(des, fs, max_iter=3, check_every=3, **kw)
    c7 = cc.admm(des, fs, c3["x"], c3["z"], c3["y"], max_iter=4, check_every=4, **kw)
    for k in ("x", "z", "y"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c7[k]), k
    assert np.abs(b["z"]).max() > 0 and (b["z"] == des["lo"]).any() | (b["z"] == des["hi"]).any()
