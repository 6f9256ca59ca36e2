"""CPU tests of the case table behind tests/test_gpu_instance_step_shapes.py (tests/instance_step_cases.py): the Python restatement of
the selection rules of the per-instance design and step uses the text, the constants and the build lists of the source; the table
reaches every build of k_design_instance_t, k_design_inverse_wave, k_design_inverse_c32, k_design_inverse_t, k_neg_gm_cols,
k_admm_inst and k_step_inst_wave that csrc/instances/*.inc instantiate -- a build added later without a case fails here --, both
design routes, both homes of the scaling, both finishes behind a per-instance model and k_rollout<1> with strides; and the inputs
are ones on which the GPU tests cannot hide a failure: well conditioned, every instance within the finish's capacity, active rows
present, models distinct, no residual of the freeze runs near its threshold."""
import os
import re

import numpy as np
import pytest

import condensed_step_cases as cc
import instance_step_cases as ic
import mpc_oracle as mo
from conftest import ROOT

CSRC = os.path.join(ROOT, "automationlabsmodelpredictivecontrol.jl_amd", "csrc")
QUAD_ID = "12-4-30"
# The register Gauss-Jordan inverse carries a few eps cond: these caps keep its error three orders below the iterate tolerance of
# 1e-9.  The quadrotor family (BASELINE configs[3], weights 100 / 0.1 on double integrators) is what it is: 6.5e6 and 1.2e5, its
# iterates are held to the same 1e-9 (as in test_admm_iterate_matches_oracle_per_instance), one order above the inverse's error.
COND_H, COND_M = 1e5, 1e3
COND_H_QUAD, COND_M_QUAD = 1e7, 2e5


def _read(*parts):
    with open(os.path.join(CSRC, *parts)) as f:
        return f.read()


def _builds(kernel, src):
    """the template arguments of every instantiation line of `kernel`, as tuples of int / bool"""
    conv = lambda t: {"true": True, "false": False}.get(t.strip(), None) if t.strip() in ("true", "false") else int(t)
    return sorted(tuple(conv(t) for t in m.split(",")) for m in re.findall(r"almpc::%s<([^>]*)>\(" % kernel, src))


def _function(src, head):
    body = src[src.index(head):]
    return body[:body.index("\n}\n")]


# ---------------------------------------------------------------------------- the restatement against the source
def test_the_restatement_uses_the_constants_and_builds_of_the_source():
    api, des, inst, ker = _read("almpc_api.hip"), _read("almpc_design.hip.h"), _read("almpc_instance.hip.h"), _read("almpc_kernels.hip.h")
    da, db = _read("instances", "design_a.inc"), _read("instances", "design_b.inc")
    ii, st = _read("instances", "instance.inc"), _read("instances", "step.inc")
    # the build lists
    assert _builds("k_design_instance_t", da) == sorted(ic.DESIGN_BUILDS)
    assert _builds("k_design_inverse_wave", db) == [(z,) for z in ic.INV_WAVE_BUILDS]
    assert _builds("k_design_inverse_c32", db) == sorted(ic.INV_C32_BUILDS)
    assert _builds("k_design_inverse_t", db) == sorted(ic.INV_TILE_BUILDS)
    assert _builds("k_neg_gm_cols", db) == [(z,) for z in ic.NEG_GM_BUILDS]
    assert _builds("k_admm_inst", ii) == sorted((b,) for b in ic.ADMM_INST_BUILDS)
    assert _builds("k_step_inst_wave", ii) == [(z,) for z in ic.WAVE_BUILDS]
    assert _builds("k_polish_sgl", st) == [(0,), (1,)] and _builds("k_polish", st) == [(False,), (True,)] and _builds("k_rollout", st) == [(1,), (4,)]
    for f, lines in ((da, 9), (db, 27), (ii, 6), (st, 19)):     # a line added to one of the four lists: say here which table covers it
        assert f.count("ALMPC_KERNEL_INSTANCE(") == len(re.findall(r"almpc::k_\w+<", f)) == lines
    for name in ("k_design_instance_t", "k_design_inverse_", "k_neg_gm_cols", "k_admm_inst", "k_step_inst_wave"):
        for other in os.listdir(os.path.join(CSRC, "instances")):
            if other not in ("design_a.inc", "design_b.inc", "instance.inc"):
                assert name not in _read("instances", other), (name, other)
    # constants
    assert "constexpr int POLISH_GLB_PER_INST = 64 * 64;" in ker and ic.POLISH_GLB_PER_INST == 64 * 64
    assert "constexpr int POLISH_WAVES = %d;" % ic.POLISH_WAVES in ker
    assert "constexpr int ADMM_INST_THREADS = 256;" in inst
    # the switches and their parsing rules
    sw = _read("almpc_switches.h")
    for name, member, rule in (("ALMPC_NO_INST_WAVE", "no_inst_wave", "ON_IF_1"), ("ALMPC_POLISH_SG_GLOBAL", "polish_sg_global", "ON_IF_SET"),
                               ("ALMPC_INV_TILE", "inv_tile", "ON_IF_SET"), ("ALMPC_INV_CW", "inv_columns_per_wave", "INTEGER"),
                               ("ALMPC_NO_RHO_FUSION", "no_rho_fusion", "ON_IF_SET"), ("ALMPC_NO_PACKED_MINV", "no_packed_minv", "ON_IF_SET"),
                               ("ALMPC_DBG_SPLIT_NEGGM", "dbg_split_neggm", "ON_IF_SET"), ("ALMPC_DBG_SPLIT_INVERSES", "dbg_split_inverses", "ON_IF_SET"),
                               ("ALMPC_DBG_SPLIT_SCALE", "dbg_split_scale", "ON_IF_SET")):
        assert "X(%s, %s, %s," % (name, member, rule) in sw, name
    # the design route, the <NC, MC> dispatch and the home of the scaling
    assert "return (size_t)4 * n * n + (size_t)n * m + (size_t)(N + 1) * n * n + (size_t)5 * N * n * m;" in _function(inst, "inline size_t design_instance_lds_doubles(int n, int m, int N) {")
    lbd = _function(api, "hipError_t launch_batched_design(almpc_handle* h")
    for text in ("size_t inst_lds = design_instance_lds_doubles(n, m, N) * sizeof(double);",
                 "if (inst_lds <= 160 * 1024) {",
                 "if (nz <= 128 && design_instance_lds_doubles(n, m, N) >= 128 && !h->sw.dbg_split_scale) {",
                 "scaled = dp.Hs != nullptr;",
                 "if (n == 12 && m == 4) DESIGN_INST(12, 4);", "else if (n == 4 && m == 2) DESIGN_INST(4, 2);",
                 "else if (n == 2 && m == 1) DESIGN_INST(2, 1);", "else DESIGN_INST(0, 0);",
                 "hipLaunchKernelGGL((k_design_instance_t<NC_, MC_>), dim3(gb), dim3(256), inst_lds, st, dp);",
                 "hipLaunchKernelGGL(k_design_blocks, dim3(1, gb),", "hipLaunchKernelGGL(k_design_gamma, dim3(N, gb),",
                 "hipLaunchKernelGGL(k_design_hessian, dim3(nrb, gb),",
                 "launch_batched_factor(h, ds2, rho, sigma, st, no_admm, scaled, true);"):
        assert text in lbd, text
    assert lbd.count("DESIGN_INST(") == 5      # the macro and its four uses: no fifth build
    assert "if (design_instance_lds_doubles(n, m, N) * sizeof(double) > 160 * 1024) {  // dense route only" in api
    # the factorisation
    lbf = _function(api, "void launch_batched_factor(almpc_handle* h")
    for text in ("if (!scaled) hipLaunchKernelGGL(k_design_scale, dim3(1, gb),",
                 "if (!v1M && !no_admm && h->rho_mode == 0 && design_inverse_makes_rho(h->sw, nz, nzs) && nz <= 64 && design_inverse_makes_v(h->sw, nz) && !h->sw.dbg_split_inverses) {",
                 "h->minv_packed = false;",
                 "else if (with_v && nz <= 64 && design_inverse_makes_v(h->sw, nz))",
                 "if (with_v) launch_neg_gm_batched(st, gb, nz, nzs, n, h->bG, h->bFs, h->bVs, ds.G, ds.Fs);",
                 "h->minv_packed = design_inverse_can_pack(h->sw, nz);",
                 "if (design_inverse_makes_rho(h->sw, nz, nzs))",
                 "hipLaunchKernelGGL(k_design_rho, dim3(1, gb), dim3(256), 0, st, nz, nzs, h->rho_mode, rho, h->bG, h->bRho, ds.G, ds.rho);",
                 "h->minv_packed ? 1 : 0);"):
        assert text in lbf, text
    assert lbf.count("launch_design_inverse(") == 6 and lbf.count("dim3(1, gb)") == 8     # (every inverse: grid.y = the batch)
    for text in ("inline bool design_inverse_makes_rho(const Switches& sw, int nz, int nzs) { return nz <= 64 && nzs <= 64 && !sw.inv_tile && !sw.no_rho_fusion; }",
                 "inline bool design_inverse_can_pack(const Switches& sw, int nz) { return nz > 64 && nz <= 128 && (nz & 1) == 0 && !sw.inv_tile && !sw.no_packed_minv; }",
                 "inline bool design_inverse_makes_v(const Switches& sw, int nz) { return nz <= 128 && !sw.inv_tile && !sw.dbg_split_neggm; }"):
        assert text in des, text
    # the inverse kernel
    ldi = _function(des, "inline void launch_design_inverse(const Switches& sw, dim3 grid,")
    for text in ("if (nz <= 64 && !sw.inv_tile) {",
                 "const dim3 g2((unsigned)(((Out2 ? 2 * b : b) + 3) / 4));",
                 "hipLaunchKernelGGL((k_design_inverse_wave<NC_>), g2, dim3(256),",
                 "if (nz <= 16) INV_WAVE(16); else if (nz <= 32) INV_WAVE(32); else if (nz <= 48) INV_WAVE(48); else INV_WAVE(64);",
                 "} else if (nz <= 64) hipLaunchKernelGGL((k_design_inverse_t<2, 8>), grid,",
                 "else if (!sw.inv_tile) {",
                 "const long cw = sw.inv_columns_per_wave.value_or(grid.y <= 256 ? 16 : 32);",
                 "if (grid.y <= 256) { if (cw == 8) INV_C32(8, true); else if (cw == 16) INV_C32(16, true); else INV_C32(32, true); }",
                 "else { if (cw == 8) INV_C32(8, false); else if (cw == 16) INV_C32(16, false); else INV_C32(32, false); }",
                 "else hipLaunchKernelGGL((k_design_inverse_t<4, 16>), grid,"):
        assert text in ldi, text
    assert ic.INV_WAVES_PER_WG == 256 // 64 and ic.C32_THROUGHPUT_ABOVE == 256
    assert re.search(r"template <int AR, int KC, int NG = 8>[^\n]*\n[^\n]*void k_design_inverse_t\(", des)   # (<2, 8> is <2, 8, 8>)
    ngm = _function(des, "inline void launch_neg_gm_batched(hipStream_t st,")
    assert "const size_t lds = (size_t)ncols * nz * sizeof(double);" in ngm
    for nc in ic.NEG_GM_BUILDS:
        assert "if (nz <= 128 && ncols <= %d && lds <= 48 * 1024) hipLaunchKernelGGL((k_neg_gm_cols<%d>), dim3(1, batch)," % (nc, nc) in ngm, nc
    assert "else hipLaunchKernelGGL(k_neg_gm, dim3(4, batch)," in ngm
    # the step: layout, route, finish, persistent grid, rollout
    for text in ("const bool blocked = !h->batched && h->roll_s > 0;",
                 "L.fused = roll.fits || blocked;",
                 "if (L.fused && !blocked && (h->N + 1) * (h->n + h->m) > per_wave) per_wave = (h->N + 1) * (h->n + h->m);",
                 "per_wave = (per_wave + 1) & ~1;",
                 "L.wave_const_off = per_wave;",
                 "per_wave += (h->nzs + h->n * (h->n + h->m) + 1) & ~1;",
                 "if (L.l_glds + slot <= 160 * 1024 && !h->batched && !h->sw.polish_sg_global) {",
                 "if (!s.o.polish) return Route::NoPolish;",
                 "if (h->batched && s.mode.guess == Guess::Admm && h->nzs <= 64 && L.fused && !h->sw.no_inst_wave &&",
                 "((size_t)L.SL.total + (size_t)L.per_wave + (size_t)h->nz * h->nzs) * sizeof(double) <= 64 * 1024)",
                 "return Route::WaveInst;", "return Route::TwoLaunch;",
                 "case Route::WaveInst: rc = step_wave(s, L, false); break;",
                 "if (h->nzs <= 16) HIP_TRY(h, launch_step_inst_wave_t<16>(h, ip, pp, lds));",
                 "else if (h->nzs <= 32) HIP_TRY(h, launch_step_inst_wave_t<32>(h, ip, pp, lds));",
                 "else if (h->nzs <= 48) HIP_TRY(h, launch_step_inst_wave_t<48>(h, ip, pp, lds));",
                 "else HIP_TRY(h, launch_step_inst_wave_t<64>(h, ip, pp, lds));",
                 "hipLaunchKernelGGL((k_step_inst_wave<NZC>), dim3((unsigned)h->batch), dim3(64), lds, h->stream, ip, pp);",
                 'if (h->batched && !L.fused) return fail(h, ALMPC_ERR_UNSUPPORTED, "calculate: per-instance models need the fused rollout (n + m <= 8 * lanes-per-row)");',
                 "const size_t sgl_wave = (size_t)L.per_wave + POLISH_GLB_PER_INST + (size_t)h->nz * h->nzs;",
                 "const size_t l_sgl = ((size_t)L.SL.total + sgl_wave) * sizeof(double);",
                 "if (L.l_glds <= 160 * 1024 && !h->sw.polish_no_glds && !h->batched) {",
                 "} else if (h->batched && h->batch <= 2 * h->num_cus && l_sgl <= 160 * 1024 && !h->sw.polish_sg_global) {",
                 "HIP_TRY(h, guess_ws ? launch_polish_sgl<1>(pp, l_sgl, st) : launch_polish_sgl<0>(pp, l_sgl, st));",
                 "hipLaunchKernelGGL((k_polish<false>), dim3((pp.ntiles * 16 + POLISH_WAVES - 1) / POLISH_WAVES), dim3(64 * POLISH_WAVES), l, st, pp);",
                 "const bool packed = h->minv_packed;",
                 "const int wgs = h->num_cus * 2 > h->batch ? h->batch : h->num_cus * 2;",
                 "HIP_TRY(h, packed ? launch_admm_inst<true>(ip, wgs, l, st) : launch_admm_inst<false>(ip, wgs, l, st));",
                 "if (!h->batched && (shared + 4 * per_wave) * sizeof(double) <= 60 * 1024) {",
                 "hipLaunchKernelGGL((k_rollout<1>), dim3(h->batch), dim3(64), l, h->stream, rp);",
                 "if (h->batched) { rp.A_stride = (long)h->n * h->n; rp.B_stride = (long)h->n * h->m; rp.d_stride = h->nzs; rp.dvec = h->bD; }"):
        assert text in api, text


def test_the_restated_rules_at_known_shapes():
    assert ic.design_instance_lds_doubles(1, 1, 1) == 12 and not ic.scale_in_tail(1, 1, 1)
    assert ic.design_instance_lds_doubles(16, 1, 59) == 21120 and ic.design_route(16, 1, 59) == "dense" and ic.pick_route(16, 1, 59) == "wave"
    assert ic.design_instance_lds_doubles(16, 2, 50) == 22112 and ic.design_route(16, 2, 50) == "dense"
    assert ic.design_instance_lds_doubles(16, 8, 16) == 15744 and ic.design_route(16, 8, 16) == "lds" and ic.scale_in_tail(16, 8, 16)
    assert not ic.scale_in_tail(4, 2, 20, {"ALMPC_DBG_SPLIT_SCALE": "0"})      # (ON_IF_SET: any value switches it on)
    assert [ic.design_build(n, m) for n, m in ((12, 4), (4, 2), (2, 1), (4, 1), (12, 3))] == [(12, 4), (4, 2), (2, 1), (0, 0), (0, 0)]
    # the one-launch mode: scalar rho, nz <= 64; the stiffness profile and every switch of the chain take two inverse launches
    f = ic.factor_plan(4, 2, 20)
    assert f["one_launch"] and f["v_in_inverse"] and not f["rho_kernel"] and not f["packed"] and f["inverses"] == [("wave", 48)] and not f["scale"]
    f = ic.factor_plan(4, 2, 20, profile="stiffness")
    assert not f["one_launch"] and f["v_in_inverse"] and f["neg_gm"] is None and f["inverses"] == [("wave", 48)] * 2
    f = ic.factor_plan(4, 2, 20, env=ic.SPLIT)
    assert f["scale"] and not f["one_launch"] and f["neg_gm"] == 4 and not f["rho_kernel"]
    f = ic.factor_plan(4, 2, 20, env={"ALMPC_NO_RHO_FUSION": "1"})
    assert not f["one_launch"] and f["rho_kernel"] and f["v_in_inverse"]
    f = ic.factor_plan(4, 2, 20, env={"ALMPC_INV_TILE": "1"})
    assert f["inverses"] == [("tile", 2, 8, 8)] * 2 and f["rho_kernel"] and f["neg_gm"] == 4
    # nz > 64: V by k_neg_gm_cols, the profile by k_design_rho, the packed triangle for even nz
    f = ic.factor_plan(2, 2, 33)
    assert f["packed"] and f["neg_gm"] == 4 and f["rho_kernel"] and f["inverses"] == [("c32", 16, True)] * 2
    assert not ic.factor_plan(5, 13, 5)["packed"] and not ic.factor_plan(2, 2, 33, env={"ALMPC_NO_PACKED_MINV": "1"})["packed"]
    assert ic.factor_plan(2, 2, 33, batch=257)["inverses"][0] == ("c32", 32, False)
    assert ic.factor_plan(2, 2, 33, batch=257, env={"ALMPC_INV_CW": "8"})["inverses"][0] == ("c32", 8, False)
    assert ic.factor_plan(2, 2, 33, env={"ALMPC_INV_CW": "12"})["inverses"][0] == ("c32", 32, True)
    assert ic.factor_plan(16, 2, 50, env={"ALMPC_INV_TILE": "1"})["inverses"][0] == ("tile", 4, 16, 8)
    assert [ic.neg_gm_build(n, 100) for n in (1, 4, 5, 8, 9, 16, 17)] == [4, 4, 8, 8, 16, 16, 0]
    assert ic.wave_inverse_grid(37, False) == (10, 1) and ic.wave_inverse_grid(37, True) == (19, 2) and ic.wave_inverse_grid(4, False) == (1, 4)
    # the step
    assert ic.pick_route(4, 2, 20) == "wave" and ic.pick_route(4, 2, 20, env=ic.NO_WAVE) == "two" and ic.pick_route(4, 2, 20, polish=False) == "nopolish"
    assert ic.pick_route(4, 2, 20, env={"ALMPC_NO_INST_WAVE": "0"}) == "wave"       # (ON_IF_1)
    assert ic.pick_route(5, 13, 5) == "two" and ic.finish(5, 13, 5) == "sgl" and ic.finish(5, 13, 5, env=ic.SG_GLOBAL) == "l2"
    assert ic.finish(5, 13, 5, batch=513) == "l2" and ic.finish(5, 13, 5, batch=512) == "sgl"
    assert ic.finish(12, 4, 30) == "l2" and ic.sgl_lds_bytes(12, 4, 30) == 21092 * 8 and ic.finish(16, 2, 50) == "sgl"
    assert ic.finish(17, 1, 17) == "unsupported"
    assert ic.admm_inst_grid(37) == 37 and ic.admm_inst_grid(512) == 512 and ic.admm_inst_grid(515) == 512
    assert ic.step_kernels(12, 4, 30) == (("admm_inst", True), ("polish", "l2")) and ic.step_kernels(5, 13, 5, polish=False) == (("admm_inst", False), ("rollout", 1))
    assert ic.step_kernels(16, 4, 16) == (("step_inst_wave", 64),)


def test_the_one_wave_step_always_fits_its_64_kib():
    """pick_route asks for (total + per_wave + nz nzs) doubles <= 64 KiB before it takes the one-wave step.  Wherever its other
    conditions hold -- nzs <= 64 and the rollout in the finish's tail: (N + 1)(n + m) <= 1024, n + m <= 8 lanes-per-row -- the sum is
    at most 4096 + (128 + 2 m + n (n + m) + (N + 1) n) + (1024 + 64 + n (n + m)) doubles with n (n + m) <= 512: the condition cannot
    fail, so the table has no row on its far side (every shape with nz <= 64 is enumerated here)."""
    worst = 0
    for n in range(1, 65):
        for m in range(1, 65):
            for N in range(1, 64 // m + 1):
                if ic.polish_layout(n, m, N)["fused"]:
                    worst = max(worst, ic.wave_step_lds_bytes(n, m, N))
    assert 48 * 1024 < worst <= 64 * 1024


# ---------------------------------------------------------------------------- the table against the builds
def test_the_table_reaches_every_instantiated_build_and_route():
    r = ic.reached()
    assert r["design"] == set(ic.DESIGN_BUILDS)
    assert r["design_route"] == {"lds", "dense"}
    assert r["scale_in_tail"] == {True, False}
    assert r["inv_wave"] == set(ic.INV_WAVE_BUILDS)
    assert r["inv_c32"] == set(ic.INV_C32_BUILDS)
    assert r["inv_tile"] == set(ic.INV_TILE_BUILDS)
    assert r["neg_gm"] == set(ic.NEG_GM_BUILDS)
    assert r["rho_kernel"] == {(False, True), (True, True), (True, False)}      # (k_design_rho runs, nz <= 64)
    assert r["one_launch"] == {True, False} and r["packed"] == {True, False}
    assert r["admm_inst"] == set(ic.ADMM_INST_BUILDS) and r["admm_inst_rounds"] == {True, False}
    assert r["step_wave"] == set(ic.WAVE_BUILDS)
    assert r["finish"] == {"sgl", "l2"} and r["rollout"] == {1}
    assert r["wave_inverse_partial"] >= {(True, True), (False, True)}           # a partial last workgroup in both modes
    for c in ic.CASES:
        assert c.nz <= 128 and c.n <= 16 and ic.finish(*c.shape) != "unsupported", c.id


def test_the_table_holds_the_required_rows():
    ids = [c.id for c in ic.CASES]
    assert ids == ["1-1-1", "3-2-6", "16-1-16", "2-1-17", "4-2-16", "13-3-11", "12-4-12", "3-24-2", "5-7-7", "16-1-59", "16-4-16", "4-2-32-heavy",
                   "5-13-5", "2-2-33", "3-23-3", "4-2-40", "6-3-30-heavy", "2-1-97", "16-2-50", "6-4-30", "12-4-30", "3-1-127", "16-8-16",
                   "2-2-5-b515", "4-2-36-b515"]
    b37 = [c for c in ic.CASES if c.batch == ic.BATCH]
    # every wave build at exact fit and one past it, on the one-wave step by default and on k_admm_inst<false> + both finishes without it
    assert {1, 12, 16, 17, 32, 33, 48, 49, 59, 64} <= {c.nz for c in b37}
    for c in b37:
        if c.nz <= 64:
            assert c.route == "wave" and ic.step_kernels(*c.shape, env=ic.NO_WAVE) == (("admm_inst", False), ("polish", "sgl")), c.id
            assert ic.NO_WAVE in c.step_envs()
    assert not ic.scale_in_tail(1, 1, 1) and ic.design_route(1, 1, 1) == "lds"
    assert ic.design_route(16, 1, 59) == "dense" and ic.design_route(16, 2, 50) == "dense"
    # every specialised design build with m N on both sides of 64
    for nm in ic.DESIGN_BUILDS[:3]:
        assert {c.nz <= 64 for c in b37 if (c.n, c.m) == nm and ic.design_route(*c.shape) == "lds"} == {True, False}, nm
    assert {c.nz <= 64 for c in b37 if ic.design_build(c.n, c.m) == (0, 0) and ic.design_route(*c.shape) == "lds"} == {True, False}
    # nz above 64
    big = [c for c in b37 if c.nz > 64]
    assert {65, 66, 69, 100, 120, 127, 128} <= {c.nz for c in big}
    assert {ic.factor_plan(*c.shape)["neg_gm"] for c in big} == {4, 8, 16}
    assert {ic.factor_plan(*c.shape)["packed"] for c in big} == {True, False}
    assert {ic.finish(*c.shape) for c in big if not c.heavy} == {"sgl", "l2"}
    assert min(ic.sgl_lds_bytes(*c.shape) for c in big) < ic.LDS_MAX < max(ic.sgl_lds_bytes(*c.shape) for c in big)
    # the switch rows
    def has(env, pred=lambda c: True):
        return [c for c in ic.CASES if env in c.envs and pred(c)]
    assert {ic.finish(*c.shape, env=ic.NO_WAVE) for c in ic.CASES if any(ic.on(e, "ALMPC_POLISH_SG_GLOBAL") for e in c.envs)} == {"sgl"}
    assert has(ic._SGW, lambda c: c.nz <= 64 and not c.heavy) and has(ic.SG_GLOBAL, lambda c: c.nz > 64 and not c.heavy)
    assert has(ic._TILE, lambda c: c.nz <= 64) and has(ic._TILE, lambda c: c.nz > 64)
    for cw in (8, 16, 32):
        assert has(ic._cw(cw), lambda c: c.nz > 64 and c.batch == ic.BATCH), cw
    assert has(ic._cw(8), lambda c: c.batch > 256) and has(ic._cw(16), lambda c: c.batch > 256)
    assert any(c.batch > 256 and c.nz > 64 and ic.inverse_build(c.nz, c.batch, {}) == ("c32", 32, False) for c in ic.CASES)
    assert has(ic._NORHO, lambda c: c.nz <= 64) and has(ic._NOPACK, lambda c: c.nz > 64 and c.nz % 2 == 0)
    assert has(ic.SPLIT, lambda c: c.nz <= 64 and c.shape != (4, 2, 20))
    assert {ic.factor_plan(*c.shape, env=ic.SPLIT)["neg_gm"] for c in has(ic.SPLIT)} == {4, 8, 16}
    # large batches at small shapes
    small, even = ic.CASE_BY_ID["2-2-5-b515"], ic.CASE_BY_ID["4-2-36-b515"]
    assert small.nz <= 16 and small.batch == ic.BIG == 515 and ic.step_kernels(*small.shape, small.batch, env=ic.NO_WAVE) == (("admm_inst", False), ("polish", "l2"))
    assert ic.wave_inverse_grid(515, False)[1] == 3 and ic.wave_inverse_grid(515, True)[1] == 2
    assert 66 <= even.nz <= 80 and even.nz % 2 == 0 and ic.step_kernels(*even.shape, even.batch) == (("admm_inst", True), ("polish", "l2"))
    assert small.exact[-3:] == even.exact[-3:] == (512, 513, 514) and small.exact[:3] == (0, 20, 40)
    assert [c.batches for c in ic.CASES if c.batches] == [(1, 3, 4, 5)] and ic.CASE_BY_ID["3-2-6"].route == "wave"
    # one heavy case per finish, the second tier in LDS and in the global scratch
    h64, h90 = ic.CASE_BY_ID["4-2-32-heavy"], ic.CASE_BY_ID["6-3-30-heavy"]
    assert [ic.step_kernels(*h64.shape, env=e)[-1] for e in h64.step_envs()] == [("step_inst_wave", 64), ("polish", "sgl"), ("polish", "l2")]
    assert [ic.step_kernels(*h90.shape, env=e)[-1] for e in h90.step_envs()] == [("polish", "sgl"), ("polish", "l2")]
    assert set(ic.HEAVY_BANDS) == {c.id for c in ic.HEAVY}
    # the freeze rows: a one-wave case, a k_admm_inst case, and the persistent grid's second round
    fr = ic.tagged("freeze")
    assert any(c.route == "wave" and c.batch == ic.BATCH for c in fr) and any(c.route == "two" and c.batch == ic.BATCH for c in fr)
    assert any(c.batch > ic.admm_inst_grid(c.batch) for c in fr)
    assert {ic.design_build(c.n, c.m) for c in ic.CASES if c.shape == ic.QUAD} == {(12, 4)}


# ---------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.id)
def test_inputs_cannot_hide_a_failure(case):
    A, B = ic.models(case)
    flat = np.concatenate([A.reshape(case.batch, -1), B.reshape(case.batch, -1)], axis=1)
    assert len({r.tobytes() for r in flat}) == case.batch                       # no two instances share a model
    assert min(np.abs(flat[i] - flat[j]).max() for i in range(0, case.batch, 7) for j in range(i)) > 1e-3
    cap_h, cap_m = (COND_H_QUAD, COND_M_QUAD) if case.id == QUAD_ID else (COND_H, COND_M)
    for profile, rho in ic.PROFILES:
        for i, d in enumerate(ic.designs(case, profile, rho)):
            assert np.linalg.cond(d["Hs"]) <= cap_h, (i, profile)
            assert np.linalg.cond(d["Hs"] + d["sigma"] * np.eye(case.nz) + np.diag(d["rho_vec"])) <= cap_m, (i, profile)
    t = ic.template(case)
    assert np.abs(mo.s_rate_gradient(t)).max() > 0 or case.N <= 2 or case.id == QUAD_ID     # fS is not zero
    assert np.array_equal(t.P, 20.0 * np.eye(case.n)) or case.id == QUAD_ID
    ref = ic.reference(case)
    assert sorted(ref["exact"]) == sorted(set(case.exact))
    for i in case.exact:
        assert np.all(ref["exact"][i]["u"] <= t.u_max[:, None] + 1e-12) and np.all(ref["exact"][i]["u"] >= t.u_min[:, None] - 1e-12)
    i0 = case.exact[1]
    assert np.abs(mo.solve_mpc_exact(ic.problem(case, i0), ref["X0"][i0])["u"] - ref["exact"][i0]["u"]).max() <= 1e-12
    na = ic.active_counts(case)
    assert na.max() >= 1
    if case.heavy:
        assert na.max() <= 60
        assert (((na >= 33) & (na <= 48)).any(), ((na >= 49) & (na <= 60)).any()) == ic.HEAVY_BANDS[case.id]
    else:
        assert na.max() <= 32


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.id)
def test_the_iterate_tolerance_sees_a_wrong_operand(case):
    """What the GPU iterate test can see, on the oracle alone: a relative error of 1e-6 in the LAST element of Minv_i (the end of the
    packed triangle) or of F'_i moves the seventh iterate of some instance by more than the 1e-9 max(1, |v|) the test allows, on
    both penalty profiles -- the inputs do not make the iterate blind to an operand"""
    X0, t = ic.x0(case), ic.template(case)
    kw = dict(max_iter=7, check_every=7)
    for profile, rho in ic.PROFILES:
        des = ic.designs(case, profile, rho)
        for key in ("Minv", "Fs"):
            moved = 0.0
            for i in range(min(case.batch, ic.BATCH)):
                p = ic.problem(case, i)
                u0 = cc.admm_u(p, des[i], cc.admm(des[i], cc.fs_of(p, des[i], X0[i]), **kw))
                wrong = dict(des[i])
                a = np.array(des[i][key])
                a[-1, -1] *= 1.0 + 1e-6
                wrong[key] = a
                u1 = cc.admm_u(p, wrong, cc.admm(wrong, cc.fs_of(p, wrong, X0[i]), **kw))
                moved = max(moved, float(np.abs(u1 - u0).max() / max(1.0, np.abs(u0 - t.u_ref).max())))
            assert moved > 10 * 1e-9, (profile, key, moved)


def test_some_instances_have_no_active_row():
    assert sum(int((ic.active_counts(c) == 0).sum()) for c in ic.CASES[:4]) >= 1


@pytest.mark.parametrize("case", ic.tagged("freeze"), ids=lambda c: c.id)
def test_freeze_inputs_stop_at_different_checks_and_far_from_the_threshold(case):
    """Equal iteration counts can be asked of the device without an allowance: no residual of any check lies within 1e-6 (relative)
    of its threshold, and neighbours in the grid stop at different checks"""
    X0 = ic.freeze_x0(case)
    des = ic.designs(case, *ic.PROFILES[0])
    iters = []
    for i in range(case.batch):
        p = ic.problem(case, i)
        trace = []
        r = cc.admm(des[i], cc.fs_of(p, des[i], X0[i]), trace=trace, **ic.FREEZE_OPTS)
        iters.append(r["iters"])
        assert r["status"] == 0 and len(trace) == r["iters"] // ic.FREEZE_OPTS["check_every"]
        for rp, tp, rd, td in trace:
            assert abs(rp - tp) > 1e-6 * tp and abs(rd - td) > 1e-6 * td, i
    assert len(set(iters)) >= 2 and any(a != b for a, b in zip(iters[:-1], iters[1:]))
    if case.batch > ic.admm_inst_grid(case.batch):
        assert len(set(iters[ic.admm_inst_grid(case.batch):] + iters[:3])) >= 2
