"""CPU tests of the case table behind tests/test_gpu_nlp_shapes.py (tests/nlp_shape_cases.py): the Python restatement of the host's
dispatch -- linearisation build, time-varying design build, the SQP step's chunks, the exact mode's limits, the fused Jacobian head --
uses the text, the constants and the build lists of the source (a threshold that moves fails here); the table reaches every build of
k_fnn_jacobian_w and k_design_ltv_reg that csrc/instances/*.inc instantiate, every network kind of k_fnn_jacobian, k_fnn_rollout and
k_fnn_lag_hessian, k_design_ltv, a chunked and an unchunked k_sqp_step and the four k_design_instance_t builds with the Jacobian as
their head; and the references are ones on which the GPU tests cannot hide a failure: the float64 restatement of the networks is held
against long double, every QP of every SQP and time-varying case solves, has an input on a bound and is strictly complementary with
margin, on every instance."""
import os
import re

import numpy as np
import pytest

import densenet_ref as dr
import nlp_shape_cases as nc
import sqp_exact_ref as ex
from conftest import ROOT

CSRC = os.path.join(ROOT, "automationlabsmodelpredictivecontrol.jl_amd", "csrc")
_ids = lambda c: c.id


def _read(*parts):
    with open(os.path.join(CSRC, *parts)) as f:
        return f.read()


def _builds(kernel, src):
    return sorted(tuple(int(t) for t in m.split(",")) for m in re.findall(r"almpc::%s<([^>]*)>\(" % kernel, src))


def _function(src, head):
    body = src[src.index(head):]
    return body[:body.index("\n}\n")]


# ---------------------------------------------------------------------------- the restatement against the source
def test_the_restatement_uses_the_constants_and_builds_of_the_source():
    api, fnn, sqp, inst = _read("almpc_api.hip"), _read("almpc_fnn.hip.h"), _read("almpc_sqp.hip.h"), _read("almpc_instance.hip.h")
    da, db = _read("instances", "design_a.inc"), _read("instances", "design_b.inc")
    # the build lists: a build added later without a case fails here
    assert _builds("k_fnn_jacobian_w", db) == sorted(nc.FNN_W_BUILDS)
    assert _builds("k_design_ltv_reg", da) == sorted((nc_, 4) for nc_ in nc.LTV_REG_BUILDS)
    for name in ("k_fnn_", "k_design_ltv", "k_sqp_"):
        for other in os.listdir(os.path.join(CSRC, "instances")):
            if other not in ("design_a.inc", "design_b.inc"):
                assert name not in _read("instances", other), (name, other)
    assert len(re.findall(r"almpc::k_fnn_\w+<", db)) == 8 and len(re.findall(r"almpc::k_design_ltv\w*<", da)) == 5
    # (k_fnn_jacobian, k_fnn_rollout, k_fnn_lag_hessian are instantiated where with_net names them: one build per kind)
    assert "constexpr int NET_FNN = 0, NET_RESNET = 1, NET_POLYNET = 2;" in fnn and "constexpr int NET_DENSENET = 3;" in fnn
    wn = _function(api, "static auto with_net(int net, F pick)") if "static auto with_net(int net, F pick)" in api else api
    for k in ("NET_RESNET", "NET_POLYNET", "NET_DENSENET", "NET_FNN"):
        assert "pick(std::integral_constant<int, %s>())" % k in wn, k
    for text in ("with_net(net, [](auto k) { return k_fnn_jacobian<k>; })", "with_net(q.net, [](auto k) { return k_fnn_rollout<k>; })"):
        assert text in api, text
    assert re.search(r"with_net\([^\n]*k_fnn_lag_hessian<k>", api)
    # the linearisation
    assert "constexpr int FNN_W_WAVES = %d;" % nc.FNN_W_WAVES in fnn
    for head, texts in (
            ("inline size_t densenet_wh_offset(int H, int l) {", ("return (size_t)H * H * l * (l + 1) / 2;",)),
            ("inline size_t fnn_weights_doubles(int n, int m, int H, int L, int net = NET_FNN) {",
             ("if (net == NET_DENSENET) return (size_t)H * (n + m) + densenet_wh_offset(H, L) + (size_t)L * H + (size_t)n * (L + 1) * H;",
              "return (size_t)H * (n + m) + (size_t)L * H * H + (size_t)L * H + (size_t)n * H;")),
            ("inline size_t fnn_wave_scratch_doubles(int n, int m, int H, int L, int net = NET_FNN) {",
             ("if (net == NET_DENSENET) return (size_t)(L + 1) * H * (1 + n + m) + H + (n + m);",
              "return 2 * (size_t)H + 2 * (size_t)H * (n + m) + (n + m) + (net == NET_POLYNET ? (size_t)H : 0);")),
            ("inline size_t fnn_w_lds_doubles(int n, int m, int H, int L, int ppw = 1, int net = NET_FNN) {",
             ("return fnn_weights_doubles(n, m, H, L, net) + FNN_W_WAVES * ppw * fnn_wave_scratch_doubles(n, m, H, L, net);",))):
        assert head in fnn, head
        for t in texts:
            assert t in (fnn[fnn.index(head):][:600]), t
    for text in ("constexpr int PPW = 64 / LW;", "const int stride = gridDim.x * FNN_W_WAVES * PPW;",
                 "for (int i0 = (blockIdx.x * FNN_W_WAVES + wv) * PPW; i0 < p.batch; i0 += stride) {",
                 "const bool valid = inst_ < p.batch;", "const int inst = valid ? inst_ : 0;"):
        assert text in fnn, text
    lfj = _function(api, "hipError_t launch_fnn_jacobian(const Switches& sw, const FnnParams& p, int net, int num_cus, hipStream_t st) {")
    for text in ("const int ppw = ((size_t)p.H * nin <= %d && !sw.fnn_one_point_per_wave) ? 2 : 1;" % nc.PPW2_MAX,
                 "const size_t lw = fnn_w_lds_doubles(p.n, p.m, p.H, p.L, ppw, net) * sizeof(double);",
                 "if (lw <= 64 * 1024 && !sw.fnn_wg) {",
                 "int wgs = (p.batch + FNN_W_WAVES * ppw - 1) / (FNN_W_WAVES * ppw);",
                 "const int cap = num_cus * %d;" % nc.WG_CAP_PER_CU, "if (wgs > cap) wgs = cap;",
                 "return ppw == 2 ? k_fnn_jacobian_w<32, k> : k_fnn_jacobian_w<64, k>;",
                 "const size_t lds = fnn_wave_scratch_doubles(p.n, p.m, p.H, p.L, net) * sizeof(double);",
                 "if (lds > 64 * 1024) {", "hipLaunchKernelGGL(kern, dim3(p.batch), dim3(256), lds, st, p);"):
        assert text in lfj, text
    assert api.count("if (fnn_wave_scratch_doubles(n, m, H, L, net) * sizeof(double) > 160 * 1024)") >= 2      # linearize, relin setup
    # the time-varying design
    assert "constexpr int LTV_REG_NZ = %d;" % nc.LTV_REG_NZ in inst
    assert "return nz * nz + 3 * (size_t)n * nz + 4 * (size_t)n * n + (size_t)n * m + 3 * (size_t)n + nz;" in _function(
        inst, "inline size_t design_ltv_lds_doubles(int n, int m, int N) {")
    assert ("return 4 * (size_t)n * LTV_REG_NZ + 4 * (size_t)n * n + 2 * (size_t)n * m + 4 * (size_t)n + 2 * (size_t)N * n + 2 * (size_t)m * m;"
            in _function(inst, "inline size_t design_ltv_reg_lds_doubles(int n, int m, int N) {"))
    for text in ("return h->nz <= LTV_REG_NZ && n * n + n * m <= 1024 - n && design_ltv_reg_lds_doubles(n, m, h->N) * sizeof(double) <= 160 * 1024 &&",
                 "!h->sw.ltv_lds;",
                 "return ltv_reg_path(h) || design_ltv_lds_doubles(h->n, h->m, h->N) * sizeof(double) <= 160 * 1024;",
                 "hipLaunchKernelGGL((k_design_ltv_reg<NC, 4>), dim3((unsigned)h->batch), dim3(1024), lds, st, lp);",
                 "hipLaunchKernelGGL(k_design_ltv, dim3((unsigned)h->batch), dim3(256), lds, st, lp);"):
        assert text in api, text
    ldl = _function(api, "hipError_t launch_design_ltv(almpc_handle* h, const DesignLtvParams& lp, hipStream_t st) {")
    for nc_ in nc.LTV_REG_BUILDS[1:]:
        assert "case %d: return launch_design_ltv_reg<%d>(h, lp, lds, st);" % (nc_, nc_) in ldl, nc_
    assert "default: return launch_design_ltv_reg<0>(h, lp, lds, st);" in ldl and ldl.count("launch_design_ltv_reg<") == len(nc.LTV_REG_BUILDS)
    for text in ("if (N > 1) AB[nab + tid] = ab_load(1);", "if (N > 2) pre = ab_load(2);", "if (k + 2 < N) AB[(k & 1) * nab + tid] = pre;",
                 "if (k + 3 < N) pre = ab_load(k + 3);", "const int ni = (wcols + DX - 1) / DX;"):
        assert text in inst, text
    for text in ("c.ltv_scales = !c.exact && ltv_reg_path(h) && nz <= 128 && !q.structured_qp && !h->sw.dbg_split_scale;",
                 "c.prep_in_design = c.ltv_scales && !h->sw.dbg_split_prepare;"):
        assert text in api, text
    # the SQP glue
    ssc = _function(sqp, "inline int sqp_step_chunk(int n, int m, int N) {")
    for text in ("const long E = (long)n * n + (long)n * m + n, fixed = (long)(N + 1) * n + (long)m * N + 16;",
                 "long ch = (%d - fixed) / E;" % nc.STEP_LDS_DOUBLES, "return (int)(ch < 1 ? 1 : (ch > N ? N : ch));"):
        assert text in ssc, text
    assert ("return (size_t)sqp_step_chunk(n, m, N) * ((size_t)n * n + (size_t)n * m + n) + (size_t)(N + 1) * n + (size_t)m * N + 16;"
            in _function(sqp, "inline size_t sqp_step_lds_doubles(int n, int m, int N) {"))
    for text in ("if (n > 64 || sqp_step_lds_doubles(n, m, N) * sizeof(double) > 160 * 1024)", "if (!sq_struct && !ltv_supported(h))",
                 "if (c.step_lds > 64 * 1024) HIP_TRY(h, ensure_dyn_lds(reinterpret_cast<const void*>(k_sqp_step), (size_t)(c.step_lds)));",
                 'if (h->batched && !L.fused) return fail(h, ALMPC_ERR_UNSUPPORTED, "calculate: per-instance models need the fused rollout (n + m <= 8 * lanes-per-row)");',
                 "h->batched = true; h->ltv = true;"):
        assert text in api, text
    # the exact mode
    fhw = _function(sqp, "inline size_t fnn_hess_wave_doubles(int n, int m, int H, int L, int net = NET_FNN) {")
    for text in ("const size_t nin = (size_t)n + m, S = net == NET_POLYNET ? 2 * (size_t)L : (size_t)L;",
                 "if (net == NET_DENSENET) return nin + (2 * (size_t)(L + 1) + 1) * H + (size_t)(L + 1) * H * nin + 2 * S * H + S * H * nin;",
                 "return nin + 3 * (size_t)H + (size_t)H * nin + 2 * S * H + S * H * nin;"):
        assert text in fhw, text
    assert ("return 2 * (size_t)n * nz + 2 * (size_t)n + nin * nz + nin + nin * nin + (size_t)n * n + (size_t)n * m + n + 8;"
            in _function(sqp, "inline size_t sqp_exact_lds_doubles(int n, int m, int nz) {"))
    sec = _function(api, "static int sqp_exact_check(almpc_handle* h) {")
    for text in ("if (q.act == 1) return fail(h, ALMPC_ERR_UNSUPPORTED,", "if (h->nz > 128) return fail(h, ALMPC_ERR_UNSUPPORTED,",
                 "if (4 * fnn_hess_wave_doubles(h->n, h->m, q.H, q.L, q.net) * sizeof(double) > 64 * 1024)",
                 "if (sqp_exact_lds_doubles(h->n, h->m, h->nz) * sizeof(double) > 64 * 1024)"):
        assert text in sec, text
    assert sec.count("return fail(h, ALMPC_ERR_UNSUPPORTED") == 7     # (a limit added later: restate it in exact_supported)
    # the re-linearisation
    dff = _function(api, "bool design_fuses_fnn(const almpc_handle* h, int H, int L, int net) {")
    for text in ("if (net != NET_FNN) return false;",
                 "const size_t lds = (design_instance_lds_doubles(h->n, h->m, h->N) + fnn_weights_doubles(h->n, h->m, H, L) + fnn_wave_scratch_doubles(h->n, h->m, H, L)) * sizeof(double);",
                 "return lds <= 160 * 1024 && !h->sw.dbg_split_jacobian;"):
        assert text in dff, text
    for text in ("const bool fuse_jac = !h->structured && design_fuses_fnn(h, q.H, q.L, q.net) && !h->t_step && !h->c_step;",
                 "if (fuse_fnn) { dp.fnn_on = 1; dp.fnn_off = fnn_off; dp.fnn = *fuse_fnn; }"):
        assert text in api, text
    assert "if (p.fnn_on) {" in inst and "fnn_jacobian_point(p.fnn, blockIdx.x, threadIdx.x, wsm," in inst
    # the switches and their parsing rule
    sw = _read("almpc_switches.h")
    for name, member in (("ALMPC_FNN_ONE_POINT_PER_WAVE", "fnn_one_point_per_wave"), ("ALMPC_FNN_WG", "fnn_wg"), ("ALMPC_LTV_LDS", "ltv_lds"),
                         ("ALMPC_DBG_SPLIT_PREPARE", "dbg_split_prepare"), ("ALMPC_DBG_SPLIT_SCALE", "dbg_split_scale"),
                         ("ALMPC_DBG_SPLIT_JACOBIAN", "dbg_split_jacobian")):
        assert "X(%s, %s, ON_IF_SET," % (name, member) in sw, name


def test_the_restated_rules_at_known_shapes():
    # the linearisation
    assert nc.lin_ppw(4, 2, 32) == 2 and nc.lin_ppw(4, 2, 33) == 1 and nc.lin_ppw(4, 2, 16, nc.ONE_POINT) == 1
    assert nc.lin_build(4, 2, 16, 2) == ("w", 32, 0) and nc.lin_build(4, 2, 64, 3) == ("wg", 0, False)      # (the shapes of today's suite)
    assert nc.lin_build(4, 2, 16, 2, "polynet", nc.ONE_POINT) == ("w", 64, 2) and nc.lin_build(4, 2, 16, 2, "densenet", nc.FNN_WG) == ("wg", 3, False)
    assert nc.fnn_w_lds_doubles(2, 3, 70, 1) == 5460 + 4 * 845 and nc.lin_build(2, 3, 70, 1) == ("wg", 0, False)
    assert nc.fnn_w_lds_doubles(2, 1, 70, 1) == 5320 + 4 * 563 and nc.lin_build(2, 1, 70, 1) == ("w", 64, 0)
    assert nc.lin_build(12, 4, 300, 0) == ("wg", 0, True) and nc.fnn_wave_scratch_doubles(12, 4, 300, 0) == 10216
    assert nc.lin_build(30, 6, 5, 1) == ("w", 32, 0) and nc.lin_build(2, 1, 260, 1) == ("wg", 0, False)
    assert nc.lin_grid(7, 2) == (1, 1, 1) and nc.lin_grid(5, 1) == (2, 1, 0) and nc.lin_grid(3 * 30, 2) == (12, 1, 0)
    assert nc.big_count(2) == 16389 and nc.lin_grid(16389, 2) == (2048, 2, 1) and nc.lin_grid(8197, 1) == (2048, 2, 0)
    assert not nc.lin_supported(40, 24, 160, 1) and nc.lin_supported(12, 4, 300, 0)
    # the time-varying design
    assert [nc.ltv_build(n, 1, 5) for n in (2, 3, 4, 6, 8, 12)] == [("reg", 2), ("reg", 0), ("reg", 4), ("reg", 6), ("reg", 0), ("reg", 12)]
    assert nc.ltv_build(4, 2, 64) == ("reg", 4) and nc.ltv_build(4, 2, 65) == ("lds",) and nc.ltv_build(4, 2, 64, nc.LTV_LDS) == ("lds",)
    assert nc.ltv_build(40, 3, 40) is None                                     # (test_ltv_error_behaviour's refused shape)
    assert nc.design_ltv_lds_doubles(7, 2, 64) == 19431 and nc.design_ltv_reg_lds_doubles(24, 1, 30) * 8 == 129424
    assert nc.ltv_fused(4, 2, 50) == (True, True) and nc.ltv_fused(4, 2, 50, nc.SPLIT_PREPARE) == (True, False)
    assert nc.ltv_fused(4, 2, 50, nc.SPLIT_SCALE) == (False, False) and nc.ltv_fused(4, 2, 50, exact=True) == (False, False)
    # the SQP step: n = 4 never chunks; (24, 1, 30) walks 18 + 12 and asks for more than 64 KB
    assert all(nc.sqp_step_chunk(4, 2, N) == N for N in range(1, 65))
    assert nc.sqp_step_chunk(24, 1, 30) == 18 and nc.sqp_chunks(24, 1, 30) == [18, 12] and nc.sqp_step_lds_doubles(24, 1, 30) * 8 > nc.LDS_STATIC
    assert nc.sqp_supported(24, 1, 30) and not nc.sqp_supported(65, 1, 4)
    # ... but the step behind the QP serves n <= 16 only: no walk inside it is chunked up to N = 36, and (16, 1, 59) is the longest
    assert not nc.step_supported(24, 1, 30) and not nc.step_supported(17, 1, 12) and nc.step_supported(16, 1, 59) and not nc.step_supported(16, 1, 60)
    assert all(len(nc.sqp_chunks(n, m, N)) == 1 for n in range(1, 17) for m in range(1, 17) for N in range(1, min(36, 128 // m) + 1))
    assert nc.sqp_chunks(16, 3, 37) == [36, 1]        # (the only chunked walk with N <= 37: a last chunk of one stage)
    assert nc.sqp_chunks(16, 1, 41) == [40, 1] and nc.sqp_chunks(16, 1, 59) == [39, 20] and nc.sqp_step_lds_doubles(16, 1, 59) * 8 > nc.LDS_STATIC
    # the exact mode: the ResNet / PolyNet pair of test_sqp_exact_refuses_a_polynet_past_the_lds_budget
    assert nc.exact_supported("resnet", 4, 2, 64, 2, 10) and not nc.exact_supported("polynet", 4, 2, 64, 2, 10)
    assert not nc.exact_supported("fnn", 4, 2, 16, 2, 10, act="relu") and not nc.exact_supported("fnn", 4, 2, 16, 2, 65)
    assert nc.fnn_hess_wave_doubles(6, 2, 33, 3, "polynet") == 2351 and nc.fnn_hess_wave_doubles(6, 2, 33, 3) == 1361
    # the re-linearisation
    assert nc.design_fuses_fnn(4, 2, 20, 16, 2) and not nc.design_fuses_fnn(4, 2, 20, 16, 2, "resnet")
    assert not nc.design_fuses_fnn(4, 2, 20, 16, 2, env=nc.SPLIT_JACOBIAN) and not nc.design_fuses_fnn(16, 2, 50, 16, 2)


# ---------------------------------------------------------------------------- the table against the builds
def test_the_table_reaches_every_instantiated_build():
    r = nc.reached()
    assert r["lin_w"] == set(nc.FNN_W_BUILDS)
    assert {b[0] for b in r["lin_wg"]} == set(range(4)) and (0, True) in r["lin_wg"] and (0, False) in r["lin_wg"]
    assert r["lin_passes"] >= {(32, 1), (32, 2), (64, 1), (64, 2)}
    assert (32, 1) in r["lin_idle_half"]                                       # an odd count on two points per wave
    assert r["ltv_reg"] == set(nc.LTV_REG_BUILDS) and r["ltv_lds"] == {"ltv", "sqp"}
    for b in (0, 2, 6, 12):     # the register builds as the SQP loop runs them, with head and tail, with the tail, with neither (<4, 4>
                                # in the loop is the 4-2 model of tests/test_gpu_sqp.py; here it runs from design_ltv)
        assert {f[1:] for f in r["ltv_fused"] if f[0] == b} == {(True, True), (True, False), (False, False)}, b
    assert r["rollout"] == set(range(4)) and r["lag_hessian"] == set(range(4))
    assert r["step_chunks"] == {True, False} and r["step_dyn"] == {True, False}
    assert r["relin"] == {(b, fused) for b in nc.ic.DESIGN_BUILDS for fused in (True, False)}
    for c in nc.CASES:
        assert c.N <= (64 if c.family == "ltv" or c.net == (16, 1, 8, 1) else 37) and (c.family == "lin" or 2 <= c.batch <= 9), c.id     # ((5, 3, 42), (7, 2, 64): nz 126, 128)
        if c.family in ("sqp", "exact", "ltv"):
            assert all(nc.ltv_build(*c.shape, e) is not None for e in c.all_envs()), c.id
        if c.family in ("sqp", "exact"):
            assert nc.sqp_supported(*c.shape) and nc.lin_supported(*c.net, c.kind), c.id
            assert nc.step_supported(*c.shape) == (c not in nc.SQP_REFUSED), c.id


def test_the_table_holds_the_required_rows():
    lin = {(c.net, c.batch) for c in nc.LIN}
    for net in ((1, 1, 4, 3), (3, 1, 5, 1), (2, 3, 70, 1), (6, 2, 33, 2), (12, 4, 16, 1), (5, 2, 8, 0), (30, 6, 5, 1), (2, 1, 260, 1)):
        assert {(c.kind, c.act) for c in nc.LIN if c.net == net} == {(k, a) for k in nc.KINDS for a in nc.ACTS}, net
    ppw2 = {p for net, p in lin if nc.lin_ppw(*net[:3]) == 2}
    assert {1, 3, 7} <= ppw2 and any(p == 5 and nc.lin_ppw(*net[:3]) == 1 for net, p in lin)
    assert nc.lin_ppw(30, 6, 5) == 2 and 30 + 6 > 32
    assert any(c.H > 64 and nc.lin_build(*c.net, c.kind)[0] == "w" for c in nc.LIN)         # a second trip of the i += 64 loops, partial
    assert any(32 < c.H < 64 and nc.lin_build(*c.net, c.kind)[:2] == ("w", 32) for c in nc.LIN)
    assert any(c.H % 64 and c.H > 32 and nc.lin_build(*c.net, c.kind)[:2] == ("w", 64) for c in nc.LIN)
    assert {(c.kind, c.big) for c in nc.LIN_BIG} == {(k, p) for k in nc.KINDS for p in (1, 2)}
    for c in nc.LIN_BIG:
        env = c.envs[0] if c.envs else {}
        assert c.net == (2, 1, 4, 1) and nc.lin_ppw(c.n, c.m, c.H, env) == c.big and nc.lin_grid(c.points(), c.big)[1] == 2
        assert c.points() - nc.NUM_CUS * 8 * 4 * c.big == 5
    ltv = [c.shape for c in nc.LTV if not c.tags]
    assert ltv == [(2, 1, 1), (2, 1, 2), (2, 1, 3), (2, 4, 32), (4, 2, 3), (4, 4, 32), (4, 3, 7), (6, 8, 16), (6, 1, 5), (12, 4, 1), (12, 4, 2),
                   (12, 4, 3), (5, 3, 42), (7, 2, 64)]
    assert [s for s in ltv if s[1] * s[2] == 128] == [(2, 4, 32), (4, 4, 32), (6, 8, 16), (7, 2, 64)]
    assert all(nc.LTV_LDS in c.envs for c in nc.LTV)                              # (every row's LDS build fits 160 KB)
    assert {tuple(sorted(c.tags)) for c in nc.LTV if c.tags} == {("plain",), ("pinst",)}
    assert nc.ltv_inputs(nc.CASE_BY_ID["ltv-4-3-N7-b4-plain"])["c_all"] is None and nc.ltv_inputs(nc.CASE_BY_ID["ltv-4-3-N7-b4-plain"])["S"] is None
    assert nc.ltv_inputs(nc.CASE_BY_ID["ltv-6-1-N5-b4-pinst"])["P"].ndim == 3
    assert [c.net + (c.N,) for c in nc.SQP_REFUSED] == [(24, 1, 8, 1, 30), (17, 1, 8, 1, 12)]
    assert [(c.kind,) + c.net + (c.N,) for c in nc.SQP] == [("fnn", 16, 1, 8, 1, 59), ("resnet", 16, 1, 8, 1, 59), ("fnn", 2, 4, 12, 1, 32),
                                                          ("polynet", 6, 8, 20, 2, 16), ("densenet", 12, 4, 16, 1, 8), ("fnn", 3, 1, 5, 1, 12),
                                                          ("resnet", 1, 1, 4, 3, 7)]
    for c in nc.SQP:
        assert list(c.envs) == [nc.SPLIT_PREPARE, nc.SPLIT_SCALE, nc.LTV_LDS] and nc.ltv_fused(*c.shape) == (True, True), c.id
        assert ("chunked" in c.tags) == (len(nc.sqp_chunks(*c.shape)) > 1)
    assert [nc.ltv_build(*c.shape) for c in nc.SQP] == [("reg", 0), ("reg", 0), ("reg", 2), ("reg", 6), ("reg", 12), ("reg", 0), ("reg", 0)]
    assert {(c.net + (c.N,), c.kind) for c in nc.EXACT if len(c.tags) == 0 and c.L < 3} == {
        (s, k) for s in ((2, 3, 70, 1, 9), (6, 2, 33, 2, 16), (16, 1, 8, 1, 59)) for k in nc.KINDS}
    for c in nc.EXACT:
        assert nc.exact_supported(c.kind, *c.net, c.N, c.act) == ("refused" not in c.tags), c.id
    assert sum("refused" in c.tags for c in nc.EXACT) == 1
    assert [c.net + (c.N,) for c in nc.RELIN] == [(12, 4, 16, 1, 10), (2, 1, 8, 2, 12), (3, 2, 33, 1, 9), (4, 2, 16, 2, 10)]
    assert [nc.design_build(c.n, c.m) for c in nc.RELIN] == [(12, 4), (2, 1), (0, 0), (4, 2)]
    for c in nc.RELIN:
        assert nc.design_fuses_fnn(*c.shape, c.H, c.L) and c.envs == (nc.SPLIT_JACOBIAN,) and nc.ic.pick_route(*c.shape) in ("wave", "two")


# ---------------------------------------------------------------------------- the references
@pytest.mark.parametrize("shape", sorted(set(nc.LIN_GAP)) + ["big"], ids=str)
def test_the_float64_restatement_is_held_against_long_double(shape):
    """The gap recorded beside a row of LIN_SHAPES is the measured one (within a factor of two, for another libm) and gives the row its
    tolerance; the vectorised restatement is the models' own jacobian / forward point by point"""
    assert np.finfo(np.longdouble).eps < 1e-18        # (an 80-bit or wider long double)
    cases = [c for c in nc.LIN_BIG] if shape == "big" else [c for c in nc.LIN if (c.net, c.batch) == shape]
    recorded = nc.LIN_BIG_GAP if shape == "big" else nc.LIN_GAP[shape]
    worst = 0.0
    for c in cases:
        ref, ld = nc.lin_reference(c), nc.lin_reference(c, dtype=np.longdouble)
        assert ld[0].dtype == np.longdouble
        worst = max(worst, max(nc.rel(a, b) for a, b in zip(ref, ld)))
        x, u = nc.lin_points(c)
        f = nc.model(c)
        for i in sorted({0, len(x) // 2, len(x) - 1}):
            A, B = f.jacobian(x[i], u[i])
            assert nc.rel(ref[0][i], A) <= 1e-14 and nc.rel(ref[1][i], B) <= 1e-14 and nc.rel(ref[2][i], f.forward(x[i], u[i])) <= 1e-14, (c.id, i)
        assert nc.lin_tol(c) == max(1e-12, 16 * recorded)
        if c.act == "relu" and not c.big:     # the points lie on both sides of the kinks
            a = f.W_in @ np.concatenate([x, u], axis=1).T
            assert (a > 0).any() and (a < 0).any(), c.id
    assert recorded / 2 <= worst <= 2 * recorded, (shape, worst, recorded)


@pytest.mark.parametrize("case", nc.LTV, ids=_ids)
def test_every_ltv_qp_is_strictly_complementary_on_every_instance(case):
    ref = nc.ltv_reference(case)
    assert len(ref) == case.batch                                          # no instance left out
    for i, r in enumerate(ref):
        nact, mult, slack = r["margins"]
        assert nact >= 1 and mult >= nc.MARGIN and slack >= nc.MARGIN, (case.id, i, r["margins"])
    a = nc.ltv_inputs(case)
    P = a["P"] if a["P"].ndim == 2 else a["P"][0]
    assert np.abs(P - np.diag(np.diag(P))).max() > 0                      # a non-diagonal terminal weight


def _margins_ok(case, ref):
    assert len(ref) == case.batch
    for i, r in enumerate(ref):
        assert len(r["margins"]) >= 1
        for nact, mult, slack in r["margins"]:
            assert nact >= 1 and mult >= nc.MARGIN and slack >= nc.MARGIN, (case.id, i, nact, mult, slack)


@pytest.mark.parametrize("case", nc.SQP, ids=_ids)
def test_every_sqp_qp_is_strictly_complementary_on_every_instance(case):
    """... so that the device and the restatement can be compared after several iterations without arguing about active sets; the loop
    makes progress (a first step well above the tolerance of the comparison) and the traced run is mo.sqp_fnn's own"""
    ref = nc.sqp_reference(case)
    _margins_ok(case, ref)
    for r in ref:
        assert len(r["margins"]) == nc.SQP_ITERS and r["hist"][0][0] > 1e-2 and r["hist"][-1][1] < r["hist"][1][1]
    if "chunked" in case.tags:
        _margins_ok(case, nc.sqp_reference(case, True))
        sol = nc.solve_reference(case)
        _margins_ok(case, sol)
        assert all(s["status"] == 0 and 2 <= s["iters"] < nc.SOLVE_ITERS for s in sol)


def test_the_exact_reference_takes_each_kinds_own_stage_hessian():
    """sqp_exact_ref.stage_hessian is its own for an Fnn (net_ref's falls back to it: patched in, it would recurse), net_ref's for a ResNet
    / PolyNet, densenet_ref's for a DenseNet -- and is put back after a reference is made"""
    own = ex.stage_hessian
    assert nc.stage_hessian_of("fnn") is own and nc.stage_hessian_of("densenet") is dr.stage_hessian
    assert nc.stage_hessian_of("resnet") is nc.nr.stage_hessian is nc.stage_hessian_of("polynet")
    for c in nc.EXACT[:4]:
        ref = nc.exact_reference(c)
        assert ex.stage_hessian is own and len(ref) == c.batch
        H, q = ref[0]
        assert np.all(np.isfinite(H)) and np.abs(H - H.T).max() == 0.0
    # the second-order term is there: the exact Hessian differs from the Gauss-Newton one
    c = nc.EXACT[0]
    kw, X0 = nc.nlp_problem(c)
    assert np.linalg.eigvalsh(nc.exact_reference(c)[0][0]).min() > 0


@pytest.mark.parametrize("case", nc.RELIN, ids=_ids)
def test_relin_references_have_active_bounds(case):
    ref = nc.relin_reference(case)
    kw, _ = nc.nlp_problem(case)
    assert sum(int((np.abs(np.abs(r["exact"]["u"]) - case.ub) < 1e-9).sum()) for r in ref["inst"]) >= 3
    assert len({r["A"].tobytes() for r in ref["inst"]}) == case.batch          # every instance its own model
