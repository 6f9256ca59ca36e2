"""CPU checks of the per-instance-weight design's case table (tests/weighted_design_cases.py) and of the new surface.

1  The table's conditions against the exact oracle, one problem per instance with that instance's weights: every instance feasible,
   every condensed Hessian positive definite, at most MAX_ACTIVE rows on a bound, weights as the table says they are drawn; in the
   sensitivity cases no input within (1e-9, 1e-5) of its width from a bound; in the state-row cases every instance feasible with a
   handful of active state rows at the most, and some.
2  The table against the source: every build of k_design_instance_t the launcher can pick, both design routes and both homes of the
   scaling have a case; every reader of the weights on the route takes a stride.
3  The G form of the parameter gradients against the direct form with each instance's own weights: the gap recorded in MEASURED_GAP.
4  The header declares the three symbols, _capi binds them, the Julia shim binds them.
"""
import os
import re

import numpy as np
import pytest

import instance_step_cases as ic
import sens_params_ref as pr
import sens_ref as sr
import weighted_design_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "automationlabsmodelpredictivecontrol.jl_amd", "csrc")
SYMBOLS = ("almpc_design_batched_weighted", "almpc_group_design_batched_weighted", "almpc_get_weights_instance")
_ids = lambda c: c.id


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


# ---------------------------------------------------------------------------- 1. the table's conditions
@pytest.mark.parametrize("case", wc.CASES, ids=_ids)
def test_weights_are_drawn_as_the_table_says(case):
    Q, R, S = wc.weights(case)
    assert Q.shape == (case.batch, case.n, case.n) and R.shape == (case.batch, case.m, case.m)
    assert (S is None) == (not case.with_s)
    for i in range(case.batch):
        dq, dr = np.diag(Q[i]), np.diag(R[i])
        assert np.array_equal(Q[i], Q[i].T) and np.all((dq >= 1.0) & (dq <= 1e3)) and np.all((dr >= 1e-2) & (dr <= 1.0))
        assert np.array_equal(R[i], np.diag(dr))
        assert np.linalg.eigvalsh(Q[i]).min() > 0.5 * dq.min()
        if case.n > 1:
            assert np.abs(Q[i] - np.diag(dq)).max() > 0.0
        if S is not None:
            ds = np.diag(S[i])
            assert np.array_equal(S[i], np.diag(ds)) and np.all((ds >= 1e-2) & (ds <= 1.0))
    # distinct sets: a stride applied to the wrong index or a shared load left in place moves every instance but one
    assert len({Q[i].tobytes() for i in range(case.batch)}) == case.batch
    assert len({R[i].tobytes() for i in range(case.batch)}) == case.batch


@pytest.mark.parametrize("case", wc.CASES, ids=_ids)
def test_every_instance_is_well_posed_with_few_active_rows(case):
    ref = wc.reference(case)
    rows = []
    for i in range(case.batch):
        p = wc.problem(case, i)
        H, F = wc.condensed(case)[i]
        np.linalg.cholesky(0.5 * (H + H.T))                      # positive definite
        u = ref["exact"][i]["u"]
        assert np.isfinite(u).all() and np.all(u >= p.u_min[:, None]) and np.all(u <= p.u_max[:, None])   # feasible (an input box alone)
        rows.append(wc.active_rows(p, u))
        if "sens" in case.tags or "fd" in case.tags:
            g = wc.bound_gaps(p, u)
            assert not ((g > wc.NEAR_BOUND[0]) & (g < wc.NEAR_BOUND[1])).any(), (case.id, i)
    print("weighted-cases %s: active rows %d .. %d (cap %d), %d instances with none" % (case.id, min(rows), max(rows), wc.MAX_ACTIVE, rows.count(0)))
    assert max(rows) <= wc.MAX_ACTIVE, (case.id, rows)
    if case.m * case.N > 1:
        assert max(rows) >= 1, (case.id, "no instance touches a bound: the finish has nothing to do")


@pytest.mark.parametrize("kind", wc.ROWS_CASES)
def test_state_row_cases_are_feasible_with_a_handful_of_active_state_rows(kind):
    ref = wc.rows_reference(kind)          # (raises where an instance is infeasible)
    na = [e["info"]["n_active_state"] for e in ref]
    print("weighted-cases rows %s: active state rows per instance %d .. %d, %d in all" % (kind, min(na), max(na), sum(na)))
    assert len(ref) == wc.ROWS_BATCH and sum(na) > 0
    if kind == "box":
        assert max(na) <= 6, na
    for i, e in enumerate(ref):
        p = wc.rows_problem(kind, i)
        assert np.all(e["u"] >= p.u_min[:, None] - 1e-12) and np.all(e["u"] <= p.u_max[:, None] + 1e-12)


# ---------------------------------------------------------------------------- 2. the table against the source
def test_the_table_reaches_every_build_route_and_home_of_the_scaling():
    got = wc.reached()
    assert got["design"] == set(ic.DESIGN_BUILDS)
    assert got["design_route"] == {"lds", "dense"}
    assert got["scale_in_tail"] == {True, False}
    # ... the switch's split and the natural one (a design LDS below 128 doubles) both
    assert any(not ic.scale_in_tail(*c.shape) for c in wc.CASES if ic.design_route(*c.shape) == "lds")
    assert any(ic.scale_in_tail(*c.shape) and wc.SPLIT_SCALE in c.envs for c in wc.CASES)
    assert {c.with_s for c in wc.CASES} == {True, False}
    # the launcher still picks among exactly these (tests/test_instance_step_cases.py holds the rules themselves against the source)
    api = _read(CSRC, "almpc_api.hip")
    assert api.count("DESIGN_INST(") == 5


def test_every_reader_of_the_weights_on_the_route_takes_a_stride():
    inst, des, dare, vjp, sens = (_read(CSRC, f) for f in ("almpc_instance.hip.h", "almpc_design.hip.h", "almpc_dare.hip.h",
                                                           "almpc_dare_vjp.hip.h", "almpc_sens.hip.h"))
    body = inst[inst.index("void k_design_instance_t(DesignInstParams p) {"):inst.index("// k_design_ltv:")]
    assert not re.search(r"p\.[QRS]\[", body)
    for text in ("p.Q + blockIdx.x * p.sQ", "p.R + blockIdx.x * p.sR", "p.S + blockIdx.x * p.sS"):
        assert text in body, text
    assert "long Q = 0, R = 0, S = 0;" in des[des.index("struct DesignStrides {"):des.index("// ---- K1/K2")]
    assert "Q += blockIdx.y * st.Q;" in des and "p.R += blockIdx.y * p.st.R; p.S += blockIdx.y * p.st.S;" in des
    for src, params in ((dare, "struct DareParams {"), (vjp, "struct DareVjpParams {")):
        assert "long Q_stride = 0, R_stride = 0;" in src[src.index(params):]
        assert not re.search(r"p\.[QR]\[", src)
        assert "p.Q + (size_t)inst * p.Q_stride" in src and "p.R + (size_t)inst * p.R_stride" in src
    body = sens[sens.index("void k_sens_params(SensGradParams p) {"):sens.index("struct SensDxParams {")]
    assert not re.search(r"p\.[QS]\[", body)
    assert "p.Q + (size_t)inst * p.Q_stride" in body and "p.S + (size_t)inst * p.S_stride" in body
    # almpc_sensitivity and almpc_sensitivity_vjp read G, V, d, A, B alone: their operand struct holds no weight
    sp = sens[sens.index("struct SensParams {"):]
    sp = sp[:sp.index("};")]
    assert "const double* G; long G_stride;" in sp and not re.search(r"double\* (Q|R|S|P)\b", sp)


# ---------------------------------------------------------------------------- 3. the parameter gradients' restatement
@pytest.mark.parametrize("case", wc.tagged("sens"), ids=_ids)
def test_g_form_equals_the_direct_form_with_each_instances_own_weights(mo, case):
    ref = wc.reference(case)
    g_u, g_x = wc.loss(case)
    worst = dict.fromkeys(pr.GROUPS, 0.0)
    moved = 0.0
    for i in range(case.batch):
        p = wc.problem(case, i)
        H, F = wc.condensed(case)[i]
        d = mo.jacobi_scaling(H)
        res = ref["exact"][i]
        act, lower = pr.sides(res["u"], p.u_min, p.u_max, d)
        a = pr.params_direct(pr.prob_of(p), H, F, act, lower, res, g_u[i], g_x[i])
        b = pr.params_gform(pr.prob_of(p), sr.g_operands(H, F, d), d, act, lower, res, g_u[i], g_x[i])
        for k, e in pr.worst_gaps(b, a).items():
            worst[k] = max(worst[k], e)
        moved = max(moved, float(np.abs(a["Q"]).max()))
    w = max(worst.values())
    print("weighted-cases %s: gap of the G form to the direct form per group: " % case.id + ", ".join("%s %.1e" % kv for kv in worst.items())
          + "; worst %.3e (recorded %g, tolerance on the device %g)" % (w, wc.MEASURED_GAP[case.id], wc.gpu_tol(case.id)))
    assert moved > 0.0
    assert w <= wc.GAP_SLACK * wc.MEASURED_GAP[case.id]


# ---------------------------------------------------------------------------- 4. the surface
def test_header_capi_and_shim_carry_the_new_symbols(pkg):
    hdr = _read(ROOT, "include", "almpc.h")
    shim = _read(ROOT, "julia", "AlmpcHIP.jl")
    for s in SYMBOLS:
        assert re.search(r"^int %s\(" % s, hdr, re.M), s
        assert "(:%s, libalmpc)" % s in shim, s
        assert s in pkg._capi.prototypes() and s not in pkg._capi._RESTYPES, s   # (declared, and returning int)
    assert "const double* Q_batch /* [batch][n*n] */" in hdr and "const double* S_batch /* [batch][m*m] or NULL */" in hdr
    for cls, names in ((pkg._capi.Solver, ("design_batched_weighted", "get_weights_instance")), (pkg._capi.Group, ("design_batched_weighted",))):
        for nm in names:
            assert callable(getattr(cls, nm, None)), (cls.__name__, nm)
    # what is deliberately not built is said where a caller reads
    i = hdr.index("int almpc_design_batched_weighted(")
    doc = hdr[hdr.rindex("/*", 0, i):i]
    for text in ("ALMPC_FLAG_STRUCTURED", "almpc_set_structured_fallback(h, 1)", "per-instance input boxes", "almpc_design_ltv", "SQP loop",
                 "ALMPC_MAX_ITER"):
        assert text in doc, text
