"""GPU tests of the one record of a design's cost weights (csrc/almpc_api.hip: almpc_handle::Kept, keep_weights, kept_on_device) between
designs and between readers: the other test files design once and call one family of readers, so a record, a device copy or a flag left
over from the design or the reader before would not show there.

Every handle below is designed more than once and read by more than one family (the certificates, the parameter gradients, the
structured-handle sensitivities), each result against its own reference at the handle's OWN returned trajectories:

  certificates          tests/cert_ref.py and tests/cert_ltv_ref.py with the bounds they derive (no measured number)
  parameter gradients   tests/sens_params_ref.params_direct, the metric of tests/test_gpu_sensitivity_params.py
  structured handles    tests/sens_face_rate_ref.py, the metrics of tests/test_gpu_sens_face_rate.py

Tolerances of the last two: the case's own (sens_params_cases.gpu_tol, sens_face_rate_cases.gpu_tol) where the weights are the case's.
For a weight set of this file's own, MEASURED[key] is the worst gap to the reference that one run of the same calls on FRESH handles
(one design, one reader) printed on an MI355X with the library of the commit before the record was introduced; a key is held to it
within GAP_SLACK, by the reasoning of tests/sens_params_cases.py (sums of roundings, the device's own rounded G).  Every check prints
its figure.  k_cert depends on nothing but the instance's data, so certificates of the same step are compared by their bytes.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import cert_ltv_cases as lc
import cert_ltv_ref as lr
import cert_ref as cr
import sens_face_rate_cases as fc
import sens_face_rate_ref as fr
import sens_params_cases as pc
import sens_params_ref as pr
import sens_ref as sr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
CERT4 = ("cost", "res", "grad", "costate")
GAP_SLACK = pc.GAP_SLACK
_dp = ctypes.POINTER(ctypes.c_double)

# worst gap of a weight set of this file's own on fresh handles (see above); the two calls of "4-2-9-S/2S" gave 2.2e-16 (K0), 4.7e-16 (VJP)
MEASURED = {"r326_s/mod": 8.1e-15, "w234": 4.2e-15, "w234/mod": 1.1e-14, "inst326": 6.9e-15, "inst326/weighted": 6.5e-15,
            "4-2-9-S/2S": 4.7e-16}


def params_tol(key):
    return pc.gpu_tol(key) if key in pc.MEASURED_GAP else GAP_SLACK * MEASURED[key]


def face_tol(key):
    return fc.gpu_tol(key) if key in fc.GAP else GAP_SLACK * MEASURED[key]


# ---------------------------------------------------------------------------- weight sets and problems
def modified(p):
    """Q2 = 3 Q + a symmetric off-diagonal term, R2 = R / 4, S2 = 2 S and a P2 of the caller's own"""
    off = np.zeros_like(p.Q); off[0, 1] = off[1, 0] = 0.7 * p.Q[0, 0]
    return dataclasses.replace(p, Q=3.0 * p.Q + off, R=p.R / 4.0, S=2.0 * p.S, P=1.5 * p.P + 0.1 * np.eye(p.n))


def r_dropped(p):
    """... with R2[0, 0] = 0: the branch drops R and S both"""
    R = p.R.copy(); R[0, 0] = 0.0
    return dataclasses.replace(p, R=R)


def w234(mo):
    """m > n: (n, m, N) = (2, 3, 4) with S, batch 5 -- an n*n / m*m mix-up of the offsets in the device copy reads other values"""
    rng = np.random.default_rng(234)
    A = rng.standard_normal((2, 2)); A *= 0.9 / np.max(np.abs(np.linalg.eigvals(A)))
    p = mo.make_problem(A, rng.standard_normal((2, 3)), 4, [-0.5, -0.8, -0.3], [0.6, 0.4, 0.9], x_ref=0.2 * rng.standard_normal(2),
                        u_ref=np.array([0.1, -0.1, 0.05]), q=10.0, r=1.0, s=0.5)
    return p, np.array([0.3, 1.0, 2.0, 4.0, 8.0])[:, None] * rng.standard_normal((5, 2))


def inst326(mo):
    """one (3, 2, 6) model per instance, batch 5, with S; [1]: the same with a weight set per instance"""
    rng = np.random.default_rng(326)
    base, _ = pc.r326(mo, 0.5)
    shared, own = [], []
    for _ in range(5):
        A = rng.standard_normal((3, 3)); A *= (0.7 + 0.3 * rng.random()) / np.max(np.abs(np.linalg.eigvals(A)))
        B = rng.standard_normal((3, 2))
        Q, R, S = base.Q * (0.5 + rng.random()) + 0.1 * np.diag(rng.random(3)), base.R * (0.5 + rng.random()), base.S * (0.5 + rng.random())
        shared.append(dataclasses.replace(base, A=A, B=B, P=mo.dare(A, B, base.Q, base.R)))
        own.append(dataclasses.replace(base, A=A, B=B, Q=Q, R=R, S=S, P=mo.dare(A, B, Q, R)))
    return shared, own, np.array([0.3, 1.0, 2.0, 3.0, 5.0])[:, None] * rng.standard_normal((5, 3))


def loss(seed, b, p):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(b, p.m, p.N)), rng.normal(size=(b, p.n, p.N + 1))


# ---------------------------------------------------------------------------- designs, steps and the checks
def design_shared(sv, p):
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, p.P, p.u_min, p.u_max)
    sv.set_reference(p.x_ref, p.u_ref)


def design_instances(sv, ps, weighted):
    A, B, P = (np.stack([getattr(p, k) for p in ps]) for k in ("A", "B", "P"))
    p = ps[0]
    if weighted:
        sv.design_batched_weighted(A, B, *(np.stack([getattr(q, k) for q in ps]) for k in ("Q", "R", "S")), P, p.u_min, p.u_max)
    else:
        sv.design_batched(A, B, p.Q, p.R, p.S, P, p.u_min, p.u_max)
    sv.set_reference(p.x_ref, p.u_ref)


def step(sv, X0):
    sv.update_initialization(X0)
    sv.calculate()


def check_certificate(tag, cert, res, ps, Ps=None, **branch):
    """every value of a k_cert certificate within cert_ref's bound at the step's own trajectories"""
    worst = 0.0
    for i, p in enumerate(ps):
        k = cr.certificate(p.A, p.B, p.Q, p.R, p.S, p.P if Ps is None else Ps[i], p.u_min, p.u_max, res["e_x"][i], res["e_u"][i], res["u"][i],
                           **branch)
        for key in CERT4:
            err = np.abs(np.asarray(cert[key][i]) - k[key])
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.max(np.where(err == 0.0, 0.0, err / k["tol_" + key]))))
            assert np.all(err <= k["tol_" + key]), (tag, i, key)
    print(f"{tag}: certificate, worst error / bound {worst:.3f}")


def same_certificate(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in CERT4)


def check_params(tag, key, sv, ps, g_u, g_x, shared):
    """every group of almpc_sensitivity_params_vjp of every instance against the direct form"""
    res, got = sv.get_results(), sv.sensitivity_params_vjp(g_u, g_x)
    assert np.all(res["status"] == 0), (tag, res["status"])
    g = sv.get_design() if shared else None
    worst = 0.0
    for i, p in enumerate(ps):
        H, F, d = (g[k] for k in ("H", "F", "d")) if shared else (sv.get_design_instance(i)[k] for k in ("H", "F", "d"))
        r = {k: res[k][i] for k in ("u", "e_u", "e_x")}
        act, lower = pr.sides(r["u"], p.u_min, p.u_max, d)
        assert got["rows"][i] == act.sum(), (tag, i)
        ref = pr.params_direct(pr.prob_of(p), H, F, act, lower, r, g_u[i], g_x[i])
        worst = max(worst, max(pr.worst_gaps({k: got[k][i] for k in pr.GROUPS}, ref).values()))
    tol = params_tol(key)
    print(f"{tag}: parameter gradients [{key}], worst gap {worst:.2e} (tolerance {tol:g})")
    assert worst <= tol, (tag, key, worst)
    return got


def check_face(tag, key, sv, p, what, g_u, g_x):
    """K0 of almpc_sensitivity_stagewise_rate ("K0") or almpc_sensitivity_stagewise_rate_vjp ("vjp") against sens_face_rate_ref"""
    res = sv.get_results()
    assert np.all(res["status"] == 0), (tag, res["status"])
    out = sv.sensitivity_stagewise_rate(("K0",)) if what == "K0" else sv.sensitivity_stagewise_rate_vjp(g_u, g_x)
    worst = 0.0
    for i in range(res["u"].shape[0]):
        act = fr.active_rows(res["u"][i], p.u_min, p.u_max)
        if what == "K0":
            J, _ = fr.jacobians(p.A, p.B, p.Q, p.R, p.S, p.P, act, p.N)
            assert out["rows"][i] == act.sum(), (tag, i)
            worst = max(worst, np.abs(out["K0"][i] - sr.shaped(J, p.m, p.N)[0]).max() / max(1.0, np.abs(J).max()))
        else:
            ref = fr.vjp(p.A, p.B, p.Q, p.R, p.S, p.P, act, g_u[i], g_x[i])
            assert out[1][i] == act.sum(), (tag, i)
            worst = max(worst, np.abs(out[0][i] - ref).max() / sr.vjp_scale(ref))
    tol = face_tol(key)
    print(f"{tag}: {what} on the face [{key}], worst error / scale {worst:.2e} (tolerance {tol:g})")
    assert worst <= tol, (tag, key, worst)


def _code(capi, call):
    with pytest.raises(capi.AlmpcError) as e:
        call()
    return e.value.code


# ---------------------------------------------------------------------------- 1. condensed shared handle
def fresh_certificate(capi, p, X0):
    sv = capi.Solver(p.n, p.m, p.N, len(X0))
    design_shared(sv, p); step(sv, X0)
    cert = sv.certificate()
    sv.close()
    return cert


@pytest.mark.parametrize("name", ["r326_s", "w234"])
def test_condensed_shared_readers_interleaved_then_redesigned(capi, mo, name):
    p, X0 = pc.case(mo, "r326_s") if name == "r326_s" else w234(mo)
    X0 = X0[:5]
    b = len(X0)
    g_u, g_x = loss(11, b, p)
    sv = capi.Solver(p.n, p.m, p.N, b)
    # design, step, certificate, every group of the parameter gradients, certificate
    design_shared(sv, p); step(sv, X0)
    c0 = sv.certificate()
    check_certificate(name, c0, sv.get_results(), [p] * b)
    got = check_params(name, name, sv, [p] * b, g_u, g_x, True)
    assert np.abs(got["S"]).max() > 0 and np.abs(got["R"]).max() > 0 and np.abs(got["P"]).max() > 0
    c1 = sv.certificate()
    assert same_certificate(c0, c1) and same_certificate(c0, fresh_certificate(capi, p, X0))
    # other weights on the same handle, the readers in the other order
    p2 = modified(p)
    design_shared(sv, p2); step(sv, X0)
    check_params(name + " redesigned", name + "/mod", sv, [p2] * b, g_u, g_x, True)
    c2 = sv.certificate()
    check_certificate(name + " redesigned", c2, sv.get_results(), [p2] * b)
    assert same_certificate(c2, sv.certificate()) and same_certificate(c2, fresh_certificate(capi, p2, X0))
    assert not same_certificate(c0, c2)
    # R[1,1] = 0: R and S both drop out
    p3 = r_dropped(p2)
    design_shared(sv, p3); step(sv, X0)
    c3 = sv.certificate()
    check_certificate(name + " R dropped", c3, sv.get_results(), [p3] * b, useR=False, useS=False)
    assert same_certificate(c3, fresh_certificate(capi, p3, X0))
    assert _code(capi, lambda: sv.sensitivity_params_vjp(g_u, g_x, terminal="dare")) == ERR_UNSUPPORTED
    sv.close()


# ---------------------------------------------------------------------------- 2. per-instance and weighted designs on one handle
def test_per_instance_then_weighted_then_per_instance(capi, mo):
    shared, own, X0 = inst326(mo)
    b = len(X0)
    g_u, g_x = loss(13, b, shared[0])
    sv = capi.Solver(3, 2, 6, b)
    certs = []
    for tag, ps, weighted in (("per instance", shared, False), ("weighted", own, True), ("per instance again", shared, False)):
        design_instances(sv, ps, weighted); step(sv, X0)
        certs.append(sv.certificate())
        check_certificate(tag, certs[-1], sv.get_results(), ps)
        check_params(tag, "inst326/weighted" if weighted else "inst326", sv, ps, g_u, g_x, False)
        assert same_certificate(certs[-1], sv.certificate())
    assert same_certificate(certs[0], certs[2]) and not same_certificate(certs[0], certs[1])
    sv.close()


# ---------------------------------------------------------------------------- 3. structured handle
def test_structured_handle_readers_interleaved_then_redesigned(capi):
    name = "4-2-9-S"
    p, X0, shared = fc.case(name)
    assert shared and p.S[0, 0] != 0.0
    g_u, g_x = fc.loss(name)
    sv = capi.Solver(p.n, p.m, p.N, len(X0), structured=True)
    design_shared(sv, p); step(sv, X0)
    check_face(name, name, sv, p, "K0", g_u, g_x)
    c0 = sv.certificate()
    check_certificate(name, c0, sv.get_results(), [p] * len(X0))
    check_face(name, name, sv, p, "vjp", g_u, g_x)
    assert same_certificate(c0, sv.certificate())
    p2 = dataclasses.replace(p, S=2.0 * p.S)
    design_shared(sv, p2); step(sv, X0)
    check_face(name + " 2 S", name + "/2S", sv, p2, "vjp", g_u, g_x)
    c2 = sv.certificate()
    check_certificate(name + " 2 S", c2, sv.get_results(), [p2] * len(X0))
    check_face(name + " 2 S", name + "/2S", sv, p2, "K0", g_u, g_x)
    assert same_certificate(c2, sv.certificate()) and not same_certificate(c0, c2)
    sv.close()


# ---------------------------------------------------------------------------- 4. the re-linearisation pipeline around a plain design
@pytest.mark.parametrize("structured", [False, True], ids=["condensed", "structured"])
def test_relin_pipeline_then_a_design_then_the_pipeline(capi, mo, structured):
    """The certificates against cert_ref on the step's own models and terminal weights, read back from the handle.  (The plain design
    in the middle also holds almpc_design_shared on a structured handle to dropping a pipeline set up there, as the condensed one does.)"""
    f = mo.synthetic_fnn()
    n, m, N, b = 4, 2, 10, 4
    x_ref, u_ref = np.zeros((n, N + 1)), np.zeros((m, N))
    Q, R, S = 100.0 * np.eye(n), 0.1 * np.eye(m), np.array([[0.3, 0.05], [0.05, 0.2]])
    Al, Bl = capi.fnn_linearize(f.W_in, f.W_h, f.b_h, f.W_out, x_ref[:, -1][None], u_ref[:, -1][None], act=f.act)
    umin, umax = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    x0 = 0.05 * np.random.default_rng(2).normal(size=(b, n))
    sv = capi.Solver(n, m, N, b, structured=structured)

    def pipeline(tag, Qs):
        sv.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Qs, R, S, capi.dare(Al[0], Bl[0], Qs, R), umin, umax, act=f.act)
        sv.update_initialization(x0)
        sv.relin_fnn_step()
        res, cert = sv.get_results(), sv.relin_fnn_certificate()
        models = [sv.model_instance(i) for i in range(b)]
        ps = [mo.MPCProblem(A=np.array(A), B=np.array(B), N=N, Q=Qs, R=R, S=S, P=np.array(sv.terminal_weight_instance(i)), x_ref=x_ref,
                            u_ref=u_ref, u_min=umin, u_max=umax) for i, (A, B) in enumerate(models)]
        check_certificate(tag, cert, res, ps)
        return cert

    c0 = pipeline("pipeline", Q)
    rng = np.random.default_rng(42)
    A = rng.standard_normal((n, n)); A *= 0.9 / np.max(np.abs(np.linalg.eigvals(A)))
    p = mo.make_problem(A, rng.standard_normal((n, m)), N, [-0.5, -0.7], [0.6, 0.4], x_ref=0.1 * rng.standard_normal(n), q=5.0, r=2.0, s=0.7)
    X0 = 2.0 * rng.standard_normal((b, n))
    design_shared(sv, p); step(sv, X0)
    c1 = sv.certificate()
    check_certificate("plain design between", c1, sv.get_results(), [p] * b)
    fresh = capi.Solver(n, m, N, b, structured=structured)
    design_shared(fresh, p); step(fresh, X0)
    assert same_certificate(c1, fresh.certificate())
    fresh.close()
    c2 = pipeline("pipeline, 3 Q", 3.0 * Q)
    assert not same_certificate(c0, c2)
    sv.close()


# ---------------------------------------------------------------------------- 5. one mask for both forms' buffers
def test_the_other_forms_getters_are_refused(capi, mo):
    name = "2-1-N2-b4"
    a = lc.inputs(name)
    n, m, N = lc.shape(name)
    sv = capi.Solver(n, m, N, 4)
    buf = np.empty(4 * n * (N + 1))
    plain = lambda: sv.L.almpc_get_certificate(sv.h, buf.ctypes.data_as(_dp), None, None, None)
    ltv = lambda: sv.L.almpc_get_certificate_ltv(sv.h, buf.ctypes.data_as(_dp), None, None, None, None, None)
    sv.design_ltv(a["A_all"], a["B_all"], a["c_all"], a["xbar"], a["ubar"], a["x_ref"], a["u_ref"], a["Q"], a["R"], a["S"], a["P"], a["umin"],
                  a["umax"], keep_stage_models=True)
    step(sv, a["xbar"][:, :, 0])
    cert = sv.certificate_ltv()
    res = sv.get_results(want=("u", "e_u"))
    for i in range(4):
        k, _ = lc.instance(name, i)
        ref = lr.certificate_ltv(k["A"], k["B"], k["c"], k["xbar"], k["xref"], k["uref"], k["Q"], k["R"], k["S"], k["P"], k["umin"], k["umax"],
                                 res["e_u"][i], res["u"][i])
        for key in CERT4 + ("x", "e_x"):
            assert np.all(np.abs(np.asarray(cert[key][i]) - ref[key]) <= ref["tol_" + key]), (i, key)
    assert ltv() == 0 and plain() == ERR_INVALID
    assert _code(capi, sv.device_certificate) == ERR_INVALID and sv.device_certificate_ltv()["x"]
    rng = np.random.default_rng(5)
    p = mo.make_problem(np.array([[0.9, 0.2], [0.0, 0.8]]), rng.standard_normal((n, m)), N, [-0.5], [0.5], s=0.5)
    design_shared(sv, p)
    assert ltv() == ERR_INVALID and plain() == ERR_INVALID   # a new design: nothing of either form
    step(sv, rng.standard_normal((4, n)))
    c = sv.certificate()
    check_certificate("plain design behind the time-varying one", c, sv.get_results(), [p] * 4)
    assert plain() == 0 and ltv() == ERR_INVALID
    assert _code(capi, sv.device_certificate_ltv) == ERR_INVALID and sv.device_certificate()["cost"]
    sv.calculate()   # a new step voids both
    assert plain() == ERR_INVALID and ltv() == ERR_INVALID
    sv.close()
