"""GPU tests of k_sens_ltv (csrc/almpc_sens_ltv.hip.h): almpc_sensitivity_ltv and almpc_sensitivity_ltv_vjp on almpc_design_ltv designs
made with the keep switch on.

Reference per instance: tests/sens_ltv_ref.py (the Riccati recursion on the face with the stage models, numpy FP64) evaluated at the
handle's OWN returned u under the contract's active-set rule, so both sides differentiate the same face.  Tolerance per case:
max(10 GAP, 1e-13) with the gap of that restatement to the direct form on the CPU (sens_ltv_cases.GAP,
tests/test_sens_ltv_restatement.py), of max(1, max|J_i|) for K0, dU, dX and of sens_ref.vjp_scale for the VJP; it is not tuned against
the device.  Every case prints its worst figure beside its tolerance.  Independent of the recursion's restatement: the per-instance
time-invariant twins against k_sens_face / k_sens_face_rate on a structured handle, and central differences of the device's own
solution in the initial deviation (dx_0 = p is the same QP as c_0 <- c_0 + A_0 p)."""
import ctypes
import functools

import numpy as np
import pytest

import sens_ltv_cases as tc
import sens_ltv_ref as tr
import sens_ref as sr
from sens_face_gpu import flat, same

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_NOT_DESIGNED = -1, -4, -5
JAC = ("K0", "dU", "dX")
_dp = ctypes.POINTER(ctypes.c_double)


def design_args(a):
    return (a["A_all"], a["B_all"], a["c_all"], a["xbar"], a["ubar"], a["x_ref"], a["u_ref"], a["Q"], a["R"], a["S"], a["P"], a["umin"], a["umax"])


def step(capi, a, opts=None, keep=True, s=None, **kw):
    """a handle designed on design_ltv's arguments `a` (the keep switch on), one step taken"""
    b, N, n, m = a["B_all"].shape
    s = s or capi.Solver(n, m, N, b)
    s.design_ltv(*design_args(a), keep_stage_models=keep, **kw)
    s.update_initialization(a["xbar"][:, :, 0])
    s.calculate(opts)
    return s


def sensitivities(s, name):
    """every sensitivity call of a stepped handle: dict(res, sens, g_u, g_x, g_x0, vrows, null, zeros)"""
    res = s.get_results(want=("u", "status"))
    sens = s.sensitivity_ltv()
    g_u, g_x = tc.loss(name)
    g_x0, vrows = s.sensitivity_ltv_vjp(g_u, g_x)
    a0 = s.sensitivity_ltv_vjp(g_u, None)
    a1 = s.sensitivity_ltv_vjp(g_u, np.zeros_like(g_x))
    return dict(res=res, sens=sens, g_u=g_u, g_x=g_x, g_x0=g_x0, vrows=vrows, null=a0, zeros=a1)


@functools.lru_cache(maxsize=None)
def device(capi, name):
    """One step of a case and every sensitivity call on it, shared by the tests below (read-only)."""
    s = step(capi, tc.inputs(name))
    d = sensitivities(s, name)
    s.close()
    return d


def check_jacobians(name, d, which):
    """K0, dU, dX, rows of the instances `which` against the restatement on the returned u; returns (worst error / scale, rows)"""
    n, m, N = tc.shape(name)
    a = tc.inputs(name)
    res, sens, tol = d["res"], d["sens"], tc.gpu_tol(name)
    worst, rows = 0.0, []
    for i in which:
        k, _ = tc.instance(name, i)
        u = res["u"][i]
        band = tc.in_band(u, a["umin"], a["umax"])
        assert not band.size, (name, i, band)
        act = tr.active_rows(u, a["umin"], a["umax"])
        rows.append(int(act.sum()))
        assert sens["rows"][i] == act.sum(), (name, i, sens["rows"][i], act.sum())
        J, dX = tr.jacobians(act=act, **k)
        K0, dU = sr.shaped(J, m, N)
        sj, sx = max(1.0, np.abs(J).max()), max(1.0, np.abs(dX).max())
        roll = tr.rollout(k["A"], k["B"], flat(sens["dU"][i]))
        for got, ref, scale in ((sens["K0"][i], K0, sj), (sens["dU"][i], dU, sj), (sens["dX"][i], dX, sx), (sens["dX"][i], roll, sx)):
            err = np.abs(got - ref).max() / scale
            worst = max(worst, err)
            assert err <= tol, (name, i, err, tol)
        assert same(sens["K0"][i], sens["dU"][i][:, 0, :]), (name, i)
        assert np.array_equal(sens["dX"][i][:, 0, :], np.eye(n)), (name, i)
    return worst, rows


def check_vjp(name, d, which):
    tol = tc.gpu_tol(name)
    worst = 0.0
    for i in which:
        k, _ = tc.instance(name, i)
        a = tc.inputs(name)
        act = tr.active_rows(d["res"]["u"][i], a["umin"], a["umax"])
        ref = tr.vjp(act=act, g_u=d["g_u"][i], g_x=d["g_x"][i], **k)
        own = sr.vjp_from_jacobians(d["sens"]["dU"][i], d["sens"]["dX"][i], d["g_u"][i], d["g_x"][i])
        scale = sr.vjp_scale(ref)
        for other in (ref, own):
            err = np.abs(d["g_x0"][i] - other).max() / scale
            worst = max(worst, err)
            assert err <= tol, (name, i, err, tol)
    return worst


@pytest.mark.parametrize("name", tc.ALL_NAMES)
def test_jacobians_of_every_case(capi, name):
    n, m, N = tc.shape(name)
    d = device(capi, name)
    assert np.all(d["res"]["status"] == 0), d["res"]["status"]
    assert d["sens"]["K0"].shape == (4, m, n) and d["sens"]["dU"].shape == (4, m, N, n) and d["sens"]["dX"].shape == (4, n, N + 1, n)
    worst, rows = check_jacobians(name, d, tc.instances(name))
    print(f"{name}: rows {min(rows)} .. {max(rows)} of {m * N}, worst error / scale {worst:.3e} (tolerance {tc.gpu_tol(name):g})")


@pytest.mark.parametrize("name", tc.ALL_NAMES)
def test_vjp_of_every_case(capi, name):
    d = device(capi, name)
    assert np.array_equal(d["vrows"], d["sens"]["rows"])
    worst = check_vjp(name, d, tc.instances(name))
    print(f"{name}: VJP worst error / scale {worst:.3e} (tolerance {tc.gpu_tol(name):g})")
    (a0, r0), (a1, r1) = d["null"], d["zeros"]
    assert a0.tobytes() == a1.tobytes() and np.array_equal(r0, r1)
    assert np.abs(a0).max() > 0 or np.all(d["sens"]["rows"] == d["res"]["u"][0].size)


@functools.lru_cache(maxsize=None)
def structured(capi, name):
    """The structured twin of a "ti-" case: almpc_design_batched on a structured handle, a step, almpc_sensitivity_stagewise_rate and its
    VJP with the case's loss (read-only)."""
    n, m, N = tc.shape(name)
    t = tc.structured_twin(name)
    g_u, g_x = tc.loss(name)
    s = capi.Solver(n, m, N, tc.BATCH, structured=True)
    s.design_batched(t["A"], t["B"], t["Q"], t["R"], t["S"], t["P"], t["umin"], t["umax"])
    s.update_initialization(t["X0"])
    s.calculate()
    res = s.get_results(want=("u", "status"))
    sens = s.sensitivity_stagewise_rate()
    g_x0, vrows = s.sensitivity_stagewise_rate_vjp(g_u, g_x)
    s.close()
    return dict(res=res, sens=sens, g_x0=g_x0, vrows=vrows)


@pytest.mark.parametrize("name", tc.TI_NAMES)
def test_time_invariant_design_equals_the_structured_handle(capi, name):
    """A_k = A_i, B_k = B_i, xbar = x0 repeated with its defects, ubar = 0 against almpc_design_batched on a structured handle and
    almpc_sensitivity_stagewise_rate (k_sens_face without S, k_sens_face_rate with it): nothing shared but the data.  The structured
    twin is no case of sens_face_cases and has no recorded tolerance of its own; with time-invariant stages the two restatements are the
    same operations (tests/test_sens_ltv_restatement.py holds them to equal bits), so its tolerance by that table's rule, max(10 GAP,
    1e-13), is the twin case's, and the sum of the two is 2 gpu_tol(name)."""
    d, t = device(capi, name), structured(capi, name)
    res, sens, g_x0, vrows = t["res"], t["sens"], t["g_x0"], t["vrows"]
    assert np.all(res["status"] == 0)
    a = tc.inputs(name)
    for i in range(tc.BATCH):   # the premise: the same face
        assert np.array_equal(tr.active_rows(res["u"][i], a["umin"], a["umax"]), tr.active_rows(d["res"]["u"][i], a["umin"], a["umax"])), i
    assert np.array_equal(sens["rows"], d["sens"]["rows"]) and np.array_equal(vrows, d["vrows"])
    tol = 2.0 * tc.gpu_tol(name)
    worst = 0.0
    for i in range(tc.BATCH):
        sj, sx = max(1.0, np.abs(sens["dU"][i]).max()), max(1.0, np.abs(sens["dX"][i]).max())
        for k, scale in (("K0", sj), ("dU", sj), ("dX", sx)):
            worst = max(worst, np.abs(sens[k][i] - d["sens"][k][i]).max() / scale)
        worst = max(worst, np.abs(g_x0[i] - d["g_x0"][i]).max() / sr.vjp_scale(g_x0[i]))
    print(f"{name}: k_sens_ltv against the structured handle's kernel: worst difference / scale {worst:.3e} (tolerance {tol:g})")
    assert worst <= tol
    assert np.any(sens["K0"] != 0.0)


@pytest.mark.parametrize("name", tc.TI_NAMES)
def test_time_invariant_design_has_the_bits_of_the_structured_handle(capi, name):
    """k_sens_ltv mirrors the stage bodies of k_sens_face / k_sens_face_rate entry for entry, in their order of summation, and the gains
    depend on the returned u through the face alone: on the same face and the same (A_i, B_i) in every stage the two kernels give the
    same bits in K0, dU, dX and the VJP.  A guard against the copies drifting apart."""
    d, t = device(capi, name), structured(capi, name)
    assert np.array_equal(t["sens"]["rows"], d["sens"]["rows"])   # (the premise, held by the test above)
    for k in JAC:
        assert same(t["sens"][k], d["sens"][k]), (name, k)
    assert same(t["g_x0"], d["g_x0"]), name


@pytest.mark.parametrize("name", ("4-3-N7-b4", "12-4-N3-b4"))
def test_finite_differences_of_the_device_solution(capi, name):
    """dx_0 = p is the same QP as c_0 <- c_0 + A_0 p: the design again with c_0 +- FD_H A_0 e_j, (u+ - u-) / 2 FD_H against column j of dU.
    (tests/test_sens_ltv_restatement.py: the oracle's active set of these instances is the same at +-FD_H.)"""
    n, m, N = tc.shape(name)
    a = tc.inputs(name)
    d = device(capi, name)
    dU = d["sens"]["dU"]
    fd = np.zeros_like(dU)
    s = None
    for j in range(n):
        u = []
        for sgn in (1.0, -1.0):
            c = a["c_all"].copy()
            c[:, 0, :] += sgn * tc.FD_H * a["A_all"][:, 0, :, j]
            s = step(capi, dict(a, c_all=c), s=s)
            r = s.get_results(want=("u", "status"))
            assert np.all(r["status"] == 0)
            u.append(r["u"])
        fd[:, :, :, j] = (u[0] - u[1]) / (2.0 * tc.FD_H)
    s.close()
    err = max(np.abs(dU[i] - fd[i]).max() / max(1.0, np.abs(dU[i]).max()) for i in range(tc.BATCH))
    print(f"{name}: dU against central differences of the device's own u: {err:.3e} (tolerance {tc.FD_TOL:g})")
    assert err <= tc.FD_TOL
    assert np.any(dU != 0.0)


def test_unsolved_instances_get_minus_one_and_zeros(capi):
    """The options of tests/test_gpu_cert_ltv.py::test_unsolved_inputs_are_certified_as_they_are (no polish, two ADMM iterations: the
    step refuses max_iter = 0 as an option) leave instances unsolved: rows = -1 and zeros in every output; a solved instance beside
    them is held to the case's tolerance as ever."""
    name = "7-2-N64-b4"
    s = step(capi, tc.inputs(name), capi.default_opts(polish=0, max_iter=2))
    d = sensitivities(s, name)
    k0 = s.sensitivity_ltv(("K0",))
    s.close()
    status, sens = d["res"]["status"], d["sens"]
    bad, good = np.nonzero(status != 0)[0], np.nonzero(status == 0)[0]
    print(f"{bad.size} unsolved of {status.size}")
    assert bad.size >= 1, status
    for i in bad:
        assert sens["rows"][i] == -1 and d["vrows"][i] == -1 and k0["rows"][i] == -1
        assert not sens["K0"][i].any() and not sens["dU"][i].any() and not sens["dX"][i].any() and not d["g_x0"][i].any() and not k0["K0"][i].any()
    if good.size:
        check_jacobians(name, d, good)
        check_vjp(name, d, good)


def _code(capi, call):
    with pytest.raises(capi.AlmpcError) as e:
        call()
    return e.value.code


def test_contract(capi, mo):
    message = lambda s: (s.L.almpc_last_error(s.h) or b"").decode().strip()
    name = "4-2-N3-b4"
    a = tc.inputs(name)
    n, m, N = tc.shape(name)
    g_u, g_x = tc.loss(name)
    gu, gx0 = np.zeros((4, N, m)), np.zeros((4, n))
    ptr = lambda x: x.ctypes.data_as(_dp)
    calls = lambda s: (lambda: s.sensitivity_ltv(("K0",)), lambda: s.sensitivity_ltv_vjp(g_u))
    sv = capi.Solver(n, m, N, 4)
    for call in calls(sv):
        assert _code(capi, call) == ERR_NOT_DESIGNED and message(sv)
    sv.design_ltv(*design_args(a), keep_stage_models=True)
    for call in calls(sv):
        assert _code(capi, call) == ERR_INVALID and message(sv)   # before the design's first step
    sv.update_initialization(a["xbar"][:, :, 0]); sv.calculate()
    # a want that is no mask, NULL pointers
    assert sv.L.almpc_sensitivity_ltv(sv.h, 0, 0.0) == ERR_INVALID and "ALMPC_SENS_" in message(sv)
    assert sv.L.almpc_sensitivity_ltv(sv.h, 8, 0.0) == ERR_INVALID
    assert sv.L.almpc_sensitivity_ltv_vjp(sv.h, None, None, 0.0, ptr(gx0), None) == ERR_INVALID and "null" in message(sv)
    assert sv.L.almpc_sensitivity_ltv_vjp(sv.h, ptr(gu), None, 0.0, None, None) == ERR_INVALID
    assert sv.L.almpc_get_sensitivity(sv.h, None, None, None, None) == ERR_INVALID   # nothing computed yet
    # the existing calls keep refusing the design, and name the new one
    for call in (lambda: sv.sensitivity(("K0",)), lambda: sv.sensitivity_vjp(g_u), lambda: sv.sensitivity_rows(("K0",)),
                 lambda: sv.sensitivity_stagewise(("K0",)), lambda: sv.sensitivity_stagewise_rate_vjp(g_u)):
        assert _code(capi, call) == ERR_UNSUPPORTED and "almpc_sensitivity_ltv" in message(sv)
    # results survive until the next step (other calls in between), and the getters refuse after it
    before = sv.get_results()
    sens = sv.sensitivity_ltv()
    sv.sensitivity_ltv_vjp(g_u, g_x)
    sv.certificate_ltv()
    got = capi._sens_read(sv.L.almpc_get_sensitivity, sv.h, sv._check, JAC, 4, n, m, N)
    for k in JAC + ("rows",):
        assert same(got[k], sens[k]), k
    k0_only = sv.sensitivity_ltv(("K0",))
    assert same(k0_only["K0"], sens["K0"])
    assert sv.L.almpc_get_sensitivity(sv.h, None, ptr(np.empty(sens["dU"].size)), None, None) == ERR_INVALID   # (K0 alone was asked for)
    views = sv.device_sensitivity()
    assert views["K0"] and not views["dU"] and not views["dX"]
    after = sv.get_results()
    for k in ("x", "e_x", "u", "e_u", "status"):
        assert before[k].tobytes() == after[k].tobytes(), k
    sv.calculate()
    assert sv.L.almpc_get_sensitivity(sv.h, ptr(np.empty(sens["K0"].size)), None, None, None) == ERR_INVALID
    assert _code(capi, sv.device_sensitivity) == ERR_INVALID
    again = sv.sensitivity_ltv()
    for k in JAC + ("rows",):
        assert same(again[k], sens[k]), k   # (the same step again: the same bytes)
    # the keep switch off: the design released its stage models, and the message names the switch
    step(capi, a, keep=False, s=sv)
    for call in calls(sv):
        assert _code(capi, call) == ERR_INVALID and "almpc_set_keep_stage_models" in message(sv)
    step(capi, a, keep=True, s=sv)
    again = sv.sensitivity_ltv()
    for k in JAC + ("rows",):
        assert same(again[k], sens[k]), k
    sv.close()
    # a state box, the terminal equality
    for kw in (dict(xmin=[-50.0] * n, xmax=[50.0] * n), dict(terminal="equality")):
        sv = step(capi, a, **kw)
        for call in calls(sv):
            assert _code(capi, call) == ERR_UNSUPPORTED and "state rows" in message(sv)
        sv.close()
    # designs that are not almpc_design_ltv's: the message names the call that serves them
    p = mo.double_integrator(N=N)
    X0 = 0.5 * np.random.default_rng(1).normal(size=(4, 2))
    for structured, serves in ((False, "almpc_sensitivity"), (True, "almpc_sensitivity_stagewise_rate")):
        sv = capi.Solver(2, 1, N, 4, structured=structured)
        sv.set_keep_stage_models(True)
        sv.design_shared(p.A, p.B, p.Q, p.R, None, None, p.u_min, p.u_max)
        sv.update_initialization(X0); sv.calculate()
        for call in (lambda: sv.sensitivity_ltv(("K0",)), lambda: sv.sensitivity_ltv_vjp(np.zeros((4, 1, N)))):
            assert _code(capi, call) == ERR_UNSUPPORTED and serves in message(sv) and "almpc_design_ltv" in message(sv)
        sv.close()
    # the SQP loop and the re-linearisation pipeline of a black-box model stay refused
    f = mo.synthetic_fnn()
    n, m, N = 4, 2, 10
    x_ref, u_ref = np.zeros((n, N + 1)), np.zeros((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    Al, Bl = capi.fnn_linearize(f.W_in, f.W_h, f.b_h, f.W_out, x_ref[:, -1][None], u_ref[:, -1][None], act=f.act)
    P = capi.dare(Al[0], Bl[0], Q, R)
    x0 = 0.05 * np.random.default_rng(2).normal(size=(4, n))
    sv = capi.Solver(n, m, N, 4)
    sv.set_keep_stage_models(True)
    sv.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act)
    sv.sqp_fnn_start(x0)
    sv.sqp_fnn_iterate(1)
    assert _code(capi, lambda: sv.sensitivity_ltv(("K0",))) == ERR_UNSUPPORTED and "SQP" in message(sv)
    sv.close()
    sv = capi.Solver(n, m, N, 4)
    sv.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act)
    sv.update_initialization(x0)
    sv.relin_fnn_step()
    assert _code(capi, lambda: sv.sensitivity_ltv(("K0",))) == ERR_UNSUPPORTED and message(sv)
    sv.close()

