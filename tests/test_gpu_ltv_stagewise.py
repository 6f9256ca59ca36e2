"""GPU tests of almpc_design_ltv_stagewise / almpc_ltv_stagewise_update (k_ltv_stage_prepare, k_ltv_stage_finish around k_riccati_t and
k_sgains + k_sdual): every case of tests/ltv_stagewise_cases.py in the host form and the device form against the stage-wise oracle, the
prepared vectors against tests/ltv_stage_ref.py, the update path, a caller's multiple-shooting loop, the certificate and sensitivities
of such a design, and the refusals.

Device arrays are float64 device memory of the handle's device, allocated and filled through the HIP runtime the library itself is
linked against (ctypes on the libamdhip64 mapped into this process, as tests/test_gpu_cert_ltv.py reads its device views).  They are
NOT torch tensors: the torch wheel brings a HIP / HSA runtime of its own, and loaded into one process with the library's each of the
two sees no device (tests/test_gpu_nlp_shapes.py::_num_cus asks torch in a child process for the same reason), so a tensor's
data_ptr() cannot be produced in the process that holds the handle.  To the entry points the two are the same thing: an address of
complete float64 data in the C layout on the handle's device.

Tolerances: U_TOL = 1e-5 on e_u is the project's parity tolerance; e_x gets U_TOL max(1, ||Gamma||_inf) (dx = Gamma v + g is linear in
v); the prepared vectors get the rounding bound of their sums, 4 (m + 2) eps sum |terms|; certificate and sensitivities get the bounds
of tests/cert_ltv_ref.py and the rule of tests/sens_ltv_cases.py (ten times the restatement's own gap to the direct form, floor 1e-13)."""
import ctypes
import functools

import numpy as np
import pytest

import cert_ltv_ref as lr
import ltv_stage_ref
import ltv_stagewise_cases as lc
import sens_ltv_ref as tr
import sens_ref as sr

pytestmark = pytest.mark.gpu

U_TOL = 1e-5
EPS = np.finfo(np.float64).eps
ERR_INVALID, ERR_UNSUPPORTED, ERR_NOT_DESIGNED = -1, -4, -5
FORMS = ("host", "device")


def design_args(d):
    return (d["x_ref"], d["u_ref"], d["Q"], d["R"], d["S"], d["P"], d["umin"], d["umax"])


@functools.lru_cache(maxsize=None)
def _hip():
    """the HIP runtime the library is linked against (it is in the process once a handle exists)"""
    with open("/proc/self/maps") as f:
        path = next(ln.split()[-1] for ln in f if "libamdhip64" in ln)
    lib = ctypes.CDLL(path)
    lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    lib.hipFree.argtypes = [ctypes.c_void_p]
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.hipSetDevice.argtypes = [ctypes.c_int]
    for fn in (lib.hipMalloc, lib.hipFree, lib.hipMemcpy, lib.hipSetDevice, lib.hipDeviceSynchronize):
        fn.restype = ctypes.c_int
    return lib


class DeviceArray:
    """float64 device memory of device 0 holding a copy of a contiguous numpy array (complete when the constructor returns)"""

    def __init__(self, a):
        hip = _hip()
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = ctypes.c_void_p()
        assert hip.hipSetDevice(0) == 0
        assert hip.hipMalloc(ctypes.byref(p), a.nbytes) == 0
        self.ptr = p.value
        assert hip.hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1) == 0   # hipMemcpyHostToDevice, synchronous

    def data_ptr(self):
        return self.ptr

    def __del__(self):
        if self.ptr:
            _hip().hipFree(self.ptr)
            self.ptr = None


def device_arrays(capi, s, d):
    """The five trajectory arrays of d in the C layout in device memory of the handle's device: (addresses, the arrays to keep)"""
    n, m, N, b = s.n, s.m, s.N, s.batch
    host = [capi._blocks(d["A_all"], b * N, n, n), capi._blocks(d["B_all"], b * N, n, m),
            None if d["c_all"] is None else np.ascontiguousarray(d["c_all"], dtype=np.float64).reshape(b, N, n),
            capi._traj_batch(d["xbar"], b, n, N + 1), capi._traj_batch(d["ubar"], b, m, N)]
    keep = [None if a is None else DeviceArray(a) for a in host]   # (complete before the call: synchronous copies)
    return [None if t is None else t.data_ptr() for t in keep], keep


def design(capi, case, d, form, s=None):
    s = s or capi.Solver(case.n, case.m, case.N, case.batch, structured=True)
    kw = dict(xmin=d["xmin"], xmax=d["xmax"], terminal=d["terminal"])
    if form == "host":
        s.design_ltv_stagewise(d["A_all"], d["B_all"], d["c_all"], d["xbar"], d["ubar"], *design_args(d), **kw)
    else:
        ptrs, keep = device_arrays(capi, s, d)
        s.design_ltv_stagewise(*ptrs, *design_args(d), on_device=True, **kw)
        s.synchronize()
        del keep
    return s


def update(capi, s, d, form):
    if form == "host":
        s.ltv_stagewise_update(d["A_all"], d["B_all"], d["c_all"], d["xbar"], d["ubar"])
        return None
    ptrs, keep = device_arrays(capi, s, d)
    s.ltv_stagewise_update(*ptrs, on_device=True)
    return keep   # (alive until the caller has synchronised)


@functools.lru_cache(maxsize=None)
def device(capi, name, form):
    """One design and step of a case in one form, shared by the tests below (read-only): dict(res, prep)"""
    case = lc.BY_NAME[name]
    d, _ = lc.answers(case)
    s = design(capi, case, d, form)
    prep = s.ltv_stagewise_prepared(eq_target=case.eq)
    s.calculate()
    res = s.get_results()
    s.close()
    return dict(res=res, prep=prep)


def check_against_oracle(mo, d, oracle, res, tag):
    """status, e_u, e_x of every instance against the oracle's answers; the two sums bit for bit; returns the worst e_u error"""
    worst = 0.0
    for i, o in enumerate(oracle):
        assert res["status"][i] == o["status"], (tag, i, res["status"][i], o["status"])
        assert np.array_equal(res["u"][i], d["ubar"][i] + res["e_u"][i]), (tag, i)
        assert np.array_equal(res["x"][i], d["xbar"][i] + res["e_x"][i]), (tag, i)
        if o["status"] != 0:
            continue
        err = float(np.abs(res["e_u"][i] - o["v"].T).max())
        worst = max(worst, err)
        assert err <= U_TOL, (tag, i, err)
        gam = lc.gamma_norm(mo, d, i)
        ex = float(np.abs(res["e_x"][i] - o["dx"]).max())
        assert ex <= U_TOL * max(1.0, gam), (tag, i, ex, gam)
        assert not res["e_x"][i][:, 0].any(), (tag, i)   # dx_0 = 0
    return worst


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_every_case_against_the_oracle(capi, mo, case, form):
    d, oracle = lc.answers(case)
    res = device(capi, case.name, form)["res"]
    assert res["u"].shape == (case.batch, case.m, case.N) and res["x"].shape == (case.batch, case.n, case.N + 1)
    worst = check_against_oracle(mo, d, oracle, res, (case.name, form))
    print(f"{case.name} [{form}] {case.build}: status {list(res['status'])}, worst |e_u - v*| {worst:.2e}")


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_both_forms_give_the_same_bits(capi, case):
    """One path: the host form uploads into the handle's buffers and then runs what the device form runs."""
    a, b = device(capi, case.name, "host"), device(capi, case.name, "device")
    for k in ("u", "e_u", "x", "e_x", "status"):
        assert a["res"][k].tobytes() == b["res"][k].tobytes(), (case.name, k)
    for k in a["prep"]:
        assert a["prep"][k].tobytes() == b["prep"][k].tobytes(), (case.name, k)


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_prepared_vectors(capi, case):
    """k_ltv_stage_prepare against the numpy restatement of the host loops, within the rounding bound of the sums"""
    d = lc.generate(case)
    prep = device(capi, case.name, "device")["prep"]
    worst = 0.0
    for i in range(case.batch):
        ref = ltv_stage_ref.prepare(d["xbar"][i], d["ubar"][i], d["x_ref"], d["u_ref"], d["R"], d["S"])
        xr = 0.0 if d["x_ref"] is None else d["x_ref"][:, 1:].T
        eb_bound = 4 * (case.m + 2) * EPS * (np.abs(d["xbar"][i][:, 1:].T) + np.abs(xr))
        assert np.all(np.abs(prep["ebar"][i] - ref["ebar"]) <= eb_bound), (case.name, i)
        q_bound = 4 * (case.m + 2) * EPS * ref["mag"]
        err = np.abs(prep["qadd"][i] - ref["qadd"])
        assert np.all(err <= q_bound), (case.name, i, float(err.max()))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(q_bound > 0, err / q_bound, 0.0))))
        if case.eq:
            assert np.array_equal(prep["eq_target"], ref["eqt"])
    if d["R"][0, 0] == 0.0:
        assert not prep["qadd"].any()   # the branch rule: R[0,0] == 0 drops R and S
    print(f"{case.name}: worst qadd error / bound {worst:.3f}")


def test_twin_of_the_condensed_design(capi, mo):
    """(5, 2, 12): the same data through almpc_design_ltv on a condensed handle; both u within U_TOL of the oracle"""
    case = lc.BY_NAME["twin-5-2-12"]
    d, oracle = lc.answers(case)
    res = device(capi, case.name, "host")["res"]
    s = capi.Solver(case.n, case.m, case.N, case.batch)
    s.design_ltv(d["A_all"], d["B_all"], d["c_all"], d["xbar"], d["ubar"], *design_args(d))
    s.update_initialization(d["xbar"][:, :, 0])
    s.calculate()
    cond = s.get_results(want=("u", "status"))
    s.close()
    for i, o in enumerate(oracle):
        ustar = d["ubar"][i] + o["v"].T
        assert cond["status"][i] == 0 and res["status"][i] == 0
        assert np.abs(cond["u"][i] - ustar).max() <= U_TOL, i
        assert np.abs(res["u"][i] - ustar).max() <= U_TOL, i


@pytest.mark.parametrize("name", ["long-4-2-70", "eq-4-2-9-S"])
def test_update_path(capi, mo, name):
    """Design once; three updates with fresh data of the same case in the device form, enqueued with the step and waited for once, each
    matching the oracle of its own data; a fourth with the first data reproduces the first result bit for bit."""
    case = lc.BY_NAME[name]
    d0, o0 = lc.answers(case)
    s = design(capi, case, d0, "device")
    s.calculate()
    first = s.get_results()
    check_against_oracle(mo, d0, o0, first, (name, "design"))
    for seed in (case.seed + 1000, case.seed + 1001, case.seed + 1002):
        d, o = lc.answers(case, seed)
        assert set(r["status"] for r in o) <= {0, 3}
        keep = update(capi, s, d, "device")
        s.calculate(sync=False)
        s.synchronize()
        del keep
        check_against_oracle(mo, d, o, s.get_results(), (name, seed))
    keep = update(capi, s, d0, "device")
    s.calculate(sync=False)
    s.synchronize()
    del keep
    again = s.get_results()
    for k in ("u", "e_u", "x", "e_x", "status"):
        assert again[k].tobytes() == first[k].tobytes(), (name, k)   # nothing of an earlier iterate survives
    update(capi, s, lc.answers(case, case.seed + 1000)[0], "host")   # the host form of the update, on the same design
    s.calculate()
    check_against_oracle(mo, *lc.answers(case, case.seed + 1000), s.get_results(), (name, "host update"))
    s.close()


# ---- a caller's outer loop: multiple shooting on a pendulum on a cart (explicit Euler; the upright position is open-loop unstable:
# 1.044 per step, 430 over the horizon), n = 4, m = 1, N = 140 -- m N beyond the condensed design's limit.
# The time step is chosen for the last check, the KKT residual of the final QP under tests/test_gpu_cert_ltv.py's bound
# 1e-9 max(1, |grad|): the gradient is H v + q with |H| ~ P (growth B)^2, so the roundings of u alone move it by eps |H| |u|.  At
# DT = 0.02 the growth is 1.5e5, |H| ~ 4e9, and that floor is ~1e-6 -- the oracle's own solution of that QP has a residual of 3.5e-6
# under tests/cert_ltv_ref.py; at DT = 0.01 |H| ~ 7e3, the floor is ~1e-10 and the oracle's residual 3e-11.
DT, GL, IL, DAMP = 0.01, 9.81 / 0.5, 1.0 / 0.5, 0.1


def cart_f(x, u):
    p, v, th, om = x
    return np.array([p + DT * v, v + DT * u[0], th + DT * om, om + DT * (GL * np.sin(th) - IL * u[0] * np.cos(th) - DAMP * om)])


def cart_jac(x, u):
    th = x[2]
    A = np.eye(4); A[0, 1] = DT; A[2, 3] = DT; A[3, 2] = DT * (GL * np.cos(th) + IL * u[0] * np.sin(th)); A[3, 3] = 1.0 - DT * DAMP
    B = np.zeros((4, 1)); B[1, 0] = DT; B[3, 0] = -DT * IL * np.cos(th)
    return A, B


def test_multiple_shooting_outer_loop(capi):
    n, m, N, b = 4, 1, 140, 4
    Q, R, P = np.diag([1.0, 0.1, 10.0, 0.1]), 0.01 * np.eye(1), 100.0 * np.eye(4)
    umin, umax = np.array([-15.0]), np.array([15.0])
    X0 = np.array([[0.3, 0, 0.25, 0], [-0.2, 0.1, -0.3, 0.2], [0.0, 0, 0.35, -0.3], [0.5, -0.2, 0.1, 0.4]])
    xbar = np.repeat(X0[:, :, None], N + 1, axis=2); ubar = np.zeros((b, m, N))

    def linearise(xbar, ubar):
        A_all, B_all, c_all = np.empty((b, N, n, n)), np.empty((b, N, n, m)), np.empty((b, N, n))
        for i in range(b):
            for k in range(N):
                A_all[i, k], B_all[i, k] = cart_jac(xbar[i, :, k], ubar[i, :, k])
                c_all[i, k] = cart_f(xbar[i, :, k], ubar[i, :, k]) - xbar[i, :, k + 1]
        return dict(A_all=A_all, B_all=B_all, c_all=c_all, xbar=xbar, ubar=ubar)

    s = capi.Solver(n, m, N, b, structured=True)
    d = linearise(xbar, ubar)
    ptrs, keep = device_arrays(capi, s, d)
    s.design_ltv_stagewise(*ptrs, None, None, Q, R, None, P, umin, umax, on_device=True)
    hist = []
    for it in range(20):
        if it > 0:
            d = linearise(xbar, ubar)
            keep = update(capi, s, d, "device")
        s.calculate()
        r = s.get_results(want=("x", "u", "e_x", "e_u", "status"))
        assert np.all(r["status"] == 0), (it, r["status"])
        hist.append((float(max(np.abs(r["e_u"]).max(), np.abs(r["e_x"]).max())), float(np.abs(d["c_all"]).max())))
        if hist[-1][0] < 1e-6 and hist[-1][1] < 1e-9:
            break
        xbar, ubar = r["x"].copy(), r["u"].copy()
    print("outer loop:", " ".join(f"{a:.1e}/{c:.1e}" for a, c in hist))
    assert hist[-1][0] < 1e-6 and hist[-1][1] < 1e-9, hist
    assert hist[0][0] > 1e-1 and np.any(np.isclose(np.abs(r["u"]), 15.0))   # a real problem: a long way to go, inputs on the box
    cert = s.certificate_ltv(("res", "grad"))
    for i in range(b):   # the KKT residual of the last QP: the bound of tests/test_gpu_cert_ltv.py
        assert cert["res"][i] <= 1e-9 * max(1.0, float(np.max(np.abs(cert["grad"][i])))), (i, cert["res"][i])
    s.close()
    del keep


def test_certificate_and_sensitivities_without_rows(capi, mo):
    """(4, 2, 70), input box only: every output of almpc_certificate_ltv against tests/cert_ltv_ref.py at the handle's own u, e_u, and
    K0 of almpc_sensitivity_ltv against tests/sens_ltv_ref.py -- no almpc_set_keep_stage_models: the solver keeps the models."""
    case = lc.BY_NAME["long-4-2-70"]
    d, _ = lc.answers(case)
    s = design(capi, case, d, "device")
    s.calculate()
    res = s.get_results()
    cert = s.certificate_ltv()
    sens = s.sensitivity_ltv(("K0",))
    s.close()
    n, m, N = case.n, case.m, case.N
    for i in range(case.batch):
        assert res["status"][i] == 0
        ref = lr.certificate_ltv(d["A_all"][i], d["B_all"][i], d["c_all"][i], d["xbar"][i], d["x_ref"], d["u_ref"], d["Q"], d["R"], d["S"],
                                 d["P"], d["umin"], d["umax"], res["e_u"][i], res["u"][i])
        for key in ("cost", "res", "grad", "costate", "x", "e_x"):
            err = np.abs(np.asarray(cert[key][i]) - ref[key])
            assert np.all(err <= ref["tol_" + key]), (i, key, float(np.max(err)))
        assert cert["res"][i] <= 1e-9 * max(1.0, float(np.max(np.abs(cert["grad"][i]))))
        # the predicted states of the certificate are the step's own x, e_x up to the rounding of two rollouts
        assert np.abs(cert["x"][i] - res["x"][i]).max() <= U_TOL * max(1.0, lc.gamma_norm(mo, d, i))
        act = tr.active_rows(res["u"][i], d["umin"], d["umax"])
        assert sens["rows"][i] == act.sum()
        J, _ = tr.jacobians(d["A_all"][i], d["B_all"][i], d["Q"], d["R"], d["S"], d["P"], act)
        H, _, _, _, Gam, _ = mo.ltv_qp(d["A_all"][i], d["B_all"][i], d["c_all"][i], d["xbar"][i], d["ubar"][i], d["x_ref"], d["u_ref"],
                                       d["Q"], d["R"], d["S"], d["P"], d["umin"], d["umax"], return_prediction=True)
        Jd, _ = tr.jac_direct(d["A_all"][i], d["B_all"][i], d["Q"], d["P"], H, Gam, act)
        scale = max(1.0, float(np.abs(J).max()))
        gap = float(np.abs(J - Jd).max()) / scale
        tol = max(10.0 * gap, 1e-13)   # the rule of tests/sens_ltv_cases.py: ten times the restatement's own gap, floor 1e-13
        K0, _ = sr.shaped(J, m, N)
        err = float(np.abs(sens["K0"][i] - K0).max()) / scale
        print(f"instance {i}: rows {int(act.sum())}, K0 error / scale {err:.2e} (tolerance {tol:.2e})")
        assert err <= tol, (i, err, tol)


def _code(capi, call):
    with pytest.raises(capi.AlmpcError) as ei:
        call()
    return ei.value.code


def message(s):
    return (s.L.almpc_last_error(s.h) or b"").decode()


def test_certificate_with_state_rows_serves_cost_and_states_only(capi):
    case = lc.BY_NAME["box-7-3-10"]
    d, _ = lc.answers(case)
    s = design(capi, case, d, "host")
    s.calculate()
    res = s.get_results()
    part = s.certificate_ltv(("cost", "x", "e_x"))
    assert set(part) == {"cost", "x", "e_x"} and np.all(np.isfinite(part["cost"]))
    for i in range(case.batch):
        ref = lr.certificate_ltv(d["A_all"][i], d["B_all"][i], d["c_all"][i], d["xbar"][i], d["x_ref"], d["u_ref"], d["Q"], d["R"], d["S"],
                                 d["P"], d["umin"], d["umax"], res["e_u"][i], res["u"][i])
        for key in ("cost", "x", "e_x"):
            assert np.all(np.abs(np.asarray(part[key][i]) - ref[key]) <= ref["tol_" + key]), (i, key)
    for want in (("res",), ("grad",), ("costate",)):
        assert _code(capi, lambda: s.certificate_ltv(want)) == ERR_UNSUPPORTED
    assert _code(capi, lambda: s.sensitivity_ltv(("K0",))) == ERR_UNSUPPORTED and "state rows" in message(s)
    s.close()


def _zeros(n, m, N, b):
    return dict(A_all=np.zeros((b, N, n, n)), B_all=np.ones((b, N, n, m)), c_all=None, xbar=np.zeros((b, n, N + 1)), ubar=np.zeros((b, m, N)))


def test_refusals(capi):
    """None of these launches anything: the shape and kind checks come before the first device call of the design."""
    n, m, N, b = 20, 9, 6, 3
    z = _zeros(n, m, N, b)
    args = (z["A_all"], z["B_all"], None, z["xbar"], z["ubar"], None, None, np.eye(n), np.eye(m))
    box = dict(umin=-np.ones(m), umax=np.ones(m))
    s = capi.Solver(n, m, N, b, structured=True)
    # (20, 9, 6) with a state box / with S (nt = 29): the table-less G = 1 builds of k_sdual
    assert _code(capi, lambda: s.design_ltv_stagewise(*args, None, np.eye(n), xmin=-np.ones(n), xmax=np.ones(n), **box)) == ERR_UNSUPPORTED
    assert "G = 1" in message(s) and "(32, 16)" in message(s) and "(48, 16)" in message(s)
    assert _code(capi, lambda: s.design_ltv_stagewise(*args, 0.4 * np.eye(m), np.eye(n), **box)) == ERR_UNSUPPORTED
    assert "G = 1" in message(s)
    assert _code(capi, lambda: s.calculate()) == ERR_NOT_DESIGNED
    # update before design
    assert _code(capi, lambda: s.ltv_stagewise_update(z["A_all"], z["B_all"], None, z["xbar"], z["ubar"])) == ERR_NOT_DESIGNED
    # the same shape with an input box alone is served (k_riccati_t), then: c_all mismatch, set_reference, almpc_design_ltv
    s.design_ltv_stagewise(*args, None, np.eye(n), **box)
    assert _code(capi, lambda: s.ltv_stagewise_update(z["A_all"], z["B_all"], np.zeros((b, N, n)), z["xbar"], z["ubar"])) == ERR_INVALID
    assert "c_all" in message(s)
    assert _code(capi, lambda: s.set_reference(np.zeros((n, N + 1)), np.zeros((m, N)))) == ERR_INVALID
    assert _code(capi, lambda: s.design_ltv(*args, None, np.eye(n), **box)) == ERR_UNSUPPORTED
    assert message(s) == "structured solve: time-varying designs go through almpc_sqp_fnn_* (stage models on the device)"
    s.close()
    sc = capi.Solver(4, 2, 9, b, structured=True)
    zc = _zeros(4, 2, 9, b)
    sc.design_ltv_stagewise(zc["A_all"], zc["B_all"], np.zeros((b, 9, 4)), zc["xbar"], zc["ubar"], None, None, np.eye(4), np.eye(2), None,
                            np.eye(4), -np.ones(2), np.ones(2))
    assert _code(capi, lambda: sc.ltv_stagewise_update(zc["A_all"], zc["B_all"], None, zc["xbar"], zc["ubar"])) == ERR_INVALID
    assert "c_all" in message(sc)
    sc.close()
    # a condensed handle: almpc_design_ltv is its call
    c = capi.Solver(4, 2, 9, b)
    assert _code(capi, lambda: c.design_ltv_stagewise(zc["A_all"], zc["B_all"], None, zc["xbar"], zc["ubar"], None, None, np.eye(4), np.eye(2),
                                                      None, np.eye(4), -np.ones(2), np.ones(2))) == ERR_UNSUPPORTED
    assert "almpc_design_ltv" in message(c)
    c.close()
