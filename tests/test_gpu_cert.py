"""GPU tests of k_cert (csrc/almpc_cert.hip.h): almpc_certificate, almpc_get_certificate, almpc_device_certificate and the group forms.

Every case of tests/cert_cases.py steps, fetches the results and the certificate, and is compared per instance with tests/cert_ref.py
evaluated at the handle's OWN returned e_x, e_u, u (and, where the design computed the terminal weight, at the P the handle kept), so
both sides certify the same trajectory.  The tolerance of every comparison is cert_ref's rounding bound 2 ops u mag / (1 - ops u)
(both sides carry at most gamma_ops mag in any summation order); it is derived, not measured.  Every case prints its worst ratio to it.
"""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import cert_cases as cc
import cert_ref as cr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_NOT_DESIGNED = -1, -4, -5
ALL = ("cost", "res", "grad", "costate")


def design(capi, c, make=None, **kw):
    """a handle (or group) designed on a case, references set"""
    s = make() if make else capi.Solver(c.n, c.m, c.N, c.batch, structured=c.structured)
    p0 = c.problems[0]
    if c.kind == "shared":
        s.design_shared(p0.A, p0.B, p0.Q, p0.R, p0.S, None if c.P == "dare" else p0.P, p0.u_min, p0.u_max, **kw)
    else:
        A, B = np.stack([p.A for p in c.problems]), np.stack([p.B for p in c.problems])
        P = None if c.P == "dare" else p0.P if c.P == "given" else np.stack([p.P for p in c.problems])
        if c.kind == "batched":
            s.design_batched(A, B, p0.Q, p0.R, p0.S, P, p0.u_min, p0.u_max)
        else:
            s.design_batched_weighted(A, B, np.stack([p.Q for p in c.problems]), np.stack([p.R for p in c.problems]),
                                      np.stack([p.S for p in c.problems]), P, p0.u_min, p0.u_max)
    if c.refs == "instance":
        s.set_reference(np.stack([p.x_ref for p in c.problems]), np.stack([p.u_ref for p in c.problems]), per_instance=True)
    else:
        s.set_reference(p0.x_ref, p0.u_ref)
    return s


def step(capi, c, opts=None, X0=None):
    s = design(capi, c)
    s.update_initialization(c.X0 if X0 is None else X0)
    s.calculate(opts)
    return s


def terminal_weights(s, c):
    """the P of every instance: the case's where the design was given it, the handle's where the design computed it"""
    if c.P != "dare":
        return [p.P for p in c.problems]
    if c.kind == "shared":
        return [np.array(s.terminal_weight_instance(0))] * c.batch
    return [np.array(s.terminal_weight_instance(i)) for i in range(c.batch)]


def reference(c, res, Ps):
    out = []
    for i, p in enumerate(c.problems):
        out.append(cr.certificate(p.A, p.B, p.Q, p.R, p.S, Ps[i], p.u_min, p.u_max, res["e_x"][i], res["e_u"][i], res["u"][i]))
    return out


def compare(name, cert, ref):
    """every value within its bound; returns the worst ratio"""
    worst = 0.0
    for i, k in enumerate(ref):
        for key, got, want, tol in (("cost", cert["cost"][i], k["cost"], k["tol_cost"]), ("res", cert["res"][i], k["res"], k["tol_res"]),
                                    ("grad", cert["grad"][i], k["grad"], k["tol_grad"]), ("costate", cert["costate"][i], k["costate"], k["tol_costate"])):
            err = np.abs(np.asarray(got) - want)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = float(np.max(np.where(err == 0.0, 0.0, err / tol)))
            worst = max(worst, ratio)
            assert np.all(err <= tol), (name, i, key, ratio)
    return worst


@functools.lru_cache(maxsize=None)
def device(capi, name):
    """One step of a case and its certificate, shared by the tests below (read-only)."""
    c = cc.case(name)
    s = step(capi, c)
    res = s.get_results()
    cert = s.certificate()
    Ps = terminal_weights(s, c)
    s.close()
    return dict(res=res, cert=cert, P=Ps)


@pytest.mark.parametrize("name", cc.NAMES)
def test_certificate_of_every_case(capi, name):
    c = cc.case(name)
    d = device(capi, name)
    res, cert = d["res"], d["cert"]
    assert cert["cost"].shape == (c.batch,) and cert["res"].shape == (c.batch,)
    assert cert["grad"].shape == res["u"].shape and cert["costate"].shape == res["x"].shape
    ref = reference(c, res, d["P"])
    worst = compare(name, cert, ref)
    print(f"{name}: worst error / bound {worst:.3f}; res max {cert['res'].max():.3e}, |g| max {np.abs(cert['grad']).max():.3e}")
    # a solved batch: the solver's verdict and the method-independent one agree
    assert np.all(res["status"] == 0), np.bincount(res["status"])
    for i in range(c.batch):
        assert cert["res"][i] <= 1e-9 * max(1.0, float(np.max(np.abs(cert["grad"][i])))), (name, i, cert["res"][i])


def test_unsolved_inputs_are_certified_as_they_are(capi):
    c = cc.case("quad-12-4-5")
    s = step(capi, c, capi.default_opts(polish=0, max_iter=2))
    res, cert = s.get_results(), s.certificate()
    s.close()
    worst = compare(c.name, cert, reference(c, res, device(capi, c.name)["P"]))
    print(f"unsolved: worst error / bound {worst:.3f}; res {cert['res'].min():.3e} .. {cert['res'].max():.3e}; status {np.bincount(res['status'])}")
    assert np.all(np.isfinite(cert["res"])) and np.any(cert["res"] > 1e-6)
    assert np.any(res["status"] != 0)   # (the certificate does not follow the status: every instance above was compared)


def test_multipliers_of_a_solved_batch(capi):
    """The signs carry no tolerance: the case holds no input that sits weakly at a bound (cert_cases.QUAD_MULTIPLIER_MARGIN, asserted at
    the exact optimum by tests/test_cert_restatement.py)."""
    c = cc.case("quad-12-4-5")
    d = device(capi, c.name)
    p = c.problems[0]
    u = d["res"]["u"]
    mu = capi.multipliers(d["cert"]["grad"], u, p.u_min, p.u_max, 1e-9)
    lo, hi = p.u_min.reshape(1, -1, 1), p.u_max.reshape(1, -1, 1)
    at_hi, at_lo = np.broadcast_to(u >= hi - 1e-9 * (hi - lo), u.shape), np.broadcast_to(u <= lo + 1e-9 * (hi - lo), u.shape)
    assert at_hi.any() and at_lo.any()
    assert np.all(mu[at_hi] >= 0.0), float(mu[at_hi].min())
    assert np.all(mu[at_lo] <= 0.0), float(mu[at_lo].max())
    assert np.all(mu[~(at_hi | at_lo)] == 0.0) and np.any(mu != 0.0)
    assert np.array_equal(mu[at_hi | at_lo], -d["cert"]["grad"][at_hi | at_lo])


def test_results_do_not_depend_on_the_position_in_the_batch(capi):
    c = cc.case("quad-12-4-5")
    X0 = c.X0.copy()
    probe = c.X0[26]   # (amplitude 3: clamped inputs)
    X0[0] = X0[1] = X0[66] = probe
    s = step(capi, c, X0=X0)
    res, cert = s.get_results(), s.certificate()
    s.close()
    one = cc.Case("quad-one", "shared", c.problems[:1], probe[None])
    s1 = step(capi, one)
    res1, cert1 = s1.get_results(), s1.certificate()
    s1.close()
    for i in (0, 1, 66):   # the premise: the step gave the three copies the same trajectories
        for k in ("e_x", "e_u", "u"):
            assert res[k][i].tobytes() == res[k][0].tobytes() == res1[k][0].tobytes(), ("step", k, i)
        for k in ALL:
            assert np.asarray(cert[k][i]).tobytes() == np.asarray(cert[k][0]).tobytes() == np.asarray(cert1[k][0]).tobytes(), (k, i)


def test_a_partial_want_returns_the_bytes_of_the_full_call(capi):
    for name in ("quad-12-4-5", "struct-4-2-70-S"):
        c = cc.case(name)
        s = step(capi, c)
        full = s.certificate()
        for k in ALL + (("cost", "res"), ("grad", "costate")):
            part = s.certificate(k)
            keys = (k,) if isinstance(k, str) else k
            assert set(part) == set(keys)
            for kk in keys:
                assert part[kk].tobytes() == full[kk].tobytes(), (name, k, kk)
            rest = [q for q in ALL if q not in keys]   # what was not asked for is not served from an earlier call
            args = [None] * 4
            args[ALL.index(rest[0])] = np.empty(full[rest[0]].size).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
            assert s.L.almpc_get_certificate(s.h, *args) == ERR_INVALID
        s.close()


def _hip():
    with open("/proc/self/maps") as f:
        path = next(ln.split()[-1] for ln in f if "libamdhip64" in ln)
    lib = ctypes.CDLL(path)
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.hipMemcpy.restype = ctypes.c_int
    return lib


def test_device_view_points_at_what_the_getter_copies(capi):
    c = cc.case("inst-dare")
    s = step(capi, c)
    with pytest.raises(capi.AlmpcError):
        s.device_certificate()   # nothing computed for this step yet
    cert = s.certificate()
    ptrs = s.device_certificate()
    hip = _hip()
    for k in ALL:
        buf = np.empty(cert[k].size)
        assert ptrs[k] and hip.hipMemcpy(buf.ctypes.data, ptrs[k], buf.nbytes, 2) == 0
        want = cert[k] if cert[k].ndim == 1 else cert[k].transpose(0, 2, 1)
        assert buf.tobytes() == np.ascontiguousarray(want).tobytes(), k
    s.certificate(("cost",))
    ptrs = s.device_certificate()
    assert ptrs["cost"] and not ptrs["res"] and not ptrs["grad"] and not ptrs["costate"]
    s.close()


@pytest.mark.parametrize("name", ("quad-12-4-5", "weighted-S", "struct-inst-5-3-12"))
def test_group_equals_one_handle(capi, name):
    c = cc.case(name)
    g = design(capi, c, make=lambda: capi.Group(c.n, c.m, c.N, c.batch, devices=[0, 0], structured=c.structured))
    g.update_initialization(c.X0)
    g.calculate()
    res, cert = g.get_results(), g.certificate()
    part = g.certificate(("res",))
    g.close()
    d = device(capi, name)
    for k in ("e_x", "e_u", "u"):
        assert res[k].tobytes() == d["res"][k].tobytes(), ("step", k)
    for k in ALL:
        assert cert[k].tobytes() == d["cert"][k].tobytes(), k
    assert part["res"].tobytes() == cert["res"].tobytes()


def _code(capi, call):
    with pytest.raises(capi.AlmpcError) as e:
        call()
    return e.value.code


def test_refusals(capi, mo):
    p = mo.double_integrator(N=10)
    X0 = 0.5 * np.random.default_rng(1).normal(size=(4, 2))
    message = lambda s: (s.L.almpc_last_error(s.h) or b"").decode().strip()
    sv = capi.Solver(2, 1, 10, 4)
    assert sv.L.almpc_certificate(sv.h, 1) == ERR_NOT_DESIGNED and message(sv)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    assert sv.L.almpc_certificate(sv.h, 1) == ERR_INVALID and message(sv)   # before a step
    sv.update_initialization(X0); sv.calculate()
    assert sv.L.almpc_certificate(sv.h, 0) == ERR_INVALID and message(sv)
    assert sv.L.almpc_certificate(sv.h, 16) == ERR_INVALID and sv.L.almpc_certificate(sv.h, 0x1F) == ERR_INVALID
    assert sv.L.almpc_get_certificate(sv.h, None, None, None, None) == ERR_INVALID   # nothing computed yet
    sv.certificate()
    sv.calculate()   # a new step: the certificate of the last one is gone
    cost = np.empty(4)
    assert sv.L.almpc_get_certificate(sv.h, cost.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None, None) == ERR_INVALID
    sv.certificate()
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)   # a new design: no step of it yet
    assert sv.L.almpc_get_certificate(sv.h, cost.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None, None) == ERR_INVALID
    assert sv.L.almpc_certificate(sv.h, 1) == ERR_INVALID
    sv.close()
    # state box, terminal equality: the cost alone
    for kw in (dict(xmin=[-50.0, -50.0], xmax=[50.0, 50.0]), dict(terminal="equality")):
        for structured in (False, True):
            sv = capi.Solver(2, 1, 10, 4, structured=structured)
            sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, **kw)
            sv.update_initialization(0.1 * X0); sv.calculate()
            for want in ("res", "grad", "costate", ALL, ("cost", "res")):
                assert _code(capi, lambda: sv.certificate(want)) == ERR_UNSUPPORTED and message(sv)
            cert, res = sv.certificate(("cost",)), sv.get_results()
            P = np.array(sv.terminal_weight_instance(0))
            for i in range(4):
                k = cr.certificate(p.A, p.B, p.Q, p.R, p.S, P, p.u_min, p.u_max, res["e_x"][i], res["e_u"][i], res["u"][i])
                assert abs(cert["cost"][i] - k["cost"]) <= k["tol_cost"], (kw, structured, i)
            sv.close()
    # time-varying design
    sv = capi.Solver(2, 1, 10, 4)
    A_all, B_all = np.tile(p.A, (4, 10, 1, 1)), np.tile(p.B, (4, 10, 1, 1))
    xbar = np.zeros((4, 2, 11)); xbar[:, :, 0] = X0
    for k in range(10):
        xbar[:, :, k + 1] = xbar[:, :, k] @ p.A.T
    sv.design_ltv(A_all, B_all, None, xbar, np.zeros((4, 1, 10)), None, None, p.Q, p.R, None, p.P, p.u_min, p.u_max)
    assert _code(capi, lambda: sv.certificate(("cost",))) == ERR_UNSUPPORTED and message(sv)
    sv.close()
    # the SQP loop and the re-linearisation pipeline of a black-box model
    f = mo.synthetic_fnn()
    n, m, N = 4, 2, 10
    x_ref, u_ref = np.zeros((n, N + 1)), np.zeros((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    Al, Bl = capi.fnn_linearize(f.W_in, f.W_h, f.b_h, f.W_out, x_ref[:, -1][None], u_ref[:, -1][None], act=f.act)
    P = capi.dare(Al[0], Bl[0], Q, R)
    x0 = 0.05 * np.random.default_rng(2).normal(size=(4, n))
    sv = capi.Solver(n, m, N, 4)
    sv.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act)
    sv.update_initialization(x0)
    sv.relin_fnn_step()
    assert _code(capi, lambda: sv.certificate(("cost",))) == ERR_UNSUPPORTED and message(sv)
    sv.close()
    sv = capi.Solver(n, m, N, 4)
    sv.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act)
    sv.sqp_fnn_start(x0)
    sv.sqp_fnn_iterate(1)
    assert _code(capi, lambda: sv.certificate(("cost",))) == ERR_UNSUPPORTED and message(sv)
    sv.close()
    # m beyond the kernel's 16
    q = mo.make_problem(np.array([[0.9, 0.1], [0.0, 0.8]]), np.ones((2, 17)), 2, -np.ones(17), np.ones(17))
    sv = capi.Solver(2, 17, 2, 3)
    sv.design_shared(q.A, q.B, q.Q, q.R, q.S, None, q.u_min, q.u_max)
    sv.update_initialization(np.ones((3, 2))); sv.calculate()
    assert _code(capi, lambda: sv.certificate(("cost",))) == ERR_UNSUPPORTED and message(sv)
    sv.close()


def test_controller_mirror(pkg, capi, mo):
    """certificate(C) of the Python mirror is Solver.certificate of its handle: a batched controller, and one instance without the
    batch axis."""
    p = mo.double_integrator(N=10)
    X, U = pkg.Hyperrectangle([-100.0] * 2, [100.0] * 2), pkg.Hyperrectangle(p.u_min, p.u_max)
    sys_ = pkg.ConstrainedLinearControlDiscreteSystem(p.A, p.B, X, U)
    X0 = 3.0 * np.random.default_rng(7).normal(size=(8, 2))
    for b in (8, 1):
        C = pkg.proceed_controller(sys_, "model_predictive_control", 10, 1, [0.0, 0.0], [0.0], mpc_batch=b)
        pkg._model_predictive_control_computation(C, X0[:b])
        got = pkg.certificate(C)
        sv = C.tuning.modeler.solver
        own = sv.certificate()
        assert sorted(got) == sorted(ALL)
        for k, v in own.items():
            assert np.array_equal(got[k], v[0] if b == 1 else v), k
        assert got["grad"].shape == ((1, 10) if b == 1 else (8, 1, 10)) and got["costate"].shape == ((2, 11) if b == 1 else (8, 2, 11))
        sv.close()
    assert "certificate" in importlib.import_module(pkg.__name__ + ".controller").__all__
