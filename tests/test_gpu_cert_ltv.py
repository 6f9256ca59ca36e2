"""GPU tests of k_cert_ltv (csrc/almpc_cert_ltv.hip.h): almpc_set_keep_stage_models, almpc_certificate_ltv, almpc_get_certificate_ltv,
almpc_device_certificate_ltv, and of almpc_relin_fnn_certificate / almpc_group_relin_fnn_certificate (k_cert on the step's own models).

Every case of tests/cert_ltv_cases.py is designed with the keep switch on, stepped, and compared per instance with tests/cert_ltv_ref.py
evaluated at the handle's OWN returned u and e_u, so both sides certify the same step.  The tolerance of every comparison is the
restatement's rounding bound 2 ops u mag / (1 - ops u) (both sides carry at most gamma_ops mag in any summation order); it is derived,
not measured.  Every case prints its worst ratio to it."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import cert_ltv_cases as lc
import cert_ltv_ref as lr
import cert_ref as cr
import nlp_shape_cases as nc
from conftest import ROOT
from test_gpu_nlp_shapes import _num_cus

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_NOT_DESIGNED = -1, -4, -5
ALL = ("cost", "res", "grad", "costate", "x", "e_x")
CERT4 = ("cost", "res", "grad", "costate")
_dp = ctypes.POINTER(ctypes.c_double)


def design_args(a):
    return (a["A_all"], a["B_all"], a["c_all"], a["xbar"], a["ubar"], a["x_ref"], a["u_ref"], a["Q"], a["R"], a["S"], a["P"], a["umin"], a["umax"])


def step(capi, a, opts=None, keep=True):
    """a handle designed on design_ltv's arguments `a` (the keep switch on), one step taken"""
    b, N, n = a["A_all"].shape[:3]
    s = capi.Solver(n, a["B_all"].shape[3], N, b)
    s.design_ltv(*design_args(a), keep_stage_models=keep)
    s.update_initialization(a["xbar"][:, :, 0])
    s.calculate(opts)
    return s


def reference(a, res, which=None):
    out = []
    for i in (range(a["A_all"].shape[0]) if which is None else which):
        P = a["P"][i] if a["P"].ndim == 3 else a["P"]
        out.append(lr.certificate_ltv(a["A_all"][i], a["B_all"][i], None if a["c_all"] is None else a["c_all"][i], a["xbar"][i], a["x_ref"],
                                      a["u_ref"], a["Q"], a["R"], a["S"], P, a["umin"], a["umax"], res["e_u"][i], res["u"][i]))
    return out


def compare(name, cert, ref, keys=ALL):
    """every value within its bound; returns the worst ratio"""
    worst = 0.0
    for i, k in enumerate(ref):
        for key in keys:
            err = np.abs(np.asarray(cert[key][i]) - k[key])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = float(np.max(np.where(err == 0.0, 0.0, err / k["tol_" + key])))
            worst = max(worst, ratio)
            assert np.all(err <= k["tol_" + key]), (name, i, key, ratio)
    return worst


@functools.lru_cache(maxsize=None)
def device(capi, name):
    """One step of a case and its certificate, shared by the tests below (read-only)."""
    s = step(capi, lc.inputs(name))
    res = s.get_results(want=("u", "e_u", "status"))
    cert = s.certificate_ltv()
    qp = {i: (s.get_design_instance(i)["H"], s.get_gradient_instance(i)) for i in range(4)} if name in ("4-3-N7-b4", "16-3-4") else None
    s.close()
    return dict(res=res, cert=cert, qp=qp)


def _kernel_constant(name):
    with open(os.path.join(ROOT, "automationlabsmodelpredictivecontrol.jl_amd", "csrc", "almpc_cert_ltv.hip.h")) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


@pytest.mark.parametrize("name", lc.NAMES)
def test_certificate_of_every_case(capi, name):
    n, m, N = lc.shape(name)
    a = lc.inputs(name)
    d = device(capi, name)
    res, cert = d["res"], d["cert"]
    assert cert["cost"].shape == (4,) and cert["res"].shape == (4,) and cert["grad"].shape == (4, m, N)
    assert cert["costate"].shape == cert["x"].shape == cert["e_x"].shape == (4, n, N + 1)
    ref = reference(a, res)
    worst = compare(name, cert, ref)
    print(f"{name}: worst error / bound {worst:.3f}; res max {cert['res'].max():.3e}, |g| max {np.abs(cert['grad']).max():.3e}")
    assert np.all(res["status"] == 0), res["status"]
    for i in range(4):
        assert cert["res"][i] <= 1e-9 * max(1.0, float(np.max(np.abs(cert["grad"][i])))), (name, i, cert["res"][i])
    if d["qp"]:
        # grad = H v + q with the handle's own H and q: the design kernels build them as mo.ltv_qp does (cert_ltv_ref.qp_bound, one side
        # each, and the product here)
        import mpc_oracle as mo
        for i in range(4):
            k, ubar = lc.instance(name, i)
            useR, useS = cr.branch(k["R"], k["S"])
            qb = lr.qp_bound(mo, k["A"], k["B"], k["c"], k["xbar"], ubar, k["xref"], k["uref"], k["Q"], k["R"], k["S"], k["P"], k["umin"],
                             k["umax"], useR, useS)
            H, q = d["qp"][i]
            v = res["e_u"][i].T.reshape(-1)
            g = (H @ v + q).reshape(N, m).T
            tol = 0.5 * ref[i]["tol_grad"] + 2.0 * cr.gamma(qb["ops"]) * (qb["H"] @ np.abs(v) + qb["q"]).reshape(N, m).T
            assert np.all(np.abs(cert["grad"][i] - g) <= tol), (name, i, float(np.max(np.abs(cert["grad"][i] - g) / tol)))


def test_every_wave_walks_three_instances_and_more(capi):
    """The persistent loop: the (2, 1, 2) case tiled to three instances per wave of the capped grid and five more.  All copies of each of
    the four instances have identical bytes in all six outputs (what a wave staged once -- the weights, the shared P, the box -- serves every instance it walks), and the first four match the restatement."""
    name = "2-1-N2-b4"
    waves = _kernel_constant("CERT_LTV_WGS_PER_CU") * _num_cus() * _kernel_constant("CERT_LTV_WAVES")
    b = 3 * waves + 5
    reps = (b + 3) // 4
    a = {k: (v if v is None or k in ("x_ref", "u_ref", "Q", "R", "S", "P", "umin", "umax") else np.tile(v, (reps,) + (1,) * (v.ndim - 1))[:b])
         for k, v in lc.inputs(name).items()}
    s = step(capi, a)
    res = s.get_results(want=("u", "e_u", "status"))
    cert = s.certificate_ltv()
    s.close()
    assert np.all(res["status"] == 0)
    for k in ("u", "e_u"):   # the premise: the step gave the copies the same inputs
        for j in range(4):
            assert np.all(res[k][j::4] == res[k][j]), ("step", k, j)
    for k in ALL:
        for j in range(4):
            copies = np.ascontiguousarray(cert[k][j::4])
            first = np.ascontiguousarray(cert[k][j:j + 1])
            assert copies.tobytes() == np.repeat(first, copies.shape[0], axis=0).tobytes(), (k, j)
    worst = compare(name, cert, reference(a, res, range(4)))
    print(f"persistent loop: batch {b}, {waves} waves; worst error / bound {worst:.3f}")


def test_results_do_not_depend_on_the_position_in_the_batch(capi):
    name = "4-3-N7-b4"
    a0 = lc.inputs(name)
    per_inst = ("A_all", "B_all", "c_all", "xbar", "ubar")
    a = dict(a0)
    for k in per_inst:
        v = a0[k].copy()
        v[0] = v[1] = v[3] = a0[k][2]
        a[k] = v
    one = dict(a0)
    for k in per_inst:
        one[k] = a0[k][2:3].copy()
    s, s1 = step(capi, a), step(capi, one)
    res, cert = s.get_results(want=("u", "e_u")), s.certificate_ltv()
    res1, cert1 = s1.get_results(want=("u", "e_u")), s1.certificate_ltv()
    s.close(); s1.close()
    for i in (0, 1, 3):
        for k in ("u", "e_u"):   # the premise
            assert res[k][i].tobytes() == res[k][2].tobytes() == res1[k][0].tobytes(), ("step", k, i)
        for k in ALL:
            assert np.asarray(cert[k][i]).tobytes() == np.asarray(cert[k][2]).tobytes() == np.asarray(cert1[k][0]).tobytes(), (k, i)


def test_a_partial_want_returns_the_bytes_of_the_full_call(capi):
    name = "6-1-N5-b4-pinst"
    s = step(capi, lc.inputs(name))
    full = s.certificate_ltv()
    for k in CERT4 + (("x", "e_x"), ("cost", "res"), ("grad", "costate"), ("cost", "x", "e_x")):
        part = s.certificate_ltv(k)
        keys = (k,) if isinstance(k, str) else k
        assert set(part) == set(keys)
        for kk in keys:
            assert part[kk].tobytes() == full[kk].tobytes(), (k, kk)
        rest = [q for q in ALL if q not in keys]   # what was not asked for is not served from an earlier call
        args = [None] * 6
        args[ALL.index(rest[0])] = np.empty(full[rest[0]].size).ctypes.data_as(_dp)
        assert s.L.almpc_get_certificate_ltv(s.h, *args) == ERR_INVALID
    s.close()


def test_unsolved_inputs_are_certified_as_they_are(capi):
    name = "7-2-N64-b4"
    a = lc.inputs(name)
    s = step(capi, a, capi.default_opts(polish=0, max_iter=2))
    res, cert = s.get_results(want=("u", "e_u", "status")), s.certificate_ltv()
    s.close()
    worst = compare(name, cert, reference(a, res))
    print(f"unsolved: worst error / bound {worst:.3f}; res {cert['res'].min():.3e} .. {cert['res'].max():.3e}; status {res['status']}")
    assert np.all(np.isfinite(cert["res"])) and np.any(cert["res"] > 1e-6)
    assert np.any(res["status"] != 0)


def _hip():
    with open("/proc/self/maps") as f:
        path = next(ln.split()[-1] for ln in f if "libamdhip64" in ln)
    lib = ctypes.CDLL(path)
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.hipMemcpy.restype = ctypes.c_int
    return lib


def test_device_view_points_at_what_the_getter_copies(capi):
    s = step(capi, lc.inputs("12-4-N3-b4"))
    with pytest.raises(capi.AlmpcError):
        s.device_certificate_ltv()   # nothing computed for this step yet
    cert = s.certificate_ltv()
    ptrs = s.device_certificate_ltv()
    hip = _hip()
    for k in ALL:
        buf = np.empty(cert[k].size)
        assert ptrs[k] and hip.hipMemcpy(buf.ctypes.data, ptrs[k], buf.nbytes, 2) == 0
        want = cert[k] if cert[k].ndim == 1 else cert[k].transpose(0, 2, 1)
        assert buf.tobytes() == np.ascontiguousarray(want).tobytes(), k
    s.certificate_ltv(("cost",))
    ptrs = s.device_certificate_ltv()
    assert ptrs["cost"] and not any(ptrs[k] for k in ALL[1:])
    s.close()


def _code(capi, call):
    with pytest.raises(capi.AlmpcError) as e:
        call()
    return e.value.code


def test_refusals(capi, mo):
    message = lambda s: (s.L.almpc_last_error(s.h) or b"").decode().strip()
    a = lc.inputs("4-2-N3-b4")
    n, m, N = lc.shape("4-2-N3-b4")
    X0 = a["xbar"][:, :, 0]
    sv = capi.Solver(n, m, N, 4)
    assert sv.L.almpc_certificate_ltv(sv.h, 1) == ERR_NOT_DESIGNED and message(sv)
    sv.design_ltv(*design_args(a), keep_stage_models=True)
    assert sv.L.almpc_certificate_ltv(sv.h, 1) == ERR_INVALID and message(sv)   # before a step
    sv.update_initialization(X0); sv.calculate()
    assert sv.L.almpc_certificate_ltv(sv.h, 0) == ERR_INVALID and message(sv)
    assert sv.L.almpc_certificate_ltv(sv.h, 32) == ERR_INVALID and sv.L.almpc_certificate_ltv(sv.h, 0x3F) == ERR_INVALID
    assert sv.L.almpc_get_certificate_ltv(sv.h, *[None] * 6) == ERR_INVALID   # nothing computed yet
    assert _code(capi, lambda: sv.certificate(("cost",))) == ERR_UNSUPPORTED   # almpc_certificate still refuses the design
    sv.certificate_ltv()
    sv.calculate()   # a new step: the certificate of the last one is gone
    cost = np.empty(4)
    assert sv.L.almpc_get_certificate_ltv(sv.h, cost.ctypes.data_as(_dp), *[None] * 5) == ERR_INVALID
    sv.certificate_ltv()
    sv.design_ltv(*design_args(a))   # a new design (the switch stays on): no step of it yet
    assert sv.L.almpc_get_certificate_ltv(sv.h, cost.ctypes.data_as(_dp), *[None] * 5) == ERR_INVALID
    assert sv.L.almpc_certificate_ltv(sv.h, 1) == ERR_INVALID
    sv.update_initialization(X0); sv.calculate()
    kept = sv.certificate_ltv()
    # the keep switch off: the design released its stage models, and the message names the switch
    sv.design_ltv(*design_args(a), keep_stage_models=False)
    sv.update_initialization(X0); sv.calculate()
    assert _code(capi, lambda: sv.certificate_ltv(("cost",))) == ERR_INVALID and "almpc_set_keep_stage_models" in message(sv)
    sv.design_ltv(*design_args(a), keep_stage_models=True)   # ... and on again: the bytes of before
    sv.update_initialization(X0); sv.calculate()
    again = sv.certificate_ltv()
    for k in ALL:
        assert again[k].tobytes() == kept[k].tobytes(), k
    # an LTI design: the message names almpc_certificate
    p = mo.double_integrator(N=N)
    sv.close()
    sv = capi.Solver(2, 1, N, 4)
    sv.set_keep_stage_models(True)
    sv.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    sv.update_initialization(np.ones((4, 2))); sv.calculate()
    assert _code(capi, lambda: sv.certificate_ltv(("cost",))) == ERR_UNSUPPORTED and "almpc_certificate" in message(sv)
    assert _code(capi, lambda: sv.relin_fnn_certificate(("cost",))) == ERR_UNSUPPORTED and message(sv)
    sv.close()
    # state box, terminal equality: the cost and the states
    for kw in (dict(xmin=[-50.0] * n, xmax=[50.0] * n), dict(terminal="equality")):
        sv = capi.Solver(n, m, N, 4)
        sv.design_ltv(*design_args(a), keep_stage_models=True, **kw)
        sv.update_initialization(X0); sv.calculate()
        for want in ("res", "grad", "costate", ALL, ("cost", "res")):
            assert _code(capi, lambda: sv.certificate_ltv(want)) == ERR_UNSUPPORTED and message(sv)
        cert, res = sv.certificate_ltv(("cost", "x", "e_x")), sv.get_results(want=("u", "e_u"))
        compare(str(kw), cert, reference(a, res), keys=("cost", "x", "e_x"))
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
    sv.set_keep_stage_models(True)
    sv.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act)
    sv.sqp_fnn_start(x0)
    sv.sqp_fnn_iterate(1)
    assert _code(capi, lambda: sv.certificate_ltv(("cost",))) == ERR_UNSUPPORTED and message(sv)
    assert _code(capi, lambda: sv.relin_fnn_certificate(("cost",))) == ERR_UNSUPPORTED and message(sv)
    sv.close()
    sv = capi.Solver(n, m, N, 4)
    assert sv.L.almpc_relin_fnn_certificate(sv.h, 1) == ERR_NOT_DESIGNED and message(sv)
    sv.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act)
    sv.update_initialization(x0)
    assert sv.L.almpc_relin_fnn_certificate(sv.h, 1) == ERR_INVALID and message(sv)   # before a step
    sv.relin_fnn_step()
    assert sv.L.almpc_relin_fnn_certificate(sv.h, 0) == ERR_INVALID and sv.L.almpc_relin_fnn_certificate(sv.h, 16) == ERR_INVALID
    assert _code(capi, lambda: sv.certificate_ltv(("cost",))) == ERR_UNSUPPORTED and message(sv)
    assert _code(capi, lambda: sv.certificate(("cost",))) == ERR_UNSUPPORTED   # almpc_certificate still refuses the pipeline
    sv.relin_fnn_certificate()
    sv.relin_fnn_step()
    assert sv.L.almpc_get_certificate(sv.h, cost.ctypes.data_as(_dp), None, None, None) == ERR_INVALID
    sv.close()
    # the pipeline with a state box: the cost alone
    sv = capi.Solver(n, m, N, 4)
    sv.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act=f.act, xmin=[-50.0] * n, xmax=[50.0] * n)
    sv.update_initialization(x0)
    sv.relin_fnn_step()
    assert _code(capi, lambda: sv.relin_fnn_certificate(("cost", "res"))) == ERR_UNSUPPORTED and message(sv)
    assert sv.relin_fnn_certificate(("cost",))["cost"].shape == (4,)
    sv.close()


def test_the_outer_loop_closes_on_the_devices_outputs(capi, mo):
    """The Fnn SQP loop of tests/test_gpu_ltv.py at b = 8, N = 20 with xbar <- x of certificate_ltv instead of the host rollout of the
    linearised dynamics, the stopping quantities from res and max|c|; its convergence assertions; at the end x is the host rollout
    within the restatement's bound."""
    f = mo.synthetic_fnn(act="tanh")
    b, n, m, N = 8, 4, 2, 20
    x_ref = np.tile(np.array([0.2, -0.1, 0.05, 0.0])[:, None], (1, N + 1)); u_ref = np.tile(np.array([0.1, -0.2])[:, None], (1, N))
    X0 = x_ref[:, 0][None, :] + 0.6 * mo.splitmix_normal(0x5EED0005, 0, b, n)
    Q, R, P = 100.0 * np.eye(n), 0.1 * np.eye(m), 150.0 * np.eye(n)
    umin, umax = -np.ones(m), np.ones(m)
    xbar = np.repeat(X0[:, :, None], N + 1, axis=2)
    ubar = np.repeat(u_ref[None], b, axis=0).copy()
    s = capi.Solver(n, m, N, b)
    s.set_keep_stage_models(True)
    hist = []
    for it in range(16):
        pts_x = xbar[:, :, :N].transpose(0, 2, 1).reshape(b * N, n); pts_u = ubar.transpose(0, 2, 1).reshape(b * N, m)
        A, B, fx = capi.fnn_linearize(f.W_in, f.W_h, f.b_h, f.W_out, pts_x, pts_u, act=f.act, want_f=True)
        A_all, B_all = A.reshape(b, N, n, n), B.reshape(b, N, n, m)
        c_all = fx.reshape(b, N, n) - xbar[:, :, 1:].transpose(0, 2, 1)
        s.design_ltv(A_all, B_all, c_all, xbar, ubar, x_ref, u_ref, Q, R, None, P, umin, umax)
        s.update_initialization(X0)
        s.calculate()
        r = s.get_results(want=("u", "e_u", "status"))
        assert np.all(r["status"] == 0)
        cert = s.certificate_ltv(("cost", "res", "grad", "x", "e_x"))
        V = r["e_u"]
        gmax = np.abs(cert["grad"]).reshape(b, -1).max(axis=1)
        assert np.all(cert["res"] <= 1e-9 * np.maximum(1.0, gmax)), (it, cert["res"])
        hist.append((float(np.abs(V).max()), float(np.abs(c_all).max()), float(np.max(cert["res"] / np.maximum(1.0, gmax)))))
        last = dict(A_all=A_all, B_all=B_all, c_all=c_all, xbar=xbar, ubar=ubar, x_ref=x_ref, u_ref=u_ref, Q=Q, R=R, S=None, P=P, umin=umin, umax=umax)
        xbar, ubar = cert["x"].copy(), r["u"].copy()
        assert np.all(ubar <= 1 + 1e-9) and np.all(ubar >= -1 - 1e-9)
    s.close()
    assert hist[-1][0] <= 1e-4 and hist[-1][1] <= 1e-9, hist
    assert hist[0][0] > 1e-2
    # the host rollout of the last iteration's linearised dynamics (what tests/test_gpu_ltv.py does every iteration)
    ref = reference(last, r)
    dx = np.zeros((b, n))
    xnew = last["xbar"].copy()
    for k in range(N):
        dx = np.einsum("bij,bj->bi", last["A_all"][:, k], dx) + np.einsum("bij,bj->bi", last["B_all"][:, k], V[:, :, k]) + last["c_all"][:, k]
        xnew[:, :, k + 1] = last["xbar"][:, :, k + 1] + dx
    for i in range(b):
        assert np.all(np.abs(cert["x"][i] - xnew[i]) <= ref[i]["tol_x"]), i


# ---------------------------------------------------------------------------- the re-linearisation pipeline
def _relin_reference(s, c, kw, res):
    out = []
    for i in range(c.batch):
        A, B = s.model_instance(i)
        P = np.array(s.terminal_weight_instance(i))
        out.append(cr.certificate(np.array(A), np.array(B), kw["Q"], kw["R"], None, P, kw["u_min"], kw["u_max"], res["e_x"][i], res["e_u"][i], res["u"][i]))
    return out


def _relin_steps(capi, c, make):
    """setup, a step, advance, a warm step: [(results, certificate, reference)] of both steps"""
    kw, X0 = nc.nlp_problem(c)
    f, ref = nc.model(c), nc.relin_reference(c)
    s = make()
    s.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], None, ref["P"], kw["u_min"], kw["u_max"],
                      act=c.act, net=c.kind)
    s.update_initialization(X0)
    out = []
    for opts in (capi.default_opts(), capi.default_opts(warm_start=1)):
        s.relin_fnn_step(opts)
        res, cert = s.get_results(), s.relin_fnn_certificate()
        out.append((res, cert, _relin_reference(s, c, kw, res)))
        if len(out) == 1:
            s.relin_fnn_advance()
    s.close()
    return out


def _compare4(name, cert, ref):
    worst = 0.0
    for i, k in enumerate(ref):
        for key in CERT4:
            err = np.abs(np.asarray(cert[key][i]) - k[key])
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.max(np.where(err == 0.0, 0.0, err / k["tol_" + key]))))
            assert np.all(err <= k["tol_" + key]), (name, i, key)
    return worst


@pytest.mark.parametrize("case", nc.RELIN, ids=lambda c: c.id)
def test_relin_certificate_is_the_certificate_of_the_steps_own_models(capi, case):
    steps = _relin_steps(capi, case, lambda: capi.Solver(case.n, case.m, case.N, case.batch))
    for which, (res, cert, ref) in zip(("cold", "warm"), steps):
        worst = _compare4(case.id, cert, ref)
        print(f"{case.id} {which}: worst error / bound {worst:.3f}; res max {cert['res'].max():.3e}; status {res['status']}")
        assert cert["grad"].shape == res["u"].shape and cert["costate"].shape == res["x"].shape


def test_relin_certificate_on_a_structured_handle_and_a_group(capi):
    case = nc.RELIN[3]
    steps = _relin_steps(capi, case, lambda: capi.Solver(case.n, case.m, case.N, case.batch, structured=True))
    for res, cert, ref in steps:
        print(f"{case.id} structured: worst error / bound {_compare4(case.id, cert, ref):.3f}")
    one = _relin_steps(capi, case, lambda: capi.Solver(case.n, case.m, case.N, case.batch))
    grp = _relin_steps(capi, case, lambda: capi.Group(case.n, case.m, case.N, case.batch, devices=[0, 0]))
    for (r1, c1, _), (rg, cg, _) in zip(one, grp):
        for k in ("e_x", "e_u", "u"):
            assert r1[k].tobytes() == rg[k].tobytes(), ("step", k)
        for k in CERT4:
            assert c1[k].tobytes() == cg[k].tobytes(), k
