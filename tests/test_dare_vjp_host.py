"""CPU checks of the adjoint of the DARE (tests/dare_vjp_ref.py, hm::dare_vjp through almpc_dare_vjp) and of the new surface.

1  The doubling restatement against central differences of scipy.linalg.solve_discrete_are with the loss sum(gP o P): shapes (1, 1),
   (2, 1), (4, 2), (12, 4) of tests/test_gpu_dare.py::random_models, three instances each, one direction per group (symmetric for Q
   and R; the R direction scaled by 0.01 so that R = 0.1 I stays positive definite), h = 1e-5, bound 1e-5 of max(1, |value|).
   Beyond (12, 4) the differences of scipy's DARE are too noisy to test against (3e-4 at (33, 3)).
2  The doubling restatement against the scipy-Lyapunov form on the nine shapes of tests/test_gpu_dare.py and on the slow-mode models
   (closed-loop radius 0.999, 0.9999), bound 1e-9 of max(1, max|group|); bad_model() with any P is status 3; the scalar model
   a = 2, b = q = r = 1 with the anti-stabilising root P = 2 - sqrt(5) (closed loop 2.618) is status 2, with 2 + sqrt(5) accepted.
3  almpc_dare_vjp (host) against the restatement on the same inputs and bound; the three status cases come back as
   ALMPC_ERR_NUMERIC with the status in the text; outputs that are NULL are skipped.  hm::dare_vjp also runs in a stand-alone
   program under ASan + UBSan (tests/sanitize/dare_vjp_driver.cpp).
4  End to end on the oracle: the problems of sens_params_cases.FD_CASES rebuilt with P = solve_discrete_are(A, B, Q, R); the gradient
   params_direct + dare_vjp(its P group) in Q, R, A, B against central differences of solve_box_qp_exact in which P is recomputed
   as the DARE at every perturbed Q, R, A, B; h = 1e-6, bound FD_RTOL = 1e-5, the face guard (MIN_MULT, MIN_GAP) of
   tests/test_sens_params_restatement.py on the solutions with the DARE's P.  Every case of FD_CASES passes the guard, none is left
   out.  The Q gradient must differ from the P-as-data one by more than the tolerance, so the chain is exercised.
5  The four symbols are in the header, in _capi's argtypes and in the Julia shim; almpc_param_grads keeps its fields.
"""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import dare_vjp_ref as dv
import sens_params_cases as pc
import sens_params_ref as pr
from test_gpu_dare import bad_model, random_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NUMERIC = -6
FD_SHAPES = [(1, 1), (2, 1), (4, 2), (12, 4)]
SHAPES = FD_SHAPES + [(16, 16), (17, 3), (32, 8), (33, 3), (48, 16)]
DARE_FD_H, DARE_FD_RTOL = 1e-5, 1e-5
FD_H, FD_RTOL = 1e-6, 1e-5
MIN_MULT, MIN_GAP = 1e-3, 1e-4
SQRT5 = np.sqrt(5.0)
SCALAR = tuple(np.array([[v]]) for v in (2.0, 1.0, 1.0, 1.0))   # a, b, q, r


def _instances(n, m, count=3):
    """(A, B, Q, R, P, gP) of `count` random models of a shape, P from scipy."""
    A, B, Q, R = random_models(n, m, count)
    rng = np.random.default_rng(2000 + n)
    return [(A[i], B[i], Q, R, sla.solve_discrete_are(A[i], B[i], Q, R), dv.random_symmetric(rng, n)) for i in range(count)]


def _slow(lam):
    A, B, Q, R = dv.slow_mode_model(lam)
    return A, B, Q, R, sla.solve_discrete_are(A, B, Q, R), dv.random_symmetric(np.random.default_rng(5), 4)


@pytest.mark.parametrize("n,m", FD_SHAPES)
def test_restatement_matches_differences_of_scipys_dare(n, m):
    rng = np.random.default_rng(3000 + n)
    worst = 0.0
    for A, B, Q, R, P, gP in _instances(n, m):
        st, got, _ = dv.dare_vjp_doubling(A, B, Q, R, P, gP)
        assert st == 0
        dirs = {"A": rng.standard_normal((n, n)), "B": rng.standard_normal((n, m)), "Q": dv.random_symmetric(rng, n),
                "R": 0.01 * dv.random_symmetric(rng, m)}
        for k, D in dirs.items():
            L = []
            for sgn in (1.0, -1.0):
                arg = dict(A=A, B=B, Q=Q, R=R)
                arg[k] = arg[k] + sgn * DARE_FD_H * D
                L.append(float((gP * sla.solve_discrete_are(arg["A"], arg["B"], arg["Q"], arg["R"])).sum()))
            fd = (L[0] - L[1]) / (2 * DARE_FD_H)
            val = float((got[k] * D).sum())
            worst = max(worst, abs(val - fd) / max(1.0, abs(val)))
    print(f"n {n} m {m}: worst error against central differences of scipy's DARE {worst:.2e}")
    assert worst <= DARE_FD_RTOL


def test_doubling_matches_the_lyapunov_form():
    for n, m in SHAPES:
        worst, steps = 0.0, []
        for A, B, Q, R, P, gP in _instances(n, m):
            st, got, it = dv.dare_vjp_doubling(A, B, Q, R, P, gP)
            assert st == 0
            worst = max(worst, dv.worst_gap(got, dv.dare_vjp_lyap(A, B, Q, R, P, gP))[0])
            steps.append(it)
            assert np.array_equal(got["Q"], got["Q"].T) and np.array_equal(got["R"], got["R"].T)
        print(f"n {n} m {m}: doublings {min(steps)} .. {max(steps)}, worst gap to the Lyapunov form {worst:.2e}")
        assert worst <= dv.RTOL
    for lam in (0.999, 0.9999):
        A, B, Q, R, P, gP = _slow(lam)
        st, got, it = dv.dare_vjp_doubling(A, B, Q, R, P, gP)
        gap = dv.worst_gap(got, dv.dare_vjp_lyap(A, B, Q, R, P, gP))[0]
        print(f"slow mode {lam}: {it} doublings, gap {gap:.2e}")
        assert st == 0 and gap <= dv.RTOL and it >= 14


def test_status_cases_of_the_restatement():
    Ab, Bb = bad_model()
    Q, R = 100.0 * np.eye(4), 0.1 * np.eye(2)
    for P in (np.eye(4), Q, 1e4 * dv.random_symmetric(np.random.default_rng(1), 4)):
        assert dv.dare_vjp_doubling(Ab, Bb, Q, R, P, np.eye(4))[0] == 3
    a, b, q, r = SCALAR
    for root, want in ((2.0 - SQRT5, 2), (2.0 + SQRT5, 0)):
        P = np.array([[root]])
        assert abs(float(pr_residual(a, b, q, r, P))) < 1e-12
        assert dv.dare_vjp_doubling(a, b, q, r, P, np.eye(1))[0] == want
    assert abs(float((a - b * dv.gain(a, b, r, np.array([[2.0 - SQRT5]])))[0, 0])) == pytest.approx(2.618, abs=1e-3)
    assert dv.dare_vjp_doubling(a, b, q, -b * (2.0 + SQRT5) * b, np.array([[2.0 + SQRT5]]), np.eye(1))[0] == 1   # R + B'PB == 0


def pr_residual(A, B, Q, R, P):
    K = dv.gain(A, B, R, P)
    return (A.T @ P @ A - P - A.T @ P @ B @ K + Q).max()


@pytest.mark.parametrize("n,m", SHAPES)
def test_host_entry_point_matches_the_restatement(capi, n, m):
    worst = 0.0
    for A, B, Q, R, P, gP in _instances(n, m):
        st, ref, _ = dv.dare_vjp_doubling(A, B, Q, R, P, gP)
        assert st == 0
        got = capi.dare_vjp(A, B, Q, R, P, gP)
        assert sorted(got) == ["A", "B", "Q", "R"]
        worst = max(worst, dv.worst_gap(got, ref)[0])
        assert np.array_equal(got["Q"], got["Q"].T) and np.array_equal(got["R"], got["R"].T)
    print(f"n {n} m {m}: almpc_dare_vjp against the restatement {worst:.2e}")
    assert worst <= dv.RTOL


def test_host_entry_point_slow_modes_statuses_and_null_outputs(capi):
    for lam in (0.999, 0.9999):
        A, B, Q, R, P, gP = _slow(lam)
        gap = dv.worst_gap(capi.dare_vjp(A, B, Q, R, P, gP), dv.dare_vjp_doubling(A, B, Q, R, P, gP)[1])[0]
        print(f"slow mode {lam}: almpc_dare_vjp against the restatement {gap:.2e}")
        assert gap <= dv.RTOL
    # the three statuses: ALMPC_ERR_NUMERIC, the status in the text, nothing written
    Ab, Bb = bad_model()
    a, b, q, r = SCALAR
    cases = [(3, (Ab, Bb, 100.0 * np.eye(4), 0.1 * np.eye(2), np.eye(4), np.eye(4))),
             (2, (a, b, q, r, np.array([[2.0 - SQRT5]]), np.eye(1))),
             (1, (a, b, q, -b * (2.0 + SQRT5) * b, np.array([[2.0 + SQRT5]]), np.eye(1)))]
    for status, args in cases:
        with pytest.raises(capi.AlmpcError) as e:
            capi.dare_vjp(*args)
        assert e.value.code == ERR_NUMERIC and f"status {status}" in str(e.value), e.value
    got = capi.dare_vjp(a, b, q, r, np.array([[2.0 + SQRT5]]), np.eye(1))
    assert dv.worst_gap(got, dv.dare_vjp_doubling(a, b, q, r, np.array([[2.0 + SQRT5]]), np.eye(1))[1])[0] <= dv.RTOL
    # a failing call leaves the caller's arrays alone
    L = capi.load()
    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    sent = [np.full(1, -12345.678) for _ in range(4)]
    P_bad, one = np.array([2.0 - SQRT5]), np.ones(1)
    assert L.almpc_dare_vjp(1, 1, dp(a), dp(b), dp(q), dp(r), dp(P_bad), dp(one), *(dp(s) for s in sent)) == ERR_NUMERIC
    assert all(s[0] == -12345.678 for s in sent)
    assert b"status 2" in L.almpc_last_error(None)
    # outputs that are NULL are skipped; the others have the bits of the full call
    A, B, Q, R, P, gP = _instances(4, 2, 1)[0]
    full = capi.dare_vjp(A, B, Q, R, P, gP)
    for want in (("Q",), ("A", "R"), ("B",)):
        part = capi.dare_vjp(A, B, Q, R, P, gP, want=want)
        assert sorted(part) == sorted(want)
        for k in want:
            assert part[k].tobytes() == full[k].tobytes(), k
    assert L.almpc_dare_vjp(4, 2, None, None, None, None, None, None, None, None, None, None) == -1


def test_host_dare_vjp_under_asan_ubsan(tmp_path):
    """hm::dare_vjp in a stand-alone program (tests/sanitize/dare_vjp_driver.cpp) under ASan + UBSan: a clean exit on an accepted
    instance of (12, 4) and on the three refusals, and the regular build's numbers."""
    import subprocess
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    exe = str(tmp_path / "dare_vjp_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + san + ["-o", exe, os.path.join(ROOT, "tests", "sanitize", "dare_vjp_driver.cpp")])
    Ab, Bb = bad_model()
    a, b, q, r = SCALAR
    cases = [(0, _instances(12, 4, 1)[0]), (3, (Ab, Bb, 100.0 * np.eye(4), 0.1 * np.eye(2), np.eye(4), np.eye(4))),
             (2, (a, b, q, r, np.array([[2.0 - SQRT5]]), np.eye(1))), (1, (a, b, q, -b * (2.0 + SQRT5) * b, np.array([[2.0 + SQRT5]]), np.eye(1)))]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for k, (status, mats) in enumerate(cases):
        n, m = mats[1].shape
        with open(tmp_path / f"in{k}.txt", "w") as fo:
            fo.write(f"{n} {m}\n")
            for M in mats:
                fo.write(" ".join(repr(float(v)) for v in np.asarray(M).flatten(order="F")) + "\n")
        res = subprocess.run([exe, str(tmp_path / f"in{k}.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stderr[-3000:]
        assert "ERROR" not in res.stderr and "runtime error" not in res.stderr
        vals = res.stdout.split()
        assert int(vals[0]) == status
        if status == 0:
            ref = dv.dare_vjp_doubling(*mats)[1]
            flat = np.array([float(v) for v in vals[1:]])
            got, at = {}, 0
            for g, shape in (("A", (n, n)), ("B", (n, m)), ("Q", (n, n)), ("R", (m, m))):
                got[g] = flat[at:at + shape[0] * shape[1]].reshape(shape, order="F")
                at += shape[0] * shape[1]
            assert at == flat.size and dv.worst_gap(got, ref)[0] <= dv.RTOL


def _solve(mo, p, x0):
    H, f, lo, hi = mo.condensed_qp(p, x0)
    v = mo.solve_box_qp_exact(H, f, lo, hi)
    return mo.rollout(p, x0, v), (H, f, lo, hi, v)


def _with_dare(p, **change):
    q = dataclasses.replace(p, **change)
    return dataclasses.replace(q, P=sla.solve_discrete_are(q.A, q.B, q.Q, q.R))


@pytest.mark.parametrize("name", pc.FD_CASES)
def test_end_to_end_against_differences_with_the_dare_recomputed(mo, name):
    p0, X0 = pc.case(mo, name)
    p = _with_dare(p0)
    _, _, H, F = mo.condense(p)
    d = mo.jacobi_scaling(H)
    rng = np.random.default_rng(83)
    sym = lambda M: 0.5 * (M + M.T)
    worst, min_mult, min_gap, rows, q_shift = {}, np.inf, np.inf, [], 0.0
    for x0 in X0:
        res, (Hq, f, lo, hi, v) = _solve(mo, p, x0)
        act, lower = pr.sides(res["u"], p.u_min, p.u_max, d)
        g = Hq @ v + f
        mult, gap = np.where(lower, g, -g)[act], np.minimum(v - lo, hi - v)[~act]
        min_mult = min(min_mult, mult.min() if mult.size else np.inf)
        min_gap = min(min_gap, gap.min() if gap.size else np.inf)
        rows.append(int(act.sum()))
        g_u, g_x = pc.loss(rng, p)
        data = pr.params_direct(pr.prob_of(p), H, F, act, lower, res, g_u, g_x)
        chain = dv.dare_vjp_lyap(p.A, p.B, p.Q, p.R, p.P, data["P"])
        got = {k: data[k] + chain[k] for k in dv.GROUPS}
        q_shift = max(q_shift, float(np.abs(chain["Q"]).max()) / max(1.0, float(np.abs(data["Q"]).max())))
        n, m = p.n, p.m
        for _ in range(3):
            for k, D in (("Q", sym(rng.normal(size=(n, n)))), ("R", sym(rng.normal(size=(m, m)))), ("A", rng.normal(size=(n, n))),
                         ("B", rng.normal(size=(n, m)))):
                L = []
                for sgn in (1.0, -1.0):
                    r, _ = _solve(mo, _with_dare(p, **{k: getattr(p, k) + sgn * FD_H * D}), x0)
                    L.append(float((g_u * r["u"]).sum() + (g_x * r["x"]).sum()))
                fd = (L[0] - L[1]) / (2 * FD_H)
                val = float((got[k] * D).sum())
                worst[k] = max(worst.get(k, 0.0), abs(val - fd) / max(1.0, abs(val)))
    print(f"{name}: rows {min(rows)} .. {max(rows)}, smallest multiplier {min_mult:.3g}, smallest gap {min_gap:.3g}; worst error against "
          "central differences with the DARE recomputed: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items())
          + f"; the DARE's share of dL/dQ {q_shift:.2e}")
    assert min_mult >= MIN_MULT and min_gap >= MIN_GAP, (name, min_mult, min_gap)
    assert max(worst.values()) <= FD_RTOL, worst
    assert q_shift > FD_RTOL


NAMES = ("almpc_dare_vjp", "almpc_dare_vjp_batched", "almpc_sensitivity_params_vjp_dare", "almpc_group_sensitivity_params_vjp_dare")


def test_header_and_bindings_carry_the_dare_adjoint(pkg):
    header = open(os.path.join(ROOT, "include", "almpc.h")).read()
    declared = set(re.findall(r"\b(almpc_[a-z0-9_]+)\s*\(", header))
    assert not [n for n in NAMES if n not in declared]
    capi = pkg._capi
    for cls in (capi.Solver, capi.Group):
        assert "terminal" in cls.sensitivity_params_vjp.__code__.co_varnames
    assert callable(capi.dare_vjp) and callable(capi.dare_vjp_batched)
    assert not [n for n in NAMES if n not in capi.prototypes()]
    shim = open(os.path.join(ROOT, "julia", "AlmpcHIP.jl")).read()
    assert not [n for n in NAMES if ("(:" + n + ", libalmpc)") not in shim]
    body = re.search(r"typedef struct almpc_param_grads \{(.*?)\} almpc_param_grads;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in capi.almpc_param_grads._fields_] == ["x0", "f", "u_ref", "u_min", "u_max", "Q", "P", "A", "R", "S", "B", "rows"]
    controller = __import__("importlib").import_module(pkg.__name__ + ".controller")
    assert "terminal" in controller.sensitivity_params.__code__.co_varnames
    with pytest.raises(ValueError):
        capi._terminal_gradient("riccati")
