"""The per-instance-weight design (almpc_design_batched_weighted) on an MI355X: pytest -m gpu.  Cases: tests/weighted_design_cases.py.

1  a batch of equal weight sets gives the bits of almpc_design_batched (H_i, F_i, d_i, P_i, a step), P given and P = NULL in both
   terminal-weight modes;
2  distinct weights against the oracle of every instance's own problem, with the tolerances of tests/test_gpu_instance_step_shapes.py
   (1e-11 of max|H|, max|F|; U_TOL, 10 X_TOL), and almpc_get_weights_instance;
3  permuted instances give permuted bits;
4  one instance's weight moves that instance alone, and the loss of that instance follows almpc_sensitivity_params_vjp's g_Q, g_R,
   g_S (central differences, h and bound of tests/test_gpu_sensitivity_params.py);
5  almpc_sensitivity_params_vjp against tests/sens_params_ref.py with each instance's own weights (ten times the CPU gap of the case),
   almpc_sensitivity_params_vjp_dare against tests/dare_vjp_ref.py (that plus dare_vjp_ref.RTOL), g_x0 = almpc_sensitivity_vjp's bits;
6  P = NULL against almpc_dare of every instance's own (A_i, B_i, Q_i, R_i) (P_RTOL of tests/test_gpu_dare.py);
7  state box and terminal equality against the exact oracle (the tolerances of tests/test_gpu_state_rows_instances.py);
8  refusals, no redo under the default, and the way back to shared weights;
9  a group over [0, 0] equals one handle.

Lines that start with `weighted` print the measured figures (pytest -s)."""
import numpy as np
import pytest

import dare_vjp_ref as dv
import instance_step_cases as ic
import sens_params_ref as pr
import weighted_design_cases as wc
from test_gpu_dare import P_RTOL, bad_model

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_NOT_DESIGNED, ERR_NUMERIC = -1, -4, -5, -6
U_TOL, X_TOL = 1e-6, 1e-5                     # tests/test_gpu_instance_step_shapes.py
ROWS_U_TOL, ROWS_X_TOL = 1e-6, 1e-6           # tests/test_gpu_state_rows_instances.py
FD_H, FD_RTOL = 1e-6, 1e-5                    # tests/test_gpu_sensitivity_params.py
KEYS = ("u", "e_u", "x", "e_x", "status", "iters", "polish_iters")
CHAINED = ("Q", "R", "A", "B")
MODES = ("given", "null_host", "null_device")
_ids = lambda c: c.id


def _note(what, key, value, bound=None):
    print("weighted %s %s %.3e%s" % (what, key, value, "" if bound is None else " of %.1e" % bound))


def _handle(capi, c, monkeypatch, env=(), make=None, **kw):
    with monkeypatch.context() as mp:
        for k, v in dict(env).items():
            mp.setenv(k, v)
        return (make or capi.Solver)(c.n, c.m, c.N, c.batch, **kw)


def _terminal(s, mode):
    if mode != "given":
        s.set_terminal_weight("dare_device" if mode == "null_device" else "given")


def _weighted(capi, c, monkeypatch, Q, R, S, mode="given", order=None, env=(), **kw):
    """a handle designed on the case's models with the given weight sets, instances in `order`"""
    s = _handle(capi, c, monkeypatch, env, **kw)
    A, B = ic.models(c.base)
    t = ic.template(c.base)
    idx = np.arange(c.batch) if order is None else order
    P = None
    if mode == "given":
        P = wc.terminal(c)
        P = P if P.ndim == 2 else P[idx]
    _terminal(s, mode)
    s.design_batched_weighted(A[idx], B[idx], Q[idx], R[idx], None if S is None else S[idx], P, t.u_min, t.u_max)
    s.set_reference(t.x_ref, t.u_ref)
    return s


def _shared(capi, c, monkeypatch, Q, R, S, mode="given", env=(), **kw):
    s = _handle(capi, c, monkeypatch, env, **kw)
    A, B = ic.models(c.base)
    t = ic.template(c.base)
    _terminal(s, mode)
    s.design_batched(A, B, Q, R, S, wc.terminal(c) if mode == "given" else None, t.u_min, t.u_max)
    s.set_reference(t.x_ref, t.u_ref)
    return s


def _step(s, X0, opts=None):
    s.update_initialization(X0)
    s.calculate(opts)
    return s.get_results()


def _design(s):
    out = []
    for i in range(s.batch):
        g = s.get_design_instance(i)
        g["P"] = s.terminal_weight_instance(i)
        out.append(g)
    return out


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_designs(a, b, what, rows=None):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if rows is not None and i not in rows:
            continue
        for k in ("H", "F", "d", "P"):
            assert _bits(x[k], y[k]), (what, i, k)


def _same_results(a, b, what, rows=None):
    for k in KEYS:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert _bits(x, y), (what, k)


def _replicated(c, i=0):
    Q, R, S = wc.weights(c)
    rep = lambda M: None if M is None else np.repeat(M[i:i + 1], c.batch, axis=0)
    return (Q[i], R[i], None if S is None else S[i]), (rep(Q), rep(R), rep(S))


# ---------------------------------------------------------------------------- 1. replicated weights are shared weights
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", wc.CASES, ids=_ids)
def test_replicated_weights_give_the_bits_of_the_shared_design(capi, case, mode, monkeypatch):
    one, many = _replicated(case)
    X0 = wc.x0(case)
    for env in ({},) + (case.envs if mode == "given" else ()):
        a = _shared(capi, case, monkeypatch, *one, mode=mode, env=env)
        b = _weighted(capi, case, monkeypatch, *many, mode=mode, env=env)
        what = (case.id, mode, ic._env_id(env))
        _same_designs(_design(a), _design(b), what)
        ra, rb = _step(a, X0), _step(b, X0)
        _same_results(ra, rb, what)
        assert np.isfinite(ra["u"]).all()
        a.close(); b.close()


# ---------------------------------------------------------------------------- 2. distinct weights against the oracle
@pytest.mark.parametrize("case", wc.CASES, ids=_ids)
def test_distinct_weights_against_the_oracle_of_every_instance(capi, case, monkeypatch):
    Q, R, S = wc.weights(case)
    ref = wc.reference(case)
    for env in ({},) + case.envs:
        s = _weighted(capi, case, monkeypatch, Q, R, S, env=env, structured_fallback=False)
        eh = ef = 0.0
        for i, (H, F) in enumerate(wc.condensed(case)):
            g = s.get_design_instance(i)
            eh = max(eh, float(np.abs(g["H"] - H).max() / np.abs(H).max()))
            ef = max(ef, float(np.abs(g["F"] - F).max() / np.abs(F).max()))
            w = s.get_weights_instance(i)
            assert np.array_equal(w["Q"], Q[i]) and np.array_equal(w["R"], R[i]), i
            assert np.array_equal(w["S"], np.zeros((case.m, case.m)) if S is None else S[i]), i
        r = _step(s, ref["X0"])
        s.close()
        who = "%s %s" % (case.id, ic._env_id(env))
        _note("design-H", who, eh, 1e-11)
        _note("design-F", who, ef, 1e-11)
        assert eh <= 1e-11 and ef <= 1e-11, (who, eh, ef)
        assert np.all(r["status"] == 0), (who, np.nonzero(r["status"])[0].tolist())
        eu = max(float(np.abs(r["u"][i] - e["u"]).max()) for i, e in enumerate(ref["exact"]))
        ex = max(float(np.abs(r["x"][i] - e["x"]).max()) for i, e in enumerate(ref["exact"]))
        _note("exact-u", who, eu, U_TOL)
        _note("exact-x", who, ex, 10 * X_TOL)
        assert eu <= U_TOL and ex <= 10 * X_TOL, (who, eu, ex)


# ---------------------------------------------------------------------------- 3. permutation
@pytest.mark.parametrize("case", wc.CASES, ids=_ids)
def test_permuted_instances_give_permuted_bits(capi, case, monkeypatch):
    Q, R, S = wc.weights(case)
    X0 = wc.x0(case)
    order = np.random.default_rng(5 + case.N).permutation(case.batch)
    assert not np.array_equal(order, np.arange(case.batch))
    a = _weighted(capi, case, monkeypatch, Q, R, S)
    b = _weighted(capi, case, monkeypatch, Q, R, S, order=order)
    da, db = _design(a), _design(b)
    _same_designs([da[j] for j in order], db, (case.id, "permuted"))
    ra, rb = _step(a, X0), _step(b, X0[order])
    a.close(); b.close()
    for k in KEYS:
        assert _bits(ra[k][order], rb[k]), (case.id, k)
    assert np.all(ra["status"] == 0)


# ---------------------------------------------------------------------------- 4. one instance's weight moves one instance
def _loss_of(r, j, g_u, g_x):
    return float((g_u[j] * r["u"][j]).sum() + (g_x[j] * r["x"][j]).sum())


def _moved_instance(case):
    """an instance whose exact solution has rows on a bound and free rows: its gradients see both kinds"""
    ref = wc.reference(case)
    rows = [wc.active_rows(wc.problem(case, i), ref["exact"][i]["u"]) for i in range(case.batch)]
    return next(i for i in range(3, case.batch) if 2 <= rows[i] <= case.m * case.N - 2)


@pytest.mark.parametrize("case", wc.tagged("fd") + (wc.CASE_BY_ID["16-1-59"],), ids=_ids)
def test_one_instances_weight_moves_one_instance(capi, case, monkeypatch):
    Q, R, S = wc.weights(case)
    X0 = wc.x0(case)
    j = _moved_instance(case)
    others = [i for i in range(case.batch) if i != j]
    a = _weighted(capi, case, monkeypatch, Q, R, S)
    Q2 = Q.copy()
    Q2[j] = Q[j] * 1.25
    b = _weighted(capi, case, monkeypatch, Q2, R, S)
    da, db = _design(a), _design(b)
    _same_designs(da, db, (case.id, "others"), rows=set(others))
    assert not _bits(da[j]["H"], db[j]["H"]) and not _bits(da[j]["F"], db[j]["F"])
    ra, rb = _step(a, X0), _step(b, X0)
    a.close(); b.close()
    _same_results(ra, rb, (case.id, "others"), rows=others)
    assert not _bits(ra["u"][j], rb["u"][j])


@pytest.mark.parametrize("case", wc.tagged("fd"), ids=_ids)
def test_the_loss_of_one_instance_follows_its_weight_gradients(capi, case, monkeypatch):
    """the change of instance j's loss under W_j + h E against h <g_W[j], E>, W = Q, R, S, E symmetric, central differences of the
    device's own designs and steps with h = 1e-6: bound 1e-5 of max(1, |value|)"""
    Q, R, S = wc.weights(case)
    X0 = wc.x0(case)
    j = _moved_instance(case)
    g_u, g_x = wc.loss(case, 47)
    s = _weighted(capi, case, monkeypatch, Q, R, S)
    r0 = _step(s, X0)
    assert np.all(r0["status"] == 0)
    got = s.sensitivity_params_vjp(g_u, g_x, want=("Q", "R", "S"))
    s.close()
    rng = np.random.default_rng(53)
    sym = lambda M: 0.5 * (M + M.T)
    W = {"Q": Q, "R": R, "S": S}
    worst = {}
    for k in ("Q", "R") + (("S",) if S is not None else ()):
        E = sym(rng.normal(size=W[k].shape[1:]))
        L = []
        for sgn in (1.0, -1.0):
            W2 = dict(W)
            W2[k] = W[k].copy()
            W2[k][j] = W[k][j] + sgn * FD_H * E
            s2 = _weighted(capi, case, monkeypatch, W2["Q"], W2["R"], W2["S"])
            r = _step(s2, X0)
            s2.close()
            assert np.all(r["status"] == 0)
            L.append(_loss_of(r, j, g_u, g_x))
        fd = (L[0] - L[1]) / (2 * FD_H)
        val = float((got[k][j] * E).sum())
        worst[k] = abs(val - fd) / max(1.0, abs(val))
        print("weighted fd %s instance %d dL/d%s . E: %.9g, central differences of the device's steps %.9g, error %.2e of %.1e"
              % (case.id, j, k, val, fd, worst[k], FD_RTOL))
        assert abs(val) > 1e-6, (k, val)
    assert max(worst.values()) <= FD_RTOL, worst


# ---------------------------------------------------------------------------- 5. the parameter gradients against the restatements
@pytest.mark.parametrize("mode", ("null_host", "null_device"))
@pytest.mark.parametrize("case", wc.tagged("sens"), ids=_ids)
def test_parameter_gradients_against_the_restatements(capi, mo, case, mode, monkeypatch):
    Q, R, S = wc.weights(case)
    X0 = wc.x0(case)
    s = _weighted(capi, case, monkeypatch, Q, R, S, mode=mode)     # P = NULL: P_i = DARE(A_i, B_i, Q_i, R_i)
    res = _step(s, X0)
    assert np.all(res["status"] == 0), np.nonzero(res["status"])[0].tolist()
    g_u, g_x = wc.loss(case)
    data = s.sensitivity_params_vjp(g_u, g_x)
    dare = s.sensitivity_params_vjp(g_u, g_x, terminal="dare")
    g_x0, vrows = s.sensitivity_vjp(g_u, g_x)
    assert _bits(data["x0"], g_x0) and np.array_equal(data["rows"], vrows)
    assert np.all(dare["dare_status"] == 0), dare["dare_status"]
    for k in [k for k in pr.GROUPS if k not in CHAINED] + ["rows"]:
        assert _bits(data[k], dare[k]), k
    worst = dict.fromkeys(pr.GROUPS, 0.0)
    chain = dict.fromkeys(CHAINED, 0.0)
    rows = []
    for i in range(case.batch):
        g = s.get_design_instance(i)
        P = s.terminal_weight_instance(i)
        p = wc.problem_with(case, i, Q[i], R[i], None if S is None else S[i], P=P)
        r = {k: res[k][i] for k in ("u", "e_u", "e_x")}
        act, lower = pr.sides(r["u"], p.u_min, p.u_max, g["d"])
        rows.append(int(act.sum()))
        assert data["rows"][i] == rows[-1], (i, data["rows"][i], rows[-1])
        ref = pr.params_direct(pr.prob_of(p), g["H"], g["F"], act, lower, r, g_u[i], g_x[i])
        for k, e in pr.worst_gaps({k: data[k][i] for k in pr.GROUPS}, ref).items():
            worst[k] = max(worst[k], e)
        A, B = s.model_instance(i)
        lyap = dv.dare_vjp_lyap(A, B, Q[i], R[i], P, data["P"][i])
        for k in CHAINED:
            want = data[k][i] + lyap[k]
            chain[k] = max(chain[k], float(np.abs(dare[k][i] - want).max()) / pr.group_scale(want))
    s.close()
    tol = wc.gpu_tol(case.id)
    print("weighted params %s %s: rows %d .. %d; worst error per group: " % (case.id, mode, min(rows), max(rows))
          + ", ".join("%s %.1e" % kv for kv in worst.items()) + "; tolerance %g" % tol)
    print("weighted params-dare %s %s: worst error of the chained groups: " % (case.id, mode)
          + ", ".join("%s %.1e" % kv for kv in chain.items()) + "; tolerance %g" % (tol + dv.RTOL))
    assert max(rows) > 0 and np.abs(data["Q"]).max() > 0 and np.abs(data["R"]).max() > 0
    if S is not None:
        assert np.abs(data["S"]).max() > 0
    assert max(worst.values()) <= tol, worst
    assert max(chain.values()) <= tol + dv.RTOL, chain


# ---------------------------------------------------------------------------- 6. P = NULL
@pytest.mark.parametrize("mode", ("null_host", "null_device"))
@pytest.mark.parametrize("case", wc.tagged("null_p"), ids=_ids)
def test_null_p_is_every_instances_own_dare(capi, case, mode, monkeypatch):
    Q, R, S = wc.weights(case)
    A, B = ic.models(case.base)
    s = _weighted(capi, case, monkeypatch, Q, R, S, mode=mode)
    worst = 0.0
    for i in range(case.batch):
        want = capi.dare(A[i], B[i], Q[i], R[i])
        worst = max(worst, float(np.abs(s.terminal_weight_instance(i) - want).max() / np.abs(want).max()))
    s.close()
    _note("dare", "%s %s" % (case.id, mode), worst, P_RTOL)
    assert worst <= P_RTOL


@pytest.mark.parametrize("mode", ("null_host", "null_device"))
def test_an_instance_without_a_stabilising_solution_is_reported(capi, mode):
    rng = np.random.default_rng(3)
    b, n, m = 24, 4, 2
    A = 0.3 * rng.standard_normal((b, n, n))
    B = rng.standard_normal((b, n, m))
    A[5], B[5] = bad_model()
    Q, R, _ = wc._weights(5, b, n, m, False)
    s = capi.Solver(n, m, 10, b)
    _terminal(s, mode)
    with pytest.raises(capi.AlmpcError) as e:
        s.design_batched_weighted(A, B, Q, R, None, None, [-1.0, -1.0], [1.0, 1.0])
    assert e.value.code == ERR_NUMERIC and "instance 5" in str(e.value), e.value
    s.close()


# ---------------------------------------------------------------------------- 7. state rows
@pytest.mark.parametrize("kind", wc.ROWS_CASES)
def test_state_rows_against_the_exact_oracle(capi, kind):
    A, B, Q, R, S, X0 = wc.rows_family()
    ref = wc.rows_reference(kind)
    s = capi.Solver(2, 1, wc.ROWS_N, wc.ROWS_BATCH)
    box = kind == "box"
    s.design_batched_weighted(A, B, Q, R, S, None, [-1.0], [1.0], xmin=wc.ROWS_XMIN if box else None, xmax=wc.ROWS_XMAX if box else None,
                              terminal="none" if box else "equality")
    r = _step(s, X0)
    s.close()
    assert np.all(r["status"] == 0), np.nonzero(r["status"])[0].tolist()
    eu = ex = 0.0
    for i, e in enumerate(ref):
        eu = max(eu, float(np.abs(r["u"][i] - e["u"]).max()))
        ex = max(ex, float(np.abs(r["x"][i] - e["x"]).max() / max(1.0, np.abs(e["x"]).max())))
        if box:
            assert np.all(r["x"][i] <= wc.ROWS_XMAX[:, None] + 1e-9) and np.all(r["x"][i] >= wc.ROWS_XMIN[:, None] - 1e-9), i
        else:
            assert np.abs(r["e_x"][i][:, -1]).max() <= 1e-9, i
    _note("rows-u", kind, eu, ROWS_U_TOL)
    _note("rows-x", kind, ex, ROWS_X_TOL)
    assert eu <= ROWS_U_TOL and ex <= ROWS_X_TOL


# ---------------------------------------------------------------------------- 8. refusals and the way back
def _refused(capi, call, code, text=None):
    with pytest.raises(capi.AlmpcError) as e:
        call()
    assert e.value.code == code, e.value
    assert str(e.value).split(":", 1)[1].strip()
    if text:
        assert text in str(e.value), e.value


def test_refusals(capi, monkeypatch):
    c = wc.CASE_BY_ID["3-2-6-s"]
    Q, R, S = wc.weights(c)
    A, B = ic.models(c.base)
    t = ic.template(c.base)
    P = wc.terminal(c)
    args = lambda Q=Q, R=R, S=S: (A, B, Q, R, S, P, t.u_min, t.u_max)
    s = capi.Solver(c.n, c.m, c.N, c.batch)
    # the branch is one for the batch: the lowest instance that leaves instance 0's is named
    R2 = R.copy(); R2[7, 0, 0] = 0.0; R2[20, 0, 0] = 0.0
    _refused(capi, lambda: s.design_batched_weighted(*args(R=R2)), ERR_INVALID, "instance 7")
    S2 = S.copy(); S2[9, 0, 0] = 0.0
    _refused(capi, lambda: s.design_batched_weighted(*args(S=S2)), ERR_INVALID, "instance 9")
    R3 = R.copy(); R3[0, 0, 0] = 0.0
    _refused(capi, lambda: s.design_batched_weighted(*args(R=R3)), ERR_INVALID, "instance 1")
    # NULL pointers
    dp = lambda M: None if M is None else np.ascontiguousarray(M, dtype=np.float64).ctypes.data_as(capi._dp)
    um, ux = np.array(t.u_min, dtype=np.float64), np.array(t.u_max, dtype=np.float64)
    full = [A, B, Q, R, S, P[0], um, ux]
    for missing in (0, 1, 2, 3, 6, 7):
        a = [None if k == missing else dp(M) for k, M in enumerate(full)]
        assert s.L.almpc_design_batched_weighted(s.h, *a[:6], 0, a[6], a[7], 0.1, 1e-6) == ERR_INVALID, missing
        assert (s.L.almpc_last_error(s.h) or b"").decode().strip()
    assert s.L.almpc_design_batched_weighted(None, *[dp(M) for M in full[:6]], 0, dp(um), dp(ux), 0.1, 1e-6) == ERR_INVALID
    _refused(capi, lambda: s.get_weights_instance(0), ERR_NOT_DESIGNED)      # before a design
    s.design_batched_weighted(*args())
    _refused(capi, lambda: s.get_weights_instance(c.batch), ERR_INVALID)
    s.close()
    # a structured handle; the redo asked for
    s = capi.Solver(c.n, c.m, c.N, c.batch, structured=True)
    _refused(capi, lambda: s.design_batched_weighted(*args()), ERR_UNSUPPORTED, "STRUCTURED")
    s.close()
    s = capi.Solver(c.n, c.m, c.N, c.batch, structured_fallback=True)
    _refused(capi, lambda: s.design_batched_weighted(*args()), ERR_UNSUPPORTED, "fallback")
    s.design_batched(A, B, Q[0], R[0], S[0], P, t.u_min, t.u_max)     # (the handle itself is fine)
    s.close()


def test_no_redo_follows_a_step_under_the_default(capi, monkeypatch):
    """polish_max_iter = 1 leaves instances with ALMPC_MAX_ITER: on almpc_design_batched the default redo solves them, on the
    weighted design of the same problems they keep their status, and the results are those of a handle with the redo off"""
    c = wc.CASE_BY_ID["4-2-16"]
    one, many = _replicated(c)
    X0 = 3.0 * wc.x0(c)
    o = capi.default_opts(polish_max_iter=1)
    a = _shared(capi, c, monkeypatch, *one)
    ra = _step(a, X0, o)
    a.close()
    b = _weighted(capi, c, monkeypatch, *many)
    rb = _step(b, X0, o)
    b.close()
    off = _weighted(capi, c, monkeypatch, *many, structured_fallback=False)
    roff = _step(off, X0, o)
    off.close()
    left = np.nonzero(rb["status"] != 0)[0]
    print("weighted no-redo: %d of %d instances keep a status != 0; the shared design's redo leaves %d"
          % (left.size, c.batch, int((ra["status"] != 0).sum())))
    assert left.size >= 1 and np.all(rb["status"][left] == 1)
    assert int((ra["status"] != 0).sum()) < left.size
    _same_results(rb, roff, "redo off")


@pytest.mark.parametrize("back", ("batched", "shared"))
def test_a_later_design_puts_the_handle_back_on_shared_weights(capi, back, monkeypatch):
    c = wc.CASE_BY_ID["3-2-6-s"]
    Q, R, S = wc.weights(c)
    A, B = ic.models(c.base)
    t = ic.template(c.base)
    X0 = wc.x0(c)
    g_u, g_x = wc.loss(c)

    def design(s):
        if back == "batched":
            s.design_batched(A, B, Q[3], R[3], S[3], t.P, t.u_min, t.u_max)
        else:
            s.design_shared(A[3], B[3], Q[3], R[3], S[3], t.P, t.u_min, t.u_max)
        s.set_reference(t.x_ref, t.u_ref)

    used = _weighted(capi, c, monkeypatch, Q, R, S)
    _step(used, X0)
    used.sensitivity_params_vjp(g_u, g_x)
    design(used)
    fresh = capi.Solver(c.n, c.m, c.N, c.batch)
    design(fresh)
    out = []
    for s in (used, fresh):
        r = _step(s, X0)
        r["params"] = s.sensitivity_params_vjp(g_u, g_x)
        r["design"] = _design(s) if back == "batched" else [s.get_design()]
        r["weights"] = s.get_weights_instance(5)
        s.close()
        out.append(r)
    _same_results(out[0], out[1], back)
    for k in pr.GROUPS + ("rows",):
        assert _bits(out[0]["params"][k], out[1]["params"][k]), k
    for x, y in zip(out[0]["design"], out[1]["design"]):
        assert all(_bits(x[k], y[k]) for k in ("H", "F", "d", "P"))
    for k, M in (("Q", Q[3]), ("R", R[3]), ("S", S[3])):
        assert np.array_equal(out[0]["weights"][k], M) and np.array_equal(out[1]["weights"][k], M), k


# ---------------------------------------------------------------------------- 9. the group form
def test_group_equals_one_handle(capi, monkeypatch):
    c = wc.CASE_BY_ID["3-2-6-s"]
    Q, R, S = wc.weights(c)
    A, B = ic.models(c.base)
    t = ic.template(c.base)
    X0 = wc.x0(c)
    g_u, g_x = wc.loss(c)
    out = []
    for make in (lambda: capi.Solver(c.n, c.m, c.N, c.batch), lambda: capi.Group(c.n, c.m, c.N, c.batch, devices=[0, 0])):
        s = make()
        s.design_batched_weighted(A, B, Q, R, S, wc.terminal(c), t.u_min, t.u_max)
        s.set_reference(t.x_ref, t.u_ref)
        r = _step(s, X0)
        r["params"] = s.sensitivity_params_vjp(g_u, g_x)
        s.close()
        out.append(r)
    _same_results(out[0], out[1], "group")
    for k in pr.GROUPS + ("rows",):
        assert _bits(out[0]["params"][k], out[1]["params"][k]), k
    # the branch rule holds across the shards
    g = capi.Group(c.n, c.m, c.N, c.batch, devices=[0, 0])
    R2 = R.copy(); R2[c.batch - 2, 0, 0] = 0.0
    with pytest.raises(capi.AlmpcError) as e:
        g.design_batched_weighted(A, B, Q, R2, S, wc.terminal(c), t.u_min, t.u_max)
    assert e.value.code == ERR_INVALID and "instance %d" % (c.batch - 2) in str(e.value), e.value
    g.close()
