"""Case table of the stage-wise time-varying design (almpc_design_ltv_stagewise): the problems, their generator and the oracle's
answers.  tests/test_ltv_stagewise_cases.py holds the table on the CPU; tests/test_gpu_ltv_stagewise.py runs it on the device.

The generator is tests/test_gpu_ltv.py's, per instance and stage:
    A_k = a I + 0.15 randn / sqrt(n / 4),  B_k = randn,  c_k = 0.1 randn,  xbar = xs randn,  ubar = 0.3 randn clipped into the box,
    x_ref = 0.2 randn, u_ref = 0.1 randn (or none),  Q = 10 I, R = I, P = 25 I + 0.2 ones,  umin = -0.6, umax = 0.8
with a = 0.9 unless the case says otherwise, xs = 0.3 with a state box (the box must hold xbar_0 ... loosely) and 1 without.
Seeds are chosen so that the properties tests/test_ltv_stagewise_cases.py asserts hold: every verdict is "solved" or "infeasible",
feasible cases with rows have an active state row, input-box cases have at least N m / 4 active inputs, at most a third of a case's
instances are infeasible.

The oracle is oracle/stagewise_oracle.py (stage_qp_from_ltv + solve_stage_dual); oracle/mpc_oracle.py's dense exact solvers
(ltv_qp + ltv_state_rows + solve_box_qp_exact / solve_qp_rows_exact) cross-check it where the case says `dense`: everywhere but the
two open-loop unstable cases, whose condensed Hessian (a^(2 N) = 1.12^140 in its entries) is what the stage-wise route exists to avoid.
"""
import functools

import numpy as np

UMIN, UMAX = -0.6, 0.8


class Case:
    def __init__(self, name, n, m, N, batch, seed, s=0.0, box=None, eq=False, a=0.9, r00_zero=False, null_refs=False, dense=True,
                 build="", feasible=True):
        self.name, self.n, self.m, self.N, self.batch, self.seed = name, n, m, N, batch, seed
        self.s, self.box, self.eq, self.a = s, box, eq, a
        self.r00_zero, self.null_refs, self.dense, self.build, self.feasible = r00_zero, null_refs, dense, build, feasible
        self.xs = 0.3 if box is not None else 1.0

    @property
    def rows(self):
        return self.box is not None or self.eq

    @property
    def route(self):   # the rule of the step: an input box alone without S -> k_riccati_t, else k_sgains + k_sdual
        return "sdual" if (self.rows or (self.s != 0.0 and not self.r00_zero)) else "riccati"

    def __repr__(self):
        return self.name


# (n, m, N) | S | rows | route / build: see the issue's table; `feasible` False: the case is meant to hold infeasible instances
CASES = [
    Case("twin-5-2-12", 5, 2, 12, 4, seed=3, build="k_riccati_t<0,0>"),
    Case("long-4-2-70", 4, 2, 70, 3, seed=11, build="k_riccati_t<4,2>"),
    Case("quad-12-4-40", 12, 4, 40, 3, seed=12, build="k_riccati_t<12,4>"),
    Case("long-4-2-70-S", 4, 2, 70, 3, seed=13, s=0.4, build="k_sdual (6, 2)"),
    Case("box-7-3-10", 7, 3, 10, 6, seed=143, box=0.9, build="k_sdual (8, 4)"),
    Case("box-7-3-10-tight", 7, 3, 10, 6, seed=143, box=0.7, build="k_sdual (8, 4)", feasible=False),
    Case("eq-4-2-9-S", 4, 2, 9, 6, seed=104, s=0.4, box=0.9, eq=True, build="k_sdual (6, 2)"),
    Case("eq-4-2-9-S-tight", 4, 2, 9, 6, seed=104, s=0.4, box=0.7, eq=True, build="k_sdual (6, 2)", feasible=False),
    Case("unstable-4-2-70", 4, 2, 70, 3, seed=18, a=1.12, dense=False, build="k_riccati_t<4,2>"),
    Case("unstable-4-2-70-S", 4, 2, 70, 3, seed=19, s=0.4, a=1.12, dense=False, build="k_sdual (6, 2)"),
    Case("widest-11-5-8", 11, 5, 8, 4, seed=100, box=0.9, eq=True, build="k_sdual (16, 8)"),
    Case("smallest-2-1-2", 2, 1, 2, 8, seed=122, s=0.4, box=0.9, eq=True, build="k_sdual (4, 2)"),
    Case("r00-3-1-37", 3, 1, 37, 4, seed=22, s=0.4, r00_zero=True, build="k_riccati_t<0,0>"),
    Case("nullrefs-4-2-16", 4, 2, 16, 4, seed=23, s=0.4, null_refs=True, build="k_sdual (6, 2)"),
    Case("generic-20-9-6", 20, 9, 6, 3, seed=24, build="k_riccati_t<0,0>"),
]
BY_NAME = {c.name: c for c in CASES}


def generate(case, seed=None, with_c=None):
    """The data of a case (seed: another draw of the five trajectory arrays of the same design, for the update path: weights, bounds and
    references stay the case's).  Shapes as Solver.design_ltv takes them."""
    rng = np.random.default_rng(case.seed if seed is None else seed)
    n, m, N, b = case.n, case.m, case.N, case.batch
    A_all = np.stack([[case.a * np.eye(n) + 0.15 * rng.standard_normal((n, n)) / np.sqrt(n / 4.0) for _ in range(N)] for _ in range(b)])
    B_all = rng.standard_normal((b, N, n, m))
    c_all = 0.1 * rng.standard_normal((b, N, n))
    xbar = case.xs * rng.standard_normal((b, n, N + 1))
    ubar = np.clip(0.3 * rng.standard_normal((b, m, N)), UMIN, UMAX)
    x_ref = 0.2 * rng.standard_normal((n, N + 1)); u_ref = 0.1 * rng.standard_normal((m, N))
    Q, R, S = 10.0 * np.eye(n), 1.0 * np.eye(m), case.s * np.eye(m)
    if case.r00_zero:
        R = R.copy(); R[0, 0] = 0.0
    P = 25.0 * np.eye(n) + 0.2 * np.ones((n, n))
    d = dict(A_all=A_all, B_all=B_all, c_all=c_all, xbar=xbar, ubar=ubar, x_ref=x_ref, u_ref=u_ref, Q=Q, R=R, S=S, P=P,
             umin=UMIN * np.ones(m), umax=UMAX * np.ones(m),
             xmin=None if case.box is None else -case.box * np.ones(n), xmax=None if case.box is None else case.box * np.ones(n),
             terminal="equality" if case.eq else "none")
    if seed is not None and seed != case.seed:   # another draw of the trajectory data: the references belong to the design
        base = generate(case)
        d["x_ref"], d["u_ref"] = base["x_ref"], base["u_ref"]
    if case.null_refs or with_c is False:
        d["c_all"] = None
    if case.null_refs:
        d["x_ref"] = d["u_ref"] = None
    return d


def rollout(d, i, v):
    """dx (n, N+1) of instance i for inputs v (N, m): dx_{k+1} = A_k dx_k + B_k v_k + c_k, dx_0 = 0"""
    N, n = d["A_all"].shape[1], d["A_all"].shape[2]
    dx = np.zeros((n, N + 1))
    for k in range(N):
        dx[:, k + 1] = d["A_all"][i, k] @ dx[:, k] + d["B_all"][i, k] @ v[k] + (0.0 if d["c_all"] is None else d["c_all"][i, k])
    return dx


def stage_qp(so, d, i):
    c = np.zeros(d["A_all"].shape[1:3]) if d["c_all"] is None else d["c_all"][i]
    return so.stage_qp_from_ltv(d["A_all"][i], d["B_all"][i], c, d["xbar"][i], d["ubar"][i], d["x_ref"], d["u_ref"], d["Q"], d["R"], d["S"],
                                d["P"], d["umin"], d["umax"], d["xmin"], d["xmax"], d["terminal"])


def solve(so, d):
    """The oracle on every instance of the data d: list of dict(status, v (N, m), dx (n, N+1), n_active_u, n_active_x)."""
    out = []
    b = d["A_all"].shape[0]
    for i in range(b):
        q = stage_qp(so, d, i)
        r = so.solve_stage_dual(q, v_guess=np.zeros_like(q.ulo))
        v = r["v"]
        on_u = int((np.isclose(v, q.ulo, atol=1e-9) | np.isclose(v, q.uhi, atol=1e-9)).sum()) if r["status"] == 0 else 0
        on_x = int(np.count_nonzero(r["lam_x"])) if r["status"] == 0 else 0
        out.append(dict(status=int(r["status"]), v=v, dx=rollout(d, i, v), n_active_u=on_u, n_active_x=on_x))
    return out


@functools.lru_cache(maxsize=None)
def _answers(name, seed):
    import stagewise_oracle as so   # (oracle/ is on the path of every test session: tests/conftest.py)
    case = BY_NAME[name]
    d = generate(case, seed)
    return d, solve(so, d)


def answers(case, seed=None):
    """(data, oracle results) of a case, computed once per session and shared: do not write into either."""
    return _answers(case.name, case.seed if seed is None else seed)


def gamma_norm(mo, d, i):
    """||Gamma||_inf of instance i: the prediction dX = Gamma v + g of the linearised dynamics"""
    c = None if d["c_all"] is None else d["c_all"][i]
    Gam = mo.ltv_qp(d["A_all"][i], d["B_all"][i], c, d["xbar"][i], d["ubar"][i], d["x_ref"], d["u_ref"], d["Q"], d["R"], d["S"], d["P"],
                    d["umin"], d["umax"], return_prediction=True)[4]
    return float(np.abs(Gam).sum(axis=1).max())


def dense_solve(mo, d, i):
    """The dense exact solvers on instance i: v (N, m), or None when they prove the QP infeasible"""
    N, m = d["B_all"].shape[1], d["B_all"].shape[3]
    c = None if d["c_all"] is None else d["c_all"][i]
    H, q, lo, hi, Gam, g = mo.ltv_qp(d["A_all"][i], d["B_all"][i], c, d["xbar"][i], d["ubar"][i], d["x_ref"], d["u_ref"], d["Q"], d["R"],
                                     d["S"], d["P"], d["umin"], d["umax"], return_prediction=True)
    if d["xmin"] is None and d["terminal"] != "equality":
        return mo.solve_box_qp_exact(H, q, lo, hi).reshape(N, m)
    if d["xmin"] is not None and (np.any(d["xbar"][i][:, 0] < d["xmin"]) or np.any(d["xbar"][i][:, 0] > d["xmax"])):
        return None   # stage 1 of the reference is x0 itself (dx_0 = 0): outside the box there is nothing to solve
    xr = np.zeros_like(d["xbar"][i]) if d["x_ref"] is None else d["x_ref"]
    C, a0, lo_c, hi_c, eq = mo.ltv_state_rows(Gam, g, d["xbar"][i], xr, d["xmin"], d["xmax"], d["terminal"])
    try:
        return mo.solve_qp_rows_exact(H, q, lo, hi, C, a0, lo_c, hi_c, eq)[0].reshape(N, m)
    except ValueError:
        return None
