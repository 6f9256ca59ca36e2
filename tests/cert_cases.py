"""The cases of the certificate tests (tests/test_cert_restatement.py on the CPU, tests/test_gpu_cert.py on the device).

A case is a design route and one problem per instance (mpc_oracle.MPCProblem: the instance's model, weights, terminal weight, bounds
and references) with its initial state:

  kind        "shared" (almpc_design_shared), "batched" (almpc_design_batched), "weighted" (almpc_design_batched_weighted)
  structured  an ALMPC_FLAG_STRUCTURED handle
  P           "dare": the design computes the terminal weight (P = NULL); "given": one P for the batch; "instance": one per instance
  refs        "shared" or "instance" (almpc_set_reference with per_instance)

  smallest horizons   2-1-1 (no recursion step, no rate pair), 2-1-2-S
  row fit             16-3-4 (RL = 16 exactly), 17-2-3, 33-5-3, 64-16-2 (the largest slice of LDS)
  routes              quad-12-4-5 (batch 67, amplitudes 0.02, 3 and 10 -- QUAD_AMPLITUDES: free and clamped inputs both occur, asserted by the
                      CPU test),
                      fused-7-4-29 (m N = 116: the one-kernel step, batch 17), fixture-4-2-5 (the reference's fixture, batch 1)
  weights, references R0-S (R[1,1] = 0, S[1,1] != 0: both terms dropped), tvref-S (time-varying per-instance u_ref with S)
  per instance        inst-dare (P = NULL), inst-P (P per instance), weighted-S (Q_i, R_i, S_i)
  structured          struct-4-2-70-S (m N = 140), struct-inst-5-3-12 (one model per instance), struct-R0-S (R0-S on a structured handle:
                      the design's own branch reaches the kernel there too)

Plants are random with spectral radius 0.97, bounds -0.5 / 0.7 and non-zero references (the recipe of
tests/condensed_step_cases.problem), initial states of amplitude 3.
"""
import copy
import functools
import os

import numpy as np

import mpc_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# The quadrotor's weights (Q = 100 I, P its DARE solution, |P| ~ 1e5) make the rounding noise of g itself large: cert_ref's bound on it
# is 3e-9 |x0|.  The solved-batch check  res <= 1e-9 max(1, |g|_inf)  is absolute where no input is clamped (g ~ 0), so it says something
# about the INPUTS only where that bound is well below 1e-9.  Hence the amplitudes: 0.02 for the instances without a clamped input
# (bound <= 0.2e-9: QUAD_NOISE_SHARE of the threshold, asserted on the CPU by tests/test_cert_restatement.py at the exact optimum),
# 3 and 10 for the clamped ones, whose |g|_inf of 1e3 .. 1e6 scales the threshold with the problem.  (count, amplitude, first instance)
QUAD_AMPLITUDES = ((22, 0.02, 0), (22, 3.0, 22), (23, 10.0, 44))
QUAD_NOISE_SHARE = 0.2
# The multiplier test asserts the signs of -g at the clamped inputs with no tolerance, so no input of the case may sit WEAKLY at a bound:
# at the exact optimum every clamped input's multiplier is at least QUAD_MULTIPLIER_MARGIN times the threshold of the solved-batch check
# (1e-9 max(1, |g|_inf), which bounds what the step's inputs may be off by in units of g); asserted on the CPU as well.
QUAD_MULTIPLIER_MARGIN = 1e3


class Case:
    def __init__(self, name, kind, problems, X0, structured=False, P="dare", refs="shared"):
        self.name, self.kind, self.problems, self.X0 = name, kind, tuple(problems), np.asarray(X0, dtype=np.float64)
        self.structured, self.P, self.refs = structured, P, refs
        p = self.problems[0]
        self.n, self.m, self.N, self.batch = p.n, p.m, p.N, len(self.problems)
        assert self.X0.shape == (self.batch, self.n) and self.batch <= 67

    def __repr__(self):
        return self.name


def _plant(rng, n, m, N, s, rho=0.97, **kw):
    A = rng.standard_normal((n, n))
    A *= rho / np.max(np.abs(np.linalg.eigvals(A)))
    B = rng.standard_normal((n, m))
    u_ref = 0.05 * rng.standard_normal((m, 1)) + 0.03 * rng.standard_normal((m, N))
    return mo.make_problem(A, B, N, -0.5 * np.ones(m), 0.7 * np.ones(m), x_ref=0.1 * rng.standard_normal(n), u_ref=u_ref, q=10.0, r=1.0, s=s, **kw)


def _shared(name, n, m, N, s, batch, amp=3.0, structured=False):
    rng = np.random.default_rng(9000 * n + 10 * m + N)
    p = _plant(rng, n, m, N, s)
    return Case(name, "shared", [p] * batch, amp * rng.standard_normal((batch, n)), structured=structured)


def _with(p, **kw):
    q = copy.copy(p)
    for k, v in kw.items():
        setattr(q, k, np.array(v, dtype=np.float64))
    return q


def _quad():
    p = mo.quadrotor(N=5)
    X0 = np.concatenate([mo.quadrotor_x0_batch(c, a, first_instance=f) for c, a, f in QUAD_AMPLITUDES])
    return Case("quad-12-4-5", "shared", [p] * 67, X0)


def _fixture():
    with open(os.path.join(GOLDEN, "linear_regressor_train_result.jls"), "rb") as f:
        A, B = mo.decode_linear_regressor_fixture(f.read())
    return Case("fixture-4-2-5", "shared", [mo.qtp_linear_fixture_problem(A, B)], 0.6 * np.ones((1, 4)))


def _r0_s(name="R0-S", structured=False):
    rng = np.random.default_rng(41)
    n, m, N, b = 3, 2, 6, 5
    p = _plant(rng, n, m, N, 0.5)   # (its P: the DARE solution with R = I, given to the design, whose own R has no DARE)
    return Case(name, "shared", [_with(p, R=np.diag([0.0, 1.0]))] * b, 3.0 * rng.standard_normal((b, n)), structured=structured, P="given")


def _tvref_s():
    rng = np.random.default_rng(43)
    n, m, N, b = 4, 2, 9, 7
    p = _plant(rng, n, m, N, 0.5)
    ps = [_with(p, x_ref=p.x_ref + 0.05 * rng.standard_normal((n, 1)), u_ref=p.u_ref + 0.04 * rng.standard_normal((m, N))) for _ in range(b)]
    return Case("tvref-S", "shared", ps, 3.0 * rng.standard_normal((b, n)), refs="instance")


def _instances(name, seed, n, m, N, b, s, P, kind="batched", structured=False):
    """one model per instance: spectral radius 0.7 .. 1.05 (the open-loop unstable ones included), shared references"""
    rng = np.random.default_rng(seed)
    base = _plant(rng, n, m, N, s)
    ps = []
    for i in range(b):
        A = rng.standard_normal((n, n)); A *= (0.7 + 0.35 * rng.random()) / np.max(np.abs(np.linalg.eigvals(A)))
        Bm = rng.standard_normal((n, m))
        kw = dict(A=A, B=Bm)
        if kind == "weighted":
            Q = base.Q * (0.5 + rng.random()) + 0.1 * np.diag(rng.random(n)); R = base.R * (0.5 + rng.random()); S = base.S * (0.5 + rng.random())
            kw.update(Q=Q, R=R, S=S)
        q = _with(base, **kw)
        if P == "instance":     # a weight of the caller's own: the DARE solution, scaled
            q.P = (1.0 + 0.5 * rng.random()) * mo.dare(q.A, q.B, q.Q, q.R)
        else:                   # the design's: restated here, read back from the handle on the device
            q.P = mo.dare(q.A, q.B, q.Q, q.R)
        ps.append(q)
    return Case(name, kind, ps, 3.0 * rng.standard_normal((b, n)), structured=structured, P=P)


@functools.lru_cache(maxsize=None)
def cases():
    cs = (
        _shared("2-1-1", 2, 1, 1, 0.0, 5), _shared("2-1-2-S", 2, 1, 2, 0.5, 5),
        _shared("16-3-4", 16, 3, 4, 0.5, 5), _shared("17-2-3", 17, 2, 3, 0.5, 5), _shared("33-5-3", 33, 5, 3, 0.5, 5),
        _shared("64-16-2", 64, 16, 2, 0.5, 5),
        _quad(), _shared("fused-7-4-29", 7, 4, 29, 0.5, 17), _fixture(),
        _r0_s(), _tvref_s(),
        _instances("inst-dare", 51, 5, 3, 8, 9, 0.5, "dare"), _instances("inst-P", 52, 5, 3, 8, 9, 0.0, "instance"),
        _instances("weighted-S", 53, 5, 3, 8, 9, 0.5, "dare", kind="weighted"),
        _shared("struct-4-2-70-S", 4, 2, 70, 0.5, 5, structured=True),
        _instances("struct-inst-5-3-12", 54, 5, 3, 12, 7, 0.0, "dare", structured=True),
        _r0_s("struct-R0-S", structured=True),
    )
    return {c.name: c for c in cs}


NAMES = ("2-1-1", "2-1-2-S", "16-3-4", "17-2-3", "33-5-3", "64-16-2", "quad-12-4-5", "fused-7-4-29", "fixture-4-2-5", "R0-S", "tvref-S",
         "inst-dare", "inst-P", "weighted-S", "struct-4-2-70-S", "struct-inst-5-3-12", "struct-R0-S")


def case(name):
    return cases()[name]


def flat_bounds(p):
    """(lo, hi) of v = vec(e_u), stage-major (mpc_oracle.condensed_qp's)"""
    return (p.u_min[:, None] - p.u_ref).T.reshape(-1), (p.u_max[:, None] - p.u_ref).T.reshape(-1)


@functools.lru_cache(maxsize=None)
def exact(name, i):
    """v* (m N,) of instance i by the exact oracle: computed once per process, read-only"""
    c = case(name)
    p = c.problems[i]
    H, f, lo, hi = mo.condensed_qp(p, c.X0[i])
    v = mo.solve_box_qp_exact(H, f, lo, hi)
    v.setflags(write=False)
    return v
