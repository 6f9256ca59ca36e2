"""What tests/test_gpu_sens_face.py and tests/test_gpu_sens_face_rate.py share: the design and solve of a case of their tables on a
handle, two array helpers and the refusal check.  Each file binds its own case table and entry points (functools.partial)."""
import numpy as np
import pytest

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
K_SENS_RTOL = 1e-8   # k_sens's tolerance (tests/test_gpu_sensitivity.py)


def design(s, name, cases, batched_S):
    """batched_S: a per-instance design is handed the case's S (the rate table) or none (the S = 0 table)"""
    ps, X0, shared = cases.case(name)
    if shared:
        p = ps
        s.design_shared(p.A, p.B, p.Q, p.R, p.S, p.P, p.u_min, p.u_max)
    else:
        p = ps[0]
        s.design_batched(np.stack([q.A for q in ps]), np.stack([q.B for q in ps]), p.Q, p.R, p.S if batched_S else None,
                         np.stack([q.P for q in ps]), p.u_min, p.u_max)
    s.set_reference(p.x_ref, p.u_ref)
    return p


def solve(capi, name, opts=None, make=None, structured=True, *, cases, batched_S):
    ps, X0, shared = cases.case(name)
    p = ps if shared else ps[0]
    s = make() if make else capi.Solver(p.n, p.m, p.N, X0.shape[0], structured=structured)
    design(s, name, cases, batched_S)
    s.update_initialization(X0)
    s.calculate(opts)
    return s


def flat(dU):
    """J (nz, n) stage-major from a Julia-shaped dU (m, N, n)"""
    m, N, n = dU.shape
    return dU.transpose(1, 0, 2).reshape(N * m, n)


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def refused(capi, s, code=ERR_UNSUPPORTED, *, jac, vjp):
    """jac, vjp: the names of the Solver's two sensitivity calls under test"""
    for call in (lambda: getattr(s, jac)(("K0",)), lambda: getattr(s, vjp)(np.zeros((s.batch, s.m, s.N)))):
        with pytest.raises(capi.AlmpcError) as e:
            call()
        assert e.value.code == code, e.value
        assert (s.L.almpc_last_error(s.h) or b"").decode().strip()
