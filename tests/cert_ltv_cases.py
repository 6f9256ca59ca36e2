"""The cases of the certificate of a time-varying design (k_cert_ltv), one table for tests/test_cert_ltv_restatement.py (CPU) and
tests/test_gpu_cert_ltv.py (GPU): the sixteen of nlp_shape_cases.LTV with their own ltv_inputs -- N = 1, 2, 3, m N = 128,
c_all = None with S = None, one P per instance -- and four more by the same recipe:
    16-3-4       n fills a 16-lane row group exactly
    16-1-59      the largest stage-model footprint an LTV step accepts ((N + 1)(n + m) = 1020 of 1024)
    4-2-3-r0     R[0,0] = 0: both weight terms dropped (useR = useS = 0)
    4-2-3-uref   a time-varying u_ref and S != 0 (non-diagonal)
Every case has batch 4."""
import functools

import numpy as np

import mpc_oracle as mo
import nlp_shape_cases as nc

QUAD_NOISE_SHARE = 0.2   # cert_cases.QUAD_NOISE_SHARE: the share of the 1e-9 max(1, |g|) threshold left to the exact optimum's residual

_EXTRA = {
    "16-3-4": nc._ltv(16, 3, 4),
    "16-1-59": nc._ltv(16, 1, 59),
    "4-2-3-r0": nc._ltv(4, 2, 3, amp=2.0, seed=1),
    "4-2-3-uref": nc._ltv(4, 2, 3, amp=2.0, seed=2),
}
_BASE = {c.id[len("ltv-"):]: c for c in nc.LTV}
NAMES = tuple(_BASE) + tuple(_EXTRA)
assert len(NAMES) == 20


def shape(name):
    return (_BASE.get(name) or _EXTRA[name]).shape


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict of design_ltv's arguments (nlp_shape_cases.ltv_inputs and the four changes above), read-only"""
    c = _BASE.get(name) or _EXTRA[name]
    a = dict(nc.ltv_inputs(c))
    n, m, N = c.shape
    if name == "4-2-3-r0":
        R = a["R"].copy(); R[0, 0] = 0.0
        a["R"] = R
    if name == "4-2-3-uref":
        a["u_ref"] = 0.1 * np.sin(1.0 + np.arange(m * N, dtype=np.float64)).reshape(m, N) * (1.0 + np.arange(N))
        a["S"] = 0.3 * np.eye(m) + 0.05 * np.ones((m, m))
    for v in a.values():
        if v is not None:
            v.setflags(write=False)
    return a


def instance(name, i):
    """the arguments of cert_ltv_ref.certificate_ltv that belong to instance i (everything but v and u), and ubar"""
    a = inputs(name)
    P = a["P"][i] if a["P"].ndim == 3 else a["P"]
    c = None if a["c_all"] is None else a["c_all"][i]
    return dict(A=a["A_all"][i], B=a["B_all"][i], c=c, xbar=a["xbar"][i], xref=a["x_ref"], uref=a["u_ref"], Q=a["Q"], R=a["R"], S=a["S"],
                P=P, umin=a["umin"], umax=a["umax"]), a["ubar"][i]


@functools.lru_cache(maxsize=None)
def qp(name, i):
    """dict(H, q, lo, hi, Gam, g, v) of instance i: mo.ltv_qp with the prediction, and its exact optimum v*"""
    k, ubar = instance(name, i)
    m = ubar.shape[0]
    S = np.zeros((m, m)) if k["S"] is None else k["S"]
    H, q, lo, hi, Gam, g = mo.ltv_qp(k["A"], k["B"], k["c"], k["xbar"], ubar, k["xref"], k["uref"], k["Q"], k["R"], S, k["P"], k["umin"],
                                     k["umax"], return_prediction=True)
    return dict(H=H, q=q, lo=lo, hi=hi, Gam=Gam, g=g, v=mo.solve_box_qp_exact(H, q, lo, hi))
