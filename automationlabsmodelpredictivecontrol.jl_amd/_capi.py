"""ctypes binding of libalmpc.so (include/almpc.h).  The HIP library is the only compute path: if it is
missing or fails to load this module raises -- there is no CPU fallback.

A new entry point is bound by one line of the prototype table below (_HANDLE_CALLS; its name in _GROUP_FORMS too if the header
has an almpc_group_ form of the same signature) and one method: on _Target if both forms exist, else on Solver or Group."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ALMPC_LIB overrides the library path (A/B builds of the same ABI); the default is the in-tree build
LIB_PATH = os.environ.get("ALMPC_LIB") or os.path.join(_HERE, "lib", "libalmpc.so")

ALMPC_OK = 0
ERR_NAMES = {0: "ALMPC_OK", -1: "ALMPC_ERR_INVALID", -2: "ALMPC_ERR_NO_DEVICE", -3: "ALMPC_ERR_HIP",
             -4: "ALMPC_ERR_UNSUPPORTED", -5: "ALMPC_ERR_NOT_DESIGNED", -6: "ALMPC_ERR_NUMERIC"}
FLAG_TIMING = 0x1
FLAG_STRUCTURED = 0x2
SOLVED, MAX_ITER, NON_FINITE, INFEASIBLE = 0, 1, 2, 3


class AlmpcError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")


class almpc_opts(ctypes.Structure):
    _fields_ = [("rho", ctypes.c_double), ("sigma", ctypes.c_double), ("alpha", ctypes.c_double),
                ("eps_abs", ctypes.c_double), ("eps_rel", ctypes.c_double), ("max_iter", ctypes.c_int32),
                ("check_every", ctypes.c_int32), ("polish", ctypes.c_int32), ("polish_max_iter", ctypes.c_int32),
                ("warm_start", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_fp = ctypes.POINTER(ctypes.c_float)
_hp = ctypes.c_void_p
_lib = None


class almpc_param_grads(ctypes.Structure):
    """almpc.h: almpc_param_grads (almpc_sensitivity_params_vjp): host pointers, NULL = not wanted."""
    _fields_ = [(k, _dp) for k in ("x0", "f", "u_ref", "u_min", "u_max", "Q", "P", "A", "R", "S", "B")] + [("rows", _ip)]


# ---- the prototypes of include/almpc.h (tests/test_capi_marshalling.py holds this table against the header)
_i, _d, _u32 = ctypes.c_int, ctypes.c_double, ctypes.c_uint32
_cip = ctypes.POINTER(ctypes.c_int)
_op = ctypes.POINTER(almpc_opts)
_gp = ctypes.POINTER(almpc_param_grads)
_vpp = ctypes.POINTER(ctypes.c_void_p)
_NET = [_i, _i, _i] + [_dp] * 4                      # H, L, activation, W_in, W_h, b_h, W_out
_BOX = [_dp, _dp, _d, _d]                            # umin, umax, rho, sigma
_BATCHED = [_dp] * 6 + [_i] + _BOX                   # A, B, Q, R, S, P, P_per_instance, ...
_SQP_SETUP = _NET + [_dp] * 6 + [_i] + _BOX          # ..., x_ref, u_ref, Q, R, S, P, P_per_instance, ...
_RELIN_SETUP = _NET + [_dp] * 6 + _BOX
_VJP = [_dp, _dp, _d, _dp, _ip]                      # g_u, g_x, act_tol, g_x0, rows
_RESULTS = [_dp] * 4 + [_ip] * 3                     # x, e_x, u, e_u, status, iters, polish_iters
_RESULTS_U0 = [_dp] * 5 + [_ip] * 3                  # ... with u0 after e_u
_LINEARIZE = [_i] * 6 + [_dp] * 4 + [_i] + [_dp] * 5

# almpc_<name>(handle, ...): the arguments after the handle
_HANDLE_CALLS = {
    "last_error": [], "set_terminal_equality": [_i], "set_rho_profile": [_i], "set_step_fusion": [_i], "set_structured_fallback": [_i],
    "set_start_from": [_hp], "set_state_box": [_dp, _dp], "set_terminal_weight": [_i], "set_model_time": [_i, _d],
    "set_keep_stage_models": [_i],
    "design_shared": [_dp] * 10 + [_d, _d], "design_batched": _BATCHED, "design_batched_weighted": _BATCHED,
    "design_ltv": [_dp] * 11 + [_i] + _BOX,
    "design_ltv_stagewise": [_dp] * 11 + [_i, _dp, _dp, _i], "ltv_stagewise_update": [_dp] * 5 + [_i],
    "get_ltv_stagewise_prepared": [_dp] * 3,
    "get_weights_instance": [_i, _dp, _dp, _dp], "get_design_instance": [_i, _dp, _dp, _dp], "get_gradient_instance": [_i, _dp],
    "get_terminal_weight_instance": [_i, _dp], "get_model_instance": [_i, _dp, _dp], "get_design": [_dp] * 4,
    "sqp_fnn_setup": _SQP_SETUP, "sqp_densenet_setup": _SQP_SETUP, "sqp_fnn_start": [_dp, _dp],
    "sqp_fnn_iterate": [_i, _d, _op, _dp, _dp], "sqp_fnn_solve": [_i, _d, _op, _ip, _ip, _dp], "sqp_fnn_skipped": [_ip],
    "sqp_fnn_set_step_rule": [_i], "sqp_fnn_set_hessian": [_i], "sqp_fnn_set_row_multipliers": [_i], "sqp_fnn_set_structured": [_i],
    "sqp_fnn_state_multipliers": [_dp],
    "relin_fnn_setup": _RELIN_SETUP, "relin_densenet_setup": _RELIN_SETUP, "relin_fnn_step": [_op], "relin_fnn_step_async": [_op],
    "relin_fnn_advance": [], "relin_fnn_timing": [_fp] * 3, "relin_fnn_terminal_status": [_ip], "relin_fnn_certificate": [_u32],
    "set_reference": [_dp, _dp, _i], "update_initialization": [_dp], "update_initialization_device": [ctypes.c_void_p],
    "update_initialization_async": [_dp], "x0_staging": [ctypes.POINTER(_dp)],
    "calculate": [_op], "calculate_async": [_op], "synchronize": [], "advance_plant": [],
    "get_results": _RESULTS, "get_results_async": [_u32], "get_results_wait": [_i] + _RESULTS_U0, "host_results": [_i] + [_vpp] * 8,
    "get_first_input": [_dp], "device_results": [_vpp] * 4,
    "sensitivity": [_u32, _d], "get_sensitivity": [_dp, _dp, _dp, _ip], "device_sensitivity": [_vpp] * 4, "sensitivity_vjp": _VJP,
    "sensitivity_rows": [_u32, _d, _d], "sensitivity_rows_vjp": [_dp, _dp, _d, _d, _dp, _ip],
    "sensitivity_stagewise": [_u32, _d], "sensitivity_stagewise_vjp": _VJP,
    "sensitivity_stagewise_rate": [_u32, _d], "sensitivity_stagewise_rate_vjp": _VJP,
    "sensitivity_ltv": [_u32, _d], "sensitivity_ltv_vjp": _VJP,
    "sensitivity_params_vjp": [_dp, _dp, _d, _gp], "sensitivity_params_vjp_dare": [_dp, _dp, _d, _gp, _ip],
    "certificate": [_u32], "get_certificate": [_dp] * 4, "device_certificate": [_vpp] * 4,
    "certificate_ltv": [_u32], "get_certificate_ltv": [_dp] * 6, "device_certificate_ltv": [_vpp] * 6,
    "get_timing": [_fp] * 4, "timing_reset": [_i], "timing_set_stride": [_i], "timing_summary": [_cip] + [_dp] * 4,
    "timing_samples": [_i, _cip] + [_fp] * 4,
    "comm_init": [ctypes.c_char_p, _i, _i], "comm_summary": [ctypes.POINTER(ctypes.c_int64)],
    "comm_allgather_first_input": [_dp, ctypes.POINTER(_dp)], "debug_poison_lds": [],
}
# almpc_group_<name>(group, ...) with the arguments of almpc_<name>(handle, ...)
_GROUP_FORMS = (
    "last_error", "set_terminal_equality", "set_rho_profile", "set_structured_fallback", "set_state_box", "set_terminal_weight",
    "set_model_time", "design_shared", "design_batched", "design_batched_weighted",
    "sqp_fnn_setup", "sqp_densenet_setup", "sqp_fnn_start", "sqp_fnn_iterate", "sqp_fnn_solve", "sqp_fnn_skipped", "sqp_fnn_set_step_rule",
    "sqp_fnn_set_hessian", "sqp_fnn_set_row_multipliers", "sqp_fnn_set_structured", "sqp_fnn_state_multipliers",
    "relin_fnn_setup", "relin_densenet_setup", "relin_fnn_step", "relin_fnn_step_async", "relin_fnn_advance", "relin_fnn_certificate",
    "set_reference", "update_initialization", "calculate", "calculate_async", "synchronize", "advance_plant",
    "get_results_async", "get_results_wait",
    "sensitivity", "get_sensitivity", "sensitivity_vjp", "sensitivity_rows", "sensitivity_rows_vjp", "sensitivity_stagewise",
    "sensitivity_stagewise_vjp", "sensitivity_stagewise_rate", "sensitivity_stagewise_rate_vjp", "sensitivity_params_vjp",
    "sensitivity_params_vjp_dare", "certificate", "get_certificate",
)
# everything else, by its full name
_OTHER_CALLS = {
    "almpc_default_opts": [_op], "almpc_create": [ctypes.POINTER(_hp), _i, _i, _i, _i, _i, _u32], "almpc_destroy": [_hp],
    "almpc_group_create": [ctypes.POINTER(_hp), _i, _i, _i, _i, _i, _cip, _u32], "almpc_group_destroy": [_hp],
    "almpc_group_size": [_hp], "almpc_group_handle": [_hp, _i], "almpc_group_shard": [_hp, _i, _cip, _cip],
    "almpc_group_get_results": [_hp] + _RESULTS_U0, "almpc_group_x0_staging": [_hp, ctypes.POINTER(_dp)],
    "almpc_group_update_initialization_staged": [_hp, ctypes.POINTER(_dp)],
    "almpc_dare": [_i, _i] + [_dp] * 5, "almpc_dare_batched": [_i] * 4 + [_dp] * 5 + [_ip],
    "almpc_dare_vjp": [_i, _i] + [_dp] * 10, "almpc_dare_vjp_batched": [_i] * 4 + [_dp] * 10 + [_ip],
    "almpc_c2d": [_i, _i, _dp, _dp, _d, _dp, _dp], "almpc_c2d_batched": [_i] * 4 + [_dp, _dp, _d, _dp, _dp, _ip],
    "almpc_fnn_linearize": _LINEARIZE, "almpc_densenet_linearize": _LINEARIZE, "almpc_comm_unique_id": [ctypes.c_char_p],
}
# the return type is int unless named here
_RESTYPES = {"almpc_default_opts": None, "almpc_destroy": None, "almpc_group_destroy": None, "almpc_last_error": ctypes.c_char_p,
             "almpc_group_last_error": ctypes.c_char_p, "almpc_group_handle": _hp}


def prototypes():
    """{symbol: argument types} of every function of include/almpc.h this module binds."""
    table = {"almpc_" + k: [_hp] + v for k, v in _HANDLE_CALLS.items()}
    table.update({"almpc_group_" + k: [_hp] + _HANDLE_CALLS[k] for k in _GROUP_FORMS})
    table.update(_OTHER_CALLS)
    return table


def load():
    """Load libalmpc.so and declare the prototypes of include/almpc.h.  Raises OSError if the
    library has not been built (`make lib` or `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} not found: build the HIP library first (make lib). There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    for name, argtypes in prototypes().items():
        getattr(L, name).argtypes = argtypes
    for name, restype in _RESTYPES.items():
        getattr(L, name).restype = restype
    _lib = L
    return L


OPT_NO_WARM_STATE = 0x1  # almpc.h: ALMPC_OPT_NO_WARM_STATE (opts.reserved[0])
OPT_FULL_FIRST_PRODUCT = 0x2  # almpc.h: ALMPC_OPT_FULL_FIRST_PRODUCT (opts.reserved[0]): A/B control of the cold start's affine first iterate
OPT_HBM_HANDOFF = 0x4  # almpc.h: ALMPC_OPT_HBM_HANDOFF (opts.reserved[0]): A/B control of the one-kernel step's LDS hand-off
# almpc.h: ALMPC_WANT_* (almpc_get_results_async)
WANT = {"x": 0x01, "e_x": 0x02, "u": 0x04, "e_u": 0x08, "status": 0x10, "iters": 0x20, "polish_iters": 0x40, "u0": 0x80}
# almpc.h: ALMPC_SENS_* (almpc_sensitivity)
SENS = {"K0": 0x1, "dU": 0x2, "dX": 0x4}
# almpc.h: ALMPC_CERT_* (almpc_certificate)
CERT = {"cost": 0x1, "res": 0x2, "grad": 0x4, "costate": 0x8}
# ... and ALMPC_CERT_STATES (almpc_certificate_ltv: x and e_x come together)
CERT_LTV = dict(CERT, x=0x10, e_x=0x10)


# ---- host arrays as the C calls take them, each conversion written once
def _vec(v, k):
    """a vector of length k"""
    return np.ascontiguousarray(v, dtype=np.float64).reshape(k)


def _blocks(M, b, r, c):
    """(b, r, c) -> one column-major r x c block per instance"""
    return np.ascontiguousarray(np.asarray(M, dtype=np.float64).reshape(b, r, c).transpose(0, 2, 1))


def _traj(T, rows, stages):
    """a shared trajectory (rows, stages) -> stage-major"""
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(rows, stages).T)


_traj_batch = _blocks   # one trajectory (rows, stages) per instance -> stage-major: the same move


def _terminal_weight(P, b, n):
    """P (n, n) shared or (b, n, n) per instance -> (array, P_per_instance)"""
    P = np.asarray(P, dtype=np.float64)
    if P.ndim == 3:
        return _blocks(P, b, n, n), 1
    return _colmajor(P, (n, n)), 0


def _rho_code(rho_profile):
    """almpc_set_rho_profile: "scalar" (OSQP: rho for every row) | "stiffness" (rho_i = rho / (H'^-1)_ii)"""
    return {"scalar": 0, "stiffness": 1}[rho_profile]


def _optional(conv, a, *args):
    return None if a is None else conv(a, *args)


def _sens_mask(want):
    mask = 0
    for k in ((want,) if isinstance(want, str) else want):
        if k not in SENS:
            raise ValueError(f"unknown sensitivity {k!r} (one of {sorted(SENS)})")
        mask |= SENS[k]
    if not mask:
        raise ValueError("sensitivity: nothing asked for")
    return mask


def _sens_read(get, handle, check, want, b, n, m, N):
    """The Jacobians of the last sensitivity call, Julia-shaped: K0 (batch, m, n), dU (batch, m, N, n), dX (batch, n, N+1, n)
    -- [b, i, k, c] = d(entry i of stage k) / d x0[c] --, and rows (batch,)."""
    mask = _sens_mask(want)
    K0 = np.empty((b, n, m)) if mask & SENS["K0"] else None
    dU = np.empty((b, n, N, m)) if mask & SENS["dU"] else None
    dX = np.empty((b, n, N + 1, n)) if mask & SENS["dX"] else None
    rows = np.empty(b, dtype=np.int32)
    check(get(handle, _ptr(K0), _ptr(dU), _ptr(dX), rows.ctypes.data_as(_ip)))
    out = {"rows": rows}
    if K0 is not None: out["K0"] = K0.transpose(0, 2, 1)
    if dU is not None: out["dU"] = dU.transpose(0, 3, 2, 1)
    if dX is not None: out["dX"] = dX.transpose(0, 3, 2, 1)
    return out


def _cert_mask(want, table=CERT):
    mask = 0
    for k in ((want,) if isinstance(want, str) else want):
        if k not in table:
            raise ValueError(f"unknown certificate quantity {k!r} (one of {sorted(table)})")
        mask |= table[k]
    if not mask:
        raise ValueError("certificate: nothing asked for")
    return mask


def _cert_read(get, handle, check, want, b, n, m, N):
    """What the last certificate call computed, shaped as get_results shapes u and x: cost (batch,), res (batch,),
    grad (batch, m, N), costate (batch, n, N+1)."""
    mask = _cert_mask(want)
    cost = np.empty(b) if mask & CERT["cost"] else None
    res = np.empty(b) if mask & CERT["res"] else None
    grad = np.empty((b, N, m)) if mask & CERT["grad"] else None
    costate = np.empty((b, N + 1, n)) if mask & CERT["costate"] else None
    check(get(handle, _ptr(cost), _ptr(res), _ptr(grad), _ptr(costate)))
    out = {}
    if cost is not None: out["cost"] = cost
    if res is not None: out["res"] = res
    if grad is not None: out["grad"] = grad.transpose(0, 2, 1)
    if costate is not None: out["costate"] = costate.transpose(0, 2, 1)
    return out


def multipliers(grad, u, umin, umax, act_tol=1e-9):
    """Multipliers of the input box from a certificate's grad and the step's u, both (batch, m, N): mu = -grad at the inputs that sit
    at a bound, zero elsewhere, in the OSQP sign convention (positive at umax, negative at umin).  An input is at a bound when it is
    within act_tol * (umax - umin) of it.  Host side: the device applies no activity tolerance."""
    grad = np.asarray(grad, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    lo = np.asarray(umin, dtype=np.float64).reshape(1, -1, 1)
    hi = np.asarray(umax, dtype=np.float64).reshape(1, -1, 1)
    tol = float(act_tol) * (hi - lo)
    active = (u - lo <= tol) | (hi - u <= tol)
    return np.where(active, -grad, 0.0)


def _sens_vjp(call, handle, check, g_u, g_x, act_tol, b, n, m, N):
    """act_tol: the tolerance of almpc_sensitivity_vjp, or the pair (act_tol_u, act_tol_x) of the rows form."""
    g_u, g_x = _traj_batch(g_u, b, m, N), _optional(_traj_batch, g_x, b, n, N + 1)
    g_x0 = np.empty((b, n))
    rows = np.empty(b, dtype=np.int32)
    tols = tuple(float(t) for t in act_tol) if isinstance(act_tol, tuple) else (float(act_tol),)
    check(call(handle, _ptr(g_u), _ptr(g_x), *tols, _ptr(g_x0), rows.ctypes.data_as(_ip)))
    return g_x0, rows


PARAM_GROUPS = ("x0", "f", "u_ref", "u_min", "u_max", "Q", "P", "A", "R", "S", "B")   # almpc.h: the fields of almpc_param_grads


TERMINAL_GRADIENTS = ("data", "dare")   # almpc_sensitivity_params_vjp, almpc_sensitivity_params_vjp_dare


def _sens_params_vjp(call, handle, check, g_u, g_x, want, act_tol, b, n, m, N, dare=False):
    """almpc_sensitivity_params_vjp: {group: array} for the groups `want` names, Julia-shaped with the batch axis first -- x0 (b, n),
    f and u_ref (b, m, N), u_min / u_max (b, m), Q / P / A (b, n, n), R / S (b, m, m), B (b, n, m) --, and rows (b,).  dare: `call` is
    the _dare form, which also fills dare_status (b,)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    for k in want:
        if k not in PARAM_GROUPS:
            raise ValueError(f"unknown parameter group {k!r} (one of {PARAM_GROUPS})")
    g_u, g_x = _traj_batch(g_u, b, m, N), _optional(_traj_batch, g_x, b, n, N + 1)
    # the C layouts: stage-major trajectories, column-major matrices
    shapes = {"x0": (b, n), "f": (b, N, m), "u_ref": (b, N, m), "u_min": (b, m), "u_max": (b, m), "Q": (b, n, n), "P": (b, n, n),
              "A": (b, n, n), "R": (b, m, m), "S": (b, m, m), "B": (b, m, n)}
    # (one block for all of them: several fresh arrays of this size cost the read-back ten times what the copies take)
    sizes = [int(np.prod(shapes[k])) for k in want]
    block, offs = np.empty(sum(sizes)), np.cumsum([0] + sizes)
    raw = {k: block[offs[i]:offs[i + 1]].reshape(shapes[k]) for i, k in enumerate(want)}
    rows = np.empty(b, dtype=np.int32)
    out = almpc_param_grads(**{k: _ptr(v) for k, v in raw.items()}, rows=rows.ctypes.data_as(_ip))
    dare_status = np.zeros(b, dtype=np.int32) if dare else None
    check(call(handle, _ptr(g_u), _ptr(g_x), float(act_tol), ctypes.byref(out), *((dare_status.ctypes.data_as(_ip),) if dare else ())))
    res = {k: (v if v.ndim == 2 else v.transpose(0, 2, 1)) for k, v in raw.items()}
    res["rows"] = rows
    if dare:
        res["dare_status"] = dare_status
    return res


def _terminal_gradient(terminal):
    if terminal not in TERMINAL_GRADIENTS:
        raise ValueError(f"unknown terminal {terminal!r}; choose from {TERMINAL_GRADIENTS}")
    return terminal == "dare"


def _want_mask(want):
    try:
        return sum(WANT[k] for k in set(want))
    except KeyError as e:
        raise ValueError(f"unknown result {e.args[0]!r}; choose from {sorted(WANT)}") from None


def _result_table(b, n, m, N):
    """{name: (shape of the C buffer, dtype, ctypes pointer type)} in the order of the C calls' arguments; the trajectories (three
    axes) are stage-major there and go back Julia-shaped, as (batch, n, N+1) and (batch, m, N) views"""
    shapes = {"x": (b, N + 1, n), "e_x": (b, N + 1, n), "u": (b, N, m), "e_u": (b, N, m), "u0": (b, m),
              "status": (b,), "iters": (b,), "polish_iters": (b,)}
    f8, i4 = np.dtype(np.float64), np.dtype(np.int32)   # (dtype objects: np.empty takes them as they are)
    return {k: (s, i4, _ip) if len(s) == 1 else (s, f8, _dp) for k, s in shapes.items()}


def _result_bufs(table, want):
    """fresh buffers for the names of `table` that `want` holds: ({name: its Julia-shaped view}, the pointer list of the C call with
    NULL = not wanted)"""
    bufs, args = {}, []
    for k, (shape, dtype, ptype) in table.items():
        if k in want:
            a = np.empty(shape, dtype)
            args.append(a.ctypes.data_as(ptype))
            bufs[k] = a.transpose(0, 2, 1) if len(shape) == 3 else a
        else:
            args.append(None)
    return bufs, args


def comm_unique_id() -> bytes:
    """128-byte RCCL id made by rank 0 (almpc_comm_unique_id); hand it to the other ranks by any channel."""
    buf = ctypes.create_string_buffer(128)
    rc = load().almpc_comm_unique_id(buf)
    if rc != ALMPC_OK:
        raise AlmpcError(rc, "almpc_comm_unique_id (librccl not loadable?)")
    return buf.raw


def default_opts(**kw) -> almpc_opts:
    """almpc_default_opts, then the given fields.  keep_warm_state=False sets ALMPC_OPT_NO_WARM_STATE (the step does not store the
    ADMM state a later warm start would need)."""
    o = almpc_opts()
    load().almpc_default_opts(ctypes.byref(o))
    if "keep_warm_state" in kw:
        if not kw.pop("keep_warm_state"):
            o.reserved[0] |= OPT_NO_WARM_STATE
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown solver option {k!r}")
        setattr(o, k, v)
    return o


def _colmajor(a, shape=None):
    a = np.asfortranarray(np.asarray(a, dtype=np.float64))
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


def dare(A, B, Q, R):
    """P = DARE(A, B, Q, R) through the library (host code, as ControlSystems.are at src/sub/design_mpc.jl:327)."""
    L = load()
    A, B = np.asfortranarray(A, dtype=np.float64), np.asfortranarray(B, dtype=np.float64)
    n, m = B.shape
    Q, R = _colmajor(Q, (n, n)), _colmajor(R, (m, m))
    P = np.empty((n, n), order="F")
    rc = L.almpc_dare(n, m, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P))
    if rc != ALMPC_OK:
        raise AlmpcError(rc, "almpc_dare")
    return P


def dare_vjp(A, B, Q, R, P, g_P, want=("A", "B", "Q", "R")) -> dict:
    """The adjoint of dare (almpc_dare_vjp, host code): for P = DARE(A, B, Q, R) and a symmetric g_P = dL/dP, what the loss gains through
    P in A (n, n), B (n, m), Q (n, n), R (m, m) -- the ones `want` names.  AlmpcError -6 when P is not the stabilising solution of this
    model; its text carries the status (1 singular R + B'PB, 2 closed loop not stable, 3 P does not solve the equation)."""
    L = load()
    A, B = np.asfortranarray(A, dtype=np.float64), np.asfortranarray(B, dtype=np.float64)
    n, m = B.shape
    Q, R, P, g_P = _colmajor(Q, (n, n)), _colmajor(R, (m, m)), _colmajor(P, (n, n)), _colmajor(g_P, (n, n))
    shapes = {"A": (n, n), "B": (n, m), "Q": (n, n), "R": (m, m)}
    out = {k: np.empty(shapes[k], order="F") for k in want}
    rc = L.almpc_dare_vjp(n, m, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P), _ptr(g_P), *(_ptr(out.get(k)) for k in ("A", "B", "Q", "R")))
    if rc != ALMPC_OK:
        raise AlmpcError(rc, "almpc_dare_vjp" if rc != -6 else L.almpc_last_error(None).decode())
    return out


def dare_vjp_batched(A, B, Q, R, P, g_P, device=0, want=("A", "B", "Q", "R"), init=None):
    """dare_vjp for a batch on the GPU (almpc_dare_vjp_batched): A, P, g_P (batch, n, n), B (batch, n, m), shared Q, R.  Returns
    ({group: array (batch, ...)} for the groups `want` names, status (batch,) int32); status 0 = followed, else the slots i are what
    init[group] held (NaN without init)."""
    L = load()
    A, B, P, g_P = (np.asarray(a, dtype=np.float64) for a in (A, B, P, g_P))
    if A.ndim != 3 or B.ndim != 3 or A.shape[0] != B.shape[0] or A.shape[1] != A.shape[2] or B.shape[1] != A.shape[1]:
        raise ValueError(f"expected A (batch, n, n) and B (batch, n, m), got {A.shape} and {B.shape}")
    b, n, m = B.shape
    if P.shape != (b, n, n) or g_P.shape != (b, n, n):
        raise ValueError(f"expected P and g_P {(b, n, n)}, got {P.shape} and {g_P.shape}")
    cm = lambda a: _blocks(a, *a.shape)
    Q, R = _colmajor(Q, (n, n)), _colmajor(R, (m, m))
    shapes = {"A": (b, n, n), "B": (b, n, m), "Q": (b, n, n), "R": (b, m, m)}
    out = {}
    for k in want:
        out[k] = np.full(shapes[k], np.nan).transpose(0, 2, 1).copy() if init is None or k not in init else \
            _blocks(init[k], *shapes[k])
    st = np.zeros(b, dtype=np.int32)
    rc = L.almpc_dare_vjp_batched(int(device), n, m, b, _ptr(cm(A)), _ptr(cm(B)), _ptr(Q), _ptr(R), _ptr(cm(P)), _ptr(cm(g_P)),
                                  *(_ptr(out.get(k)) for k in ("A", "B", "Q", "R")), st.ctypes.data_as(_ip))
    if rc != ALMPC_OK:
        raise AlmpcError(rc, "almpc_dare_vjp_batched")
    return {k: np.ascontiguousarray(v.transpose(0, 2, 1)) for k, v in out.items()}, st


TERMINAL_WEIGHT_MODES = {"given": 0, "dare_device": 1}  # almpc.h: ALMPC_TERMINAL_*


def _terminal_mode(mode):
    if isinstance(mode, str):
        if mode not in TERMINAL_WEIGHT_MODES:
            raise ValueError(f"unknown terminal-weight mode {mode!r}; choose from {sorted(TERMINAL_WEIGHT_MODES)}")
        return TERMINAL_WEIGHT_MODES[mode]
    return int(mode)


def dare_batched(A, B, Q, R, device=0, P_init=None):
    """P_i = DARE(A_i, B_i, Q, R) on the GPU (almpc_dare_batched): A (batch, n, n), B (batch, n, m), shared Q, R.  Returns
    (P (batch, n, n), status (batch,) int32); status 0 = solved, else slot i of P is what P_init held (NaN without P_init)."""
    L = load()
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if A.ndim != 3 or B.ndim != 3 or A.shape[0] != B.shape[0] or A.shape[1] != A.shape[2] or B.shape[1] != A.shape[1]:
        raise ValueError(f"expected A (batch, n, n) and B (batch, n, m), got {A.shape} and {B.shape}")
    b, n, m = B.shape
    Ac, Bc = _blocks(A, b, n, n), _blocks(B, b, n, m)
    Q, R = _colmajor(Q, (n, n)), _colmajor(R, (m, m))
    if P_init is None:
        P = np.full((b, n, n), np.nan)
    else:
        P = _blocks(P_init, b, n, n)
    st = np.zeros(b, dtype=np.int32)
    rc = L.almpc_dare_batched(int(device), n, m, b, _ptr(Ac), _ptr(Bc), _ptr(Q), _ptr(R), _ptr(P), st.ctypes.data_as(_ip))
    if rc != ALMPC_OK:
        raise AlmpcError(rc, "almpc_dare_batched")
    return np.ascontiguousarray(P.transpose(0, 2, 1)), st


MODEL_TIME_MODES = {"discrete": 0, "continuous": 1}  # almpc.h: ALMPC_MODEL_*


def _model_time_mode(mode):
    if isinstance(mode, str):
        if mode not in MODEL_TIME_MODES:
            raise ValueError(f"unknown model-time mode {mode!r}; choose from {sorted(MODEL_TIME_MODES)}")
        return MODEL_TIME_MODES[mode]
    return int(mode)


def c2d(A, B, Ts):
    """Exact zero-order hold of x' = A x + B u at the sample time Ts (almpc_c2d, host math): returns (A_d, B_d)."""
    L = load()
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(n, -1)
    m = B.shape[1]
    A, B = _colmajor(A, (n, n)), _colmajor(B, (n, m))
    Ad, Bd = np.empty((n, n), order="F"), np.empty((n, m), order="F")
    rc = L.almpc_c2d(n, m, _ptr(A), _ptr(B), float(Ts), _ptr(Ad), _ptr(Bd))
    if rc != ALMPC_OK:
        raise AlmpcError(rc, "almpc_c2d")
    return Ad, Bd


def c2d_batched(A, B, Ts, device=0, out_init=None):
    """Zero-order hold of a batch of continuous-time models on the GPU (almpc_c2d_batched): A (batch, n, n), B (batch, n, m), one
    sample time.  Returns (A_d (batch, n, n), B_d (batch, n, m), status (batch,) int32); status 0 = discretised, else slots i of A_d
    and B_d are what out_init = (A_init, B_init) held (NaN without out_init)."""
    L = load()
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if A.ndim != 3 or B.ndim != 3 or A.shape[0] != B.shape[0] or A.shape[1] != A.shape[2] or B.shape[1] != A.shape[1]:
        raise ValueError(f"expected A (batch, n, n) and B (batch, n, m), got {A.shape} and {B.shape}")
    b, n, m = B.shape
    Ac, Bc = _blocks(A, b, n, n), _blocks(B, b, n, m)
    if out_init is None:
        Ad, Bd = np.full((b, n, n), np.nan), np.full((b, m, n), np.nan)
    else:
        Ad, Bd = _blocks(out_init[0], b, n, n), _blocks(out_init[1], b, n, m)
    st = np.zeros(b, dtype=np.int32)
    rc = L.almpc_c2d_batched(int(device), n, m, b, _ptr(Ac), _ptr(Bc), float(Ts), _ptr(Ad), _ptr(Bd), st.ctypes.data_as(_ip))
    if rc != ALMPC_OK:
        raise AlmpcError(rc, "almpc_c2d_batched")
    return np.ascontiguousarray(Ad.transpose(0, 2, 1)), np.ascontiguousarray(Bd.transpose(0, 2, 1)), st


FNN_ACTIVATIONS = {"identity": 0, "relu": 1, "tanh": 2, "sigmoid": 3, "swish": 4}
# network kinds in the Fnn weight layout (include/almpc.h ALMPC_NET_*): only the hidden-layer recurrence differs
NET_KINDS = {"fnn", "resnet", "polynet"}
_NET_CODES = {"fnn": 0, "resnet": 1, "polynet": 2}


def net_code(net="fnn", act="relu"):
    """ALMPC_NET_CODE(kind, activation): the `activation` argument of the network calls (a bare activation for an Fnn)."""
    if net not in NET_KINDS:
        raise ValueError(f"net must be one of {sorted(NET_KINDS)}, not {net!r}")
    return (_NET_CODES[net] << 8) | FNN_ACTIVATIONS[act]


SQP_HESSIANS = {"gauss_newton": 0, "exact": 1}   # almpc_sqp_fnn_set_hessian


def _pack_densenet(W_in, W_h, b_h, W_out, n=None, m=None):
    """The DenseNet buffers of include/almpc.h: W_in (H, n+m), W_h[l] (H, (l+1) H) packed column-major one after another, b_h[l] (H,),
    W_out (n, (L+1) H).  ValueError on any shape that does not fit (n, m: the handle's, when given).  -> H, L, W_in, W_h, b_h, W_out"""
    W_in, W_out = np.asfortranarray(W_in, dtype=np.float64), np.asfortranarray(W_out, dtype=np.float64)
    if W_in.ndim != 2 or W_out.ndim != 2:
        raise ValueError("DenseNet: W_in and W_out must be matrices")
    H, nin = W_in.shape
    W_h, b_h = [np.asarray(w, dtype=np.float64) for w in W_h], [np.asarray(v, dtype=np.float64) for v in b_h]
    nl = len(W_h)
    if len(b_h) != nl:
        raise ValueError(f"DenseNet: {nl} hidden weight blocks but {len(b_h)} bias vectors")
    for l, (w, v) in enumerate(zip(W_h, b_h)):
        if w.shape != (H, (l + 1) * H):
            raise ValueError(f"DenseNet: W_h[{l}] must be {(H, (l + 1) * H)}, got {w.shape}")
        if v.shape != (H,):
            raise ValueError(f"DenseNet: b_h[{l}] must be {(H,)}, got {v.shape}")
    if W_out.shape[1] != (nl + 1) * H:
        raise ValueError(f"DenseNet: W_out must have (L+1) H = {(nl + 1) * H} columns, got {W_out.shape}")
    if (n is not None and W_out.shape[0] != n) or (m is not None and nin != n + m) or nin <= W_out.shape[0]:
        raise ValueError(f"DenseNet: W_in {W_in.shape} and W_out {W_out.shape} do not fit n = {n}, m = {m}")
    Wh = np.concatenate([w.ravel(order="F") for w in W_h]) if nl else np.zeros(1)
    bh = np.ascontiguousarray(np.stack(b_h)) if nl else np.zeros((1, 1))
    return H, nl, W_in, Wh, bh, W_out


def _densenet_act(act):
    """the bare activation code of the almpc_*densenet* calls"""
    if act not in FNN_ACTIVATIONS:
        raise ValueError(f"act must be one of {sorted(FNN_ACTIVATIONS)}, not {act!r}")
    return FNN_ACTIVATIONS[act]


def _fnn_buffers(W_in, W_h, b_h, W_out, act, net):
    """The buffers of a network in the Fnn weight layout (include/almpc.h): W_in (H, n+m), W_h[l] (H, H) one after another, b_h[l] (H,),
    W_out (n, H), all column-major (one-element dummies for L = 0).  -> H, L, code, W_in, W_h, b_h, W_out"""
    W_in, W_out = np.asfortranarray(W_in, dtype=np.float64), np.asfortranarray(W_out, dtype=np.float64)
    nl = len(W_h)
    Wh = np.ascontiguousarray(np.stack([np.asfortranarray(W, dtype=np.float64).T for W in W_h])) if nl else np.zeros((1, 1, 1))
    bh = np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.float64) for v in b_h])) if nl else np.zeros((1, 1))
    return W_in.shape[0], nl, net_code(net, act), W_in, Wh, bh, W_out


def _densenet_buffers(W_in, W_h, b_h, W_out, act, n, m):
    """_fnn_buffers for a DenseNet: the layout of _pack_densenet and a bare activation code"""
    H, nl, W_in, Wh, bh, W_out = _pack_densenet(W_in, W_h, b_h, W_out, n, m)
    return H, nl, _densenet_act(act), W_in, Wh, bh, W_out


def _linearize(call, name, device, n, m, net, x, u, want_f):
    H, nl, code, *W = net
    batch = x.shape[0]
    A = np.empty((batch, n, n)); B = np.empty((batch, m, n)); f = np.empty((batch, n)) if want_f else None
    rc = call(int(device), n, m, H, nl, code, *[_ptr(w) for w in W], batch, _ptr(x), _ptr(u), _ptr(A), _ptr(B), _ptr(f))
    if rc != ALMPC_OK:
        raise AlmpcError(rc, name)
    A, B = A.transpose(0, 2, 1), B.transpose(0, 2, 1)  # column-major buffers -> (batch, row, col)
    return (A, B, f) if want_f else (A, B)


def fnn_linearize(W_in, W_h, b_h, W_out, x, u, act="relu", device=0, want_f=False, net="fnn"):
    """Batched Jacobians of a network model on the GPU: x (batch, n), u (batch, m) -> A (batch, n, n), B (batch, n, m).
    net: "fnn", "resnet" or "polynet" (NET_KINDS), all in the Fnn weight layout."""
    net = _fnn_buffers(W_in, W_h, b_h, W_out, act, net)
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
    n = net[6].shape[0]   # (W_out is n x H, W_in H x (n + m))
    return _linearize(load().almpc_fnn_linearize, "almpc_fnn_linearize", device, n, net[3].shape[1] - n, net, x, u, want_f)


def densenet_linearize(W_in, W_h, b_h, W_out, x, u, act="relu", device=0, want_f=False):
    """fnn_linearize for a DenseNet (almpc_densenet_linearize): W_h a list of (H, (l+1) H) blocks, W_out (n, (L+1) H)."""
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
    if u.shape[0] != x.shape[0]:
        raise ValueError("x and u must hold the same number of points")
    net = _densenet_buffers(W_in, W_h, b_h, W_out, act, x.shape[1], u.shape[1])
    return _linearize(load().almpc_densenet_linearize, "almpc_densenet_linearize", device, x.shape[1], u.shape[1], net, x, u, want_f)


class _Form:
    """The C functions of one form of the API -- almpc_<name> for a handle, almpc_group_<name> for a group --, looked up once."""

    def __init__(self, L, prefix):
        for name in _GROUP_FORMS + ("get_results",):
            setattr(self, name, getattr(L, prefix + name))


class _Target:
    """What a handle and a group can both do, written once: self._t is the almpc_handle* or the almpc_group*, self._f the C
    functions of that form.  Host arrays cover the target's whole batch."""

    _PREFIX = None          # of the C functions: "almpc_" or "almpc_group_"
    _NO_U0 = None           # almpc_get_results has no u0 argument, almpc_group_get_results has

    def _bind(self, L, n, m, N, batch):
        self.L = L
        self.n, self.m, self.N, self.batch = int(n), int(m), int(N), int(batch)
        self.nz = self.m * self.N
        self._f = _Form(L, self._PREFIX)
        self._results = _result_table(self.batch, self.n, self.m, self.N)
        self._get_results = {k: v for k, v in self._results.items() if k != "u0"} if self._NO_U0 else self._results
        self._t = None

    def _check(self, rc):
        if rc != ALMPC_OK:
            raise AlmpcError(rc, (self._f.last_error(self._t) or b"").decode())

    # ---- designs
    def design_shared(self, A, B, Q, R, S=None, P=None, umin=None, umax=None, xmin=None, xmax=None, rho=0.1, sigma=1e-6,
                      terminal="none", rho_profile="scalar"):
        """xmin/xmax: state box (the reference's kw mpc_state_constraint); terminal: "none" | "equality";
        rho_profile: "scalar" (OSQP: rho for every row) | "stiffness" (rho_i = rho / (H'^-1)_ii)."""
        n, m = self.n, self.m
        if terminal not in ("none", "equality"):
            raise ValueError("terminal must be 'none' or 'equality'")
        self._check(self._f.set_terminal_equality(self._t, 1 if terminal == "equality" else 0))
        self._check(self._f.set_rho_profile(self._t, _rho_code(rho_profile)))
        A, B, Q, R = _colmajor(A, (n, n)), _colmajor(B, (n, m)), _colmajor(Q, (n, n)), _colmajor(R, (m, m))
        S, P = _optional(_colmajor, S, (m, m)), _optional(_colmajor, P, (n, n))
        umin, umax = _vec(umin, m), _vec(umax, m)
        xmin, xmax = _optional(_vec, xmin, n), _optional(_vec, xmax, n)
        self._check(self._f.design_shared(self._t, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(S), _ptr(P), _ptr(umin), _ptr(umax),
                                          _ptr(xmin), _ptr(xmax), float(rho), float(sigma)))

    def _state_rows(self, xmin, xmax, terminal):
        """State box / terminal equality of the designs without xmin / xmax arguments (almpc_set_state_box, almpc_set_terminal_equality)."""
        if (xmin is None) != (xmax is None):
            raise ValueError("give both xmin and xmax or neither")
        self._check(self._f.set_terminal_equality(self._t, 1 if terminal == "equality" else 0))
        lo, hi = _optional(_vec, xmin, self.n), _optional(_vec, xmax, self.n)
        self._check(self._f.set_state_box(self._t, _ptr(lo), _ptr(hi)))

    def _design_batched(self, design, weight, A_batch, B_batch, Q, R, S, P, umin, umax, rho, sigma, rho_profile, xmin, xmax, terminal):
        """weight(W, k): the conversion of a k x k weight, shared or one per instance"""
        n, m, b = self.n, self.m, self.batch
        self._state_rows(xmin, xmax, terminal)
        self._check(self._f.set_rho_profile(self._t, _rho_code(rho_profile)))
        A, B = _blocks(A_batch, b, n, n), _blocks(B_batch, b, n, m)
        Q, R, S = weight(Q, n), weight(R, m), _optional(weight, S, m)
        P, p_inst = (None, 0) if P is None else _terminal_weight(P, b, n)
        umin, umax = _vec(umin, m), _vec(umax, m)
        self._check(design(self._t, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(S), _ptr(P), p_inst, _ptr(umin), _ptr(umax), float(rho),
                           float(sigma)))

    def design_batched(self, A_batch, B_batch, Q, R, S=None, P=None, umin=None, umax=None, rho=0.1, sigma=1e-6,
                       rho_profile="scalar", xmin=None, xmax=None, terminal="none"):
        """One model per instance: A_batch (batch, n, n), B_batch (batch, n, m).  P: None (DARE per instance), (n, n) shared
        or (batch, n, n).  xmin / xmax: state box (stages 1..N+1); terminal = "equality": e_x[:, N+1] = 0."""
        self._design_batched(self._f.design_batched, lambda W, k: _colmajor(W, (k, k)), A_batch, B_batch, Q, R, S, P, umin, umax, rho,
                             sigma, rho_profile, xmin, xmax, terminal)

    def design_batched_weighted(self, A_batch, B_batch, Q_batch, R_batch, S_batch=None, P=None, umin=None, umax=None, rho=0.1, sigma=1e-6,
                                rho_profile="scalar", xmin=None, xmax=None, terminal="none"):
        """design_batched with one weight set per instance (almpc_design_batched_weighted): Q_batch (batch, n, n), R_batch and
        S_batch (batch, m, m), S_batch None for S = 0 everywhere.  The other arguments are design_batched's."""
        self._design_batched(self._f.design_batched_weighted, lambda W, k: _blocks(W, self.batch, k, k), A_batch, B_batch, Q_batch,
                             R_batch, S_batch, P, umin, umax, rho, sigma, rho_profile, xmin, xmax, terminal)

    def set_terminal_weight(self, mode):
        """Before a design: "given" / 0 (default) or "dare_device" / 1 -- design_batched(P=None) and every relin_fnn step take each
        instance's terminal weight from the DARE of its own model, solved on the device (almpc_set_terminal_weight)."""
        self._check(self._f.set_terminal_weight(self._t, _terminal_mode(mode)))

    def set_model_time(self, mode, Ts=0.0):
        """Before a design: "discrete" / 0 (default) or "continuous" / 1 with the sample time Ts -- the models given to design_shared and
        design_batched, and the network of the relin_fnn pipeline, are continuous-time and are discretised by zero-order hold at Ts
        (almpc_set_model_time)."""
        self._check(self._f.set_model_time(self._t, _model_time_mode(mode), float(Ts)))

    # ---- network models: the SQP loop (almpc_sqp_fnn_*) and the per-step re-linearisation (almpc_relin_fnn_*)
    def _net_setup(self, setup, net, x_ref, u_ref, Q, R, S, P, umin, umax, rho, sigma, rho_profile, xmin, xmax, terminal, qp_solver=None):
        """net: (H, L, code, W_in, W_h, b_h, W_out).  qp_solver None: a relin setup (shared P, no P_per_instance argument)."""
        n, m, N = self.n, self.m, self.N
        self._state_rows(xmin, xmax, terminal)
        if qp_solver is not None:
            self._check(self._f.sqp_fnn_set_structured(self._t, 1 if qp_solver == "structured" else 0))
        self._check(self._f.set_rho_profile(self._t, _rho_code(rho_profile)))
        xr, ur = _optional(_traj, x_ref, n, N + 1), _optional(_traj, u_ref, m, N)
        Q, R, S = _colmajor(Q, (n, n)), _colmajor(R, (m, m)), _optional(_colmajor, S, (m, m))
        if qp_solver is None:
            P, p_inst = _colmajor(P, (n, n)), ()
        else:
            P, p_inst = _terminal_weight(P, self.batch, n)
            p_inst = (p_inst,)
        umin, umax = _vec(umin, m), _vec(umax, m)
        self._check(setup(self._t, *net[:3], *[_ptr(w) for w in net[3:]], _ptr(xr), _ptr(ur), _ptr(Q), _ptr(R), _ptr(S), _ptr(P), *p_inst,
                          _ptr(umin), _ptr(umax), float(rho), float(sigma)))

    def sqp_fnn_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu", rho=0.1,
                      sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none", qp_solver="condensed", net="fnn"):
        """SQP outer loop for a network model (almpc_sqp_fnn_*): network (and net) as in fnn_linearize, x_ref (n, N+1) / u_ref (m, N) or None,
        P (n, n) or (batch, n, n).  qp_solver: "condensed" (default) or "structured" (every QP through k_riccati, no condensed design).  xmin / xmax: the state box of the reference's NLP branch
        (.../fnn/mpc_modeler_implementation_fnn.jl:146-153) as rows of every iteration's QP; terminal = "equality"."""
        self._net_setup(self._f.sqp_fnn_setup, _fnn_buffers(W_in, W_h, b_h, W_out, act, net), x_ref, u_ref, Q, R, S, P, umin, umax, rho,
                        sigma, rho_profile, xmin, xmax, terminal, qp_solver)

    def sqp_densenet_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu",
                           rho=0.1, sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none", qp_solver="condensed"):
        """sqp_fnn_setup for a DenseNet (almpc_sqp_densenet_setup; network as in densenet_linearize); then the sqp_fnn_* calls."""
        self._net_setup(self._f.sqp_densenet_setup, _densenet_buffers(W_in, W_h, b_h, W_out, act, self.n, self.m), x_ref, u_ref, Q, R, S,
                        P, umin, umax, rho, sigma, rho_profile, xmin, xmax, terminal, qp_solver)

    def relin_fnn_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu", rho=0.1,
                        sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none", net="fnn"):
        """Device-resident per-step re-linearisation of a network model (almpc_relin_fnn_*, BASELINE configs[3]): network (and net)
        as in fnn_linearize, shared x_ref (n, N+1) / u_ref (m, N) or None, shared P (n, n); xmin / xmax / terminal as in design_batched."""
        self._net_setup(self._f.relin_fnn_setup, _fnn_buffers(W_in, W_h, b_h, W_out, act, net), x_ref, u_ref, Q, R, S, P, umin, umax, rho,
                        sigma, rho_profile, xmin, xmax, terminal)

    def relin_densenet_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu",
                             rho=0.1, sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none"):
        """relin_fnn_setup for a DenseNet (almpc_relin_densenet_setup; network as in densenet_linearize); then the relin_fnn_* calls."""
        self._net_setup(self._f.relin_densenet_setup, _densenet_buffers(W_in, W_h, b_h, W_out, act, self.n, self.m), x_ref, u_ref, Q, R,
                        S, P, umin, umax, rho, sigma, rho_profile, xmin, xmax, terminal)

    def relin_fnn_step(self, opts: almpc_opts | None = None, sync=True):
        fn = self._f.relin_fnn_step if sync else self._f.relin_fnn_step_async
        self._check(fn(self._t, ctypes.byref(opts) if opts is not None else None))

    def relin_fnn_advance(self):
        """x0 <- fnn(x0, u[:,1]) on the device (closed loop of the black-box model)."""
        self._check(self._f.relin_fnn_advance(self._t))

    def relin_fnn_certificate(self, want=("cost", "res", "grad", "costate")) -> dict:
        """almpc_relin_fnn_certificate + almpc_get_certificate: `certificate` of the last relin_fnn_step, with that step's own models,
        terminal weights and weights."""
        return self._certificate(self._f.relin_fnn_certificate, want)

    def sqp_fnn_start(self, x0, u_guess=None):
        """x0 (batch, n); u_guess (batch, m, N) or None."""
        x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(self.batch, self.n))
        ug = _optional(_traj_batch, u_guess, self.batch, self.m, self.N)
        self._check(self._f.sqp_fnn_start(self._t, _ptr(x0), _ptr(ug)))

    def sqp_fnn_iterate(self, iters, step_scale=1.0, opts=None, step_rule="fixed"):
        """-> (step_inf[iters], defect_inf[iters]); raises AlmpcError(ALMPC_ERR_NUMERIC) when an instance had to skip an iteration
        (the histories are still filled: see .sqp_last).  step_rule: "fixed" | "merit" (l1 merit-function safeguard)."""
        self._check(self._f.sqp_fnn_set_step_rule(self._t, {"fixed": 0, "merit": 1}[step_rule]))
        st, de = np.zeros(int(iters)), np.zeros(int(iters))
        self.sqp_last = (st, de)
        self._check(self._f.sqp_fnn_iterate(self._t, int(iters), float(step_scale), ctypes.byref(opts) if opts is not None else None,
                                            _ptr(st), _ptr(de)))
        return st, de

    def sqp_fnn_solve(self, max_iters, tol, opts=None, step_rule="merit"):
        """Solve to a tolerance (almpc_sqp_fnn_solve): at most max_iters iterations, each instance frozen once its iterate passes the
        first-order test (zero defects, projected adjoint-gradient residual <= tol).  -> dict(status (batch,) int32: 0 converged,
        1 iteration limit, 2 skipped, 3 infeasible QP; iters (batch,) int32; kkt (batch,) residual of the last test).
        The step rule is a setting of the handle and stays in force: a later sqp_fnn_iterate sets its own (default "fixed")."""
        self._check(self._f.sqp_fnn_set_step_rule(self._t, {"fixed": 0, "merit": 1}[step_rule]))
        st, it, kk = np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch)
        self._check(self._f.sqp_fnn_solve(self._t, int(max_iters), float(tol), ctypes.byref(opts) if opts is not None else None,
                                          st.ctypes.data_as(_ip), it.ctypes.data_as(_ip), _ptr(kk)))
        return dict(status=st, iters=it, kkt=kk)

    def sqp_fnn_set_hessian(self, mode):
        """Hessian of the loop's QPs: "gauss_newton" (default) or "exact" (almpc_sqp_fnn_set_hessian); stays in force."""
        self._check(self._f.sqp_fnn_set_hessian(self._t, SQP_HESSIANS[mode]))

    def sqp_fnn_set_row_multipliers(self, on):
        """State rows (state box, terminal equality) in the loop's stopping test and exact Hessian: the finishes hand the row multipliers
        of every iteration's QP out (almpc_sqp_fnn_set_row_multipliers; default off, stays in force)."""
        self._check(self._f.sqp_fnn_set_row_multipliers(self._t, 1 if on else 0))

    def sqp_fnn_state_multipliers(self):
        """-> (batch, n, N): multiplier of the row of x_{k+1}[i] at [:, i, k] in each instance's last solved QP (> 0 upper bound, < 0 lower
        bound, free on a terminal-equality row, 0 outside the working set); zeros with the switch off or without state rows."""
        mu = np.zeros((self.batch, self.N, self.n))
        self._check(self._f.sqp_fnn_state_multipliers(self._t, _ptr(mu)))
        return np.ascontiguousarray(mu.transpose(0, 2, 1))

    def sqp_fnn_skipped(self):
        out = np.zeros(self.batch, dtype=np.int32)
        self._check(self._f.sqp_fnn_skipped(self._t, out.ctypes.data_as(_ip)))
        return out

    # ---- the step
    def set_reference(self, x_ref, u_ref, per_instance=False):
        """x_ref (n, N+1) / u_ref (m, N), or with per_instance (batch, n, N+1) / (batch, m, N)."""
        n, m, N = self.n, self.m, self.N
        if per_instance:
            xr, ur = _traj_batch(x_ref, self.batch, n, N + 1), _traj_batch(u_ref, self.batch, m, N)
        else:
            xr, ur = _traj(x_ref, n, N + 1), _traj(u_ref, m, N)
        self._check(self._f.set_reference(self._t, _ptr(xr), _ptr(ur), 1 if per_instance else 0))

    def update_initialization(self, x0):
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(self.batch, self.n)
        self._check(self._f.update_initialization(self._t, _ptr(x0)))

    def calculate(self, opts: almpc_opts | None = None, sync=True):
        fn = self._f.calculate if sync else self._f.calculate_async
        self._check(fn(self._t, None if opts is None else ctypes.byref(opts)))

    def synchronize(self):
        self._check(self._f.synchronize(self._t))

    def advance_plant(self):
        self._check(self._f.advance_plant(self._t))

    def get_results(self, want=("x", "e_x", "u", "e_u", "status", "iters", "polish_iters")):
        """The last step's results, Julia-shaped: x, e_x (batch, n, N+1), u, e_u (batch, m, N), status, iters, polish_iters (batch,)."""
        bufs, args = _result_bufs(self._get_results, want)
        self._check(self._f.get_results(self._t, *args))
        return bufs

    def get_results_async(self, want=("u0", "status")) -> int:
        """Ask for results of the last enqueued step (names of WANT; "u0" = u[:, 1] of every instance); returns a ticket."""
        t = self._f.get_results_async(self._t, _want_mask(want))
        if t < 0:
            self._check(t)
        return t

    def get_results_wait(self, ticket, want=("u0", "status")):
        """Results of a ticket in fresh arrays (almpc_get_results_wait).  Shapes as get_results; u0 (batch, m)."""
        _want_mask(want)
        bufs, args = _result_bufs(self._results, want)
        self._check(self._f.get_results_wait(self._t, int(ticket), *args))
        return bufs

    # ---- sensitivities of the last step to x0 (include/almpc.h "Sensitivities"; an extension beyond the reference's surface)
    def _sensitivity(self, call, want, *tols):
        self._check(call(self._t, _sens_mask(want), *[float(t) for t in tols]))
        return _sens_read(self._f.get_sensitivity, self._t, self._check, want, self.batch, self.n, self.m, self.N)

    def _vjp(self, call, g_u, g_x, act_tol):
        return _sens_vjp(call, self._t, self._check, g_u, g_x, act_tol, self.batch, self.n, self.m, self.N)

    def sensitivity(self, want=("K0", "dU", "dX"), act_tol=0.0) -> dict:
        """almpc_sensitivity + almpc_get_sensitivity: K0 (batch, m, n) = du[:,1]/dx0, dU (batch, m, N, n), dX (batch, n, N+1, n),
        each [b, i, k, c] = d(entry i of stage k) / d x0[c], and rows (batch,) = rows at a bound (-1: instance not solved, zeros).
        act_tol <= 0: 1e-9 (in units of the row's Jacobi scale)."""
        return self._sensitivity(self._f.sensitivity, want, act_tol)

    def sensitivity_vjp(self, g_u, g_x=None, act_tol=0.0):
        """dL/dx0 (batch, n) for a loss with gradients g_u (batch, m, N) and g_x (batch, n, N+1) or None on the returned
        trajectories (almpc_sensitivity_vjp: no Jacobian is formed); also returns rows (batch,)."""
        return self._vjp(self._f.sensitivity_vjp, g_u, g_x, act_tol)

    def sensitivity_stagewise(self, want=("K0", "dU", "dX"), act_tol=0.0) -> dict:
        """sensitivity on a structured handle (almpc_sensitivity_stagewise + almpc_get_sensitivity): the Riccati recursion on the face
        where the inputs at a bound are held; input box only, S = 0.  act_tol is relative to the width of the input box (0: 1e-7)."""
        return self._sensitivity(self._f.sensitivity_stagewise, want, act_tol)

    def sensitivity_stagewise_vjp(self, g_u, g_x=None, act_tol=0.0):
        """sensitivity_vjp on a structured handle (almpc_sensitivity_stagewise_vjp): (g_x0 (batch, n), rows (batch,))."""
        return self._vjp(self._f.sensitivity_stagewise_vjp, g_u, g_x, act_tol)

    def sensitivity_stagewise_rate(self, want=("K0", "dU", "dX"), act_tol=0.0) -> dict:
        """sensitivity_stagewise for every structured input-box design, with or without an input-rate weight S
        (almpc_sensitivity_stagewise_rate + almpc_get_sensitivity): with S the recursion runs in the stage state [dx_k; du_(k-1)]
        (k_sens_face_rate), without it the call is sensitivity_stagewise to the byte."""
        return self._sensitivity(self._f.sensitivity_stagewise_rate, want, act_tol)

    def sensitivity_stagewise_rate_vjp(self, g_u, g_x=None, act_tol=0.0):
        """sensitivity_stagewise_vjp for designs with or without S (almpc_sensitivity_stagewise_rate_vjp): (g_x0 (batch, n), rows (batch,))."""
        return self._vjp(self._f.sensitivity_stagewise_rate_vjp, g_u, g_x, act_tol)

    def sensitivity_rows(self, want=("K0", "dU", "dX"), act_tol_u=0.0, act_tol_x=0.0) -> dict:
        """sensitivity for shared designs with a state box and / or the terminal equality as well (almpc_sensitivity_rows +
        almpc_get_sensitivity): rows counts input, state-box and terminal-equality rows at a bound; act_tol_x is the state rows'
        threshold (0: 1e-7, relative to max(1, |bound|)).  Without state rows it is sensitivity(want, act_tol_u), bit for bit."""
        return self._sensitivity(self._f.sensitivity_rows, want, act_tol_u, act_tol_x)

    def sensitivity_rows_vjp(self, g_u, g_x=None, act_tol_u=0.0, act_tol_x=0.0):
        """sensitivity_vjp in the rows form (almpc_sensitivity_rows_vjp): (g_x0 (batch, n), rows (batch,))."""
        return self._vjp(self._f.sensitivity_rows_vjp, g_u, g_x, (act_tol_u, act_tol_x))

    def sensitivity_params_vjp(self, g_u, g_x=None, want=PARAM_GROUPS, act_tol=0.0, terminal="data") -> dict:
        """Gradients of the loss of sensitivity_vjp in the problem data, per instance (almpc_sensitivity_params_vjp): x0, the QP's
        linear term f, u_ref, the input box, the weights Q, P, R, S and the model A, B -- what `want` names -- and rows.  For a shared
        design the caller sums over the batch.  terminal="data": P is data; "dare" (almpc_sensitivity_params_vjp_dare): P_i =
        DARE(A_i, B_i, Q, R) is followed into Q, R, A, B, and the dict also carries dare_status (batch,): 0 followed, else the
        instance keeps its P-as-data values (its P is not the stabilising DARE solution of the design's model)."""
        dare = _terminal_gradient(terminal)
        call = self._f.sensitivity_params_vjp_dare if dare else self._f.sensitivity_params_vjp
        return _sens_params_vjp(call, self._t, self._check, g_u, g_x, want, act_tol, self.batch, self.n, self.m, self.N, dare)

    # ---- certificate of the last step (include/almpc.h "Certificate of the last step")
    def _certificate(self, call, want):
        self._check(call(self._t, _cert_mask(want)))
        return _cert_read(self._f.get_certificate, self._t, self._check, want, self.batch, self.n, self.m, self.N)

    def certificate(self, want=("cost", "res", "grad", "costate")) -> dict:
        """almpc_certificate + almpc_get_certificate: cost (batch,) the objective value, res (batch,) the KKT residual of the returned
        inputs, grad (batch, m, N) the gradient of the objective in the inputs, costate (batch, n, N+1) (costate[:, :, 0] = dJ/dx0).
        From the returned trajectories alone: every instance is certified whatever its status."""
        return self._certificate(self._f.certificate, want)


class Solver(_Target):
    """Thin object wrapper of an almpc_handle: one device, one batch shard."""

    _PREFIX = "almpc_"
    _NO_U0 = True

    def __init__(self, n, m, N, batch, device=0, timing=False, structured=False, structured_fallback=None):
        """structured: ALMPC_FLAG_STRUCTURED (the stage-wise solve of the multiple-shooting form is the handle's solver: no m*N <= 128
        limit).  structured_fallback: the redo of the instances a condensed step leaves without a certificate by the stage-wise
        solvers -- None: the library default (on wherever they cover the design), True: required, False: off."""
        self._bind(load(), n, m, N, batch)
        h = _hp()
        rc = self.L.almpc_create(ctypes.byref(h), self.n, self.m, self.N, self.batch, int(device),
                                 (FLAG_TIMING if timing else 0) | (FLAG_STRUCTURED if structured else 0))
        if rc != ALMPC_OK:
            raise AlmpcError(rc, "almpc_create failed (is a gfx950 GPU visible? there is no CPU fallback)")
        self.h = self._t = h
        if structured_fallback is not None:
            self._check(self.L.almpc_set_structured_fallback(self.h, 1 if structured_fallback else 0))

    def close(self):
        if getattr(self, "h", None):
            self.L.almpc_destroy(self.h)
            self.h = self._t = None

    __del__ = close

    # ---- what a design leaves on the handle
    def get_weights_instance(self, i):
        """dict(Q (n, n), R (m, m), S (m, m)): the weights instance i is designed on, as the design kernels read them
        (almpc_get_weights_instance)."""
        Q, R, S = np.empty((self.n, self.n), order="F"), np.empty((self.m, self.m), order="F"), np.empty((self.m, self.m), order="F")
        self._check(self.L.almpc_get_weights_instance(self.h, int(i), _ptr(Q), _ptr(R), _ptr(S)))
        return dict(Q=Q, R=R, S=S)

    def get_gradient_instance(self, i):
        q = np.empty(self.nz)
        self._check(self.L.almpc_get_gradient_instance(self.h, int(i), _ptr(q)))
        return q

    def get_design_instance(self, i):
        n, nz = self.n, self.nz
        H = np.empty((nz, nz), order="F"); F = np.empty((nz, n), order="F"); d = np.empty(nz)
        self._check(self.L.almpc_get_design_instance(self.h, int(i), _ptr(H), _ptr(F), _ptr(d)))
        return dict(H=H, F=F, d=d)

    def get_design(self):
        n, nz = self.n, self.nz
        H = np.empty((nz, nz), order="F"); F = np.empty((nz, n), order="F"); P = np.empty((n, n), order="F"); d = np.empty(nz)
        self._check(self.L.almpc_get_design(self.h, _ptr(H), _ptr(F), _ptr(P), _ptr(d)))
        return dict(H=H, F=F, P=P, d=d)

    def terminal_weight_instance(self, i):
        """(n, n) terminal weight instance i was designed with (almpc_get_terminal_weight_instance)."""
        P = np.empty((self.n, self.n), order="F")
        self._check(self.L.almpc_get_terminal_weight_instance(self.h, int(i), _ptr(P)))
        return P

    def model_instance(self, i):
        """(A (n, n), B (n, m)): the DISCRETE model instance i is designed on (almpc_get_model_instance)."""
        A, B = np.empty((self.n, self.n), order="F"), np.empty((self.n, self.m), order="F")
        self._check(self.L.almpc_get_model_instance(self.h, int(i), _ptr(A), _ptr(B)))
        return A, B

    def relin_terminal_status(self):
        """(batch,) int32 of the last relin_fnn step with the mode on: 0 = the instance's own DARE solution, 1 = the setup's P."""
        out = np.zeros(self.batch, dtype=np.int32)
        self._check(self.L.almpc_relin_fnn_terminal_status(self.h, out.ctypes.data_as(_ip)))
        return out

    # ---- time-varying designs and their certificate (include/almpc.h "Certificate of a step of a time-varying design")
    def set_keep_stage_models(self, on=True):
        """almpc_set_keep_stage_models: the next design_ltv keeps its stage models on the device for certificate_ltv
        (batch N n (n + m + 1) doubles of device memory)."""
        self._check(self.L.almpc_set_keep_stage_models(self.h, 1 if on else 0))

    def design_ltv(self, A_all, B_all, c_all, xbar, ubar, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, rho=0.1, sigma=1e-6,
                   rho_profile="scalar", xmin=None, xmax=None, terminal="none", keep_stage_models=None):
        """Time-varying models: A_all (batch, N, n, n), B_all (batch, N, n, m), c_all (batch, N, n) or None, xbar (batch, n, N+1),
        ubar (batch, m, N), x_ref (n, N+1) / u_ref (m, N) or None, P (n, n) or (batch, n, n).  The QP variable is v = u - ubar.
        xmin / xmax: state box on xbar + dx (stages 1..N+1); terminal = "equality": xbar + dx = x_ref at stage N+1.
        keep_stage_models: None leaves the handle's switch as it is; True / False sets it first (set_keep_stage_models)."""
        n, m, N, b = self.n, self.m, self.N, self.batch
        if keep_stage_models is not None:
            self.set_keep_stage_models(keep_stage_models)
        self._state_rows(xmin, xmax, terminal)
        self._check(self.L.almpc_set_rho_profile(self.h, _rho_code(rho_profile)))
        A, B = _blocks(A_all, b * N, n, n), _blocks(B_all, b * N, n, m)
        c = None if c_all is None else np.ascontiguousarray(np.asarray(c_all, dtype=np.float64).reshape(b, N, n))
        xb, ub = _traj_batch(xbar, b, n, N + 1), _traj_batch(ubar, b, m, N)
        xr, ur = _optional(_traj, x_ref, n, N + 1), _optional(_traj, u_ref, m, N)
        Q, R, S = _colmajor(Q, (n, n)), _colmajor(R, (m, m)), _optional(_colmajor, S, (m, m))
        P, p_inst = _terminal_weight(P, b, n)
        umin, umax = _vec(umin, m), _vec(umax, m)
        self._check(self.L.almpc_design_ltv(self.h, _ptr(A), _ptr(B), _ptr(c), _ptr(xb), _ptr(ub), _ptr(xr), _ptr(ur), _ptr(Q), _ptr(R),
                                            _ptr(S), _ptr(P), p_inst, _ptr(umin), _ptr(umax), float(rho), float(sigma)))

    def _ltv_stage_data(self, A_all, B_all, c_all, xbar, ubar, on_device):
        """The five trajectory arrays of design_ltv_stagewise / ltv_stagewise_update as the C call takes them, and what keeps them alive.
        Host form: numpy arrays in design_ltv's shapes.  Device form: integer device addresses (c_all: None or an address) of float64
        memory in the C layout -- A_all [batch][N][n*n] and B_all [batch][N][n*m] column-major blocks, c_all [batch][N][n],
        xbar [batch][N+1][n], ubar [batch][N][m]."""
        n, m, N, b = self.n, self.m, self.N, self.batch
        if on_device:
            for name, a in (("A_all", A_all), ("B_all", B_all), ("xbar", xbar), ("ubar", ubar)):
                if not isinstance(a, (int, np.integer)) or int(a) == 0:
                    raise TypeError(f"on_device=True: {name} must be a non-zero integer device address")
            if c_all is not None and not isinstance(c_all, (int, np.integer)):
                raise TypeError("on_device=True: c_all must be None or an integer device address")
            dev = lambda a: None if a is None else ctypes.cast(ctypes.c_void_p(int(a)), _dp)
            return [dev(A_all), dev(B_all), dev(c_all), dev(xbar), dev(ubar)], None
        A, B = _blocks(A_all, b * N, n, n), _blocks(B_all, b * N, n, m)
        c = None if c_all is None else np.ascontiguousarray(np.asarray(c_all, dtype=np.float64).reshape(b, N, n))
        xb, ub = _traj_batch(xbar, b, n, N + 1), _traj_batch(ubar, b, m, N)
        keep = (A, B, c, xb, ub)
        return [_ptr(a) for a in keep], keep

    def design_ltv_stagewise(self, A_all, B_all, c_all, xbar, ubar, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None,
                             xmin=None, xmax=None, terminal="none", on_device=False):
        """design_ltv's problem on the stage-wise solvers of a structured handle (almpc_design_ltv_stagewise): no m N <= 128 limit, no
        rho / sigma.  Arrays as design_ltv takes them, or with on_device=True the five trajectory arrays as integer device addresses
        (see _ltv_stage_data for the layout; e.g. torch tensors' data_ptr()).  Weights, references, P and bounds are host arrays in
        both forms.  get_results() then has every output: u = ubar + v, e_u = v, x = xbar + dx, e_x = dx.  No group form."""
        n, m, b = self.n, self.m, self.batch
        self._state_rows(xmin, xmax, terminal)
        data, keep = self._ltv_stage_data(A_all, B_all, c_all, xbar, ubar, on_device)
        xr, ur = _optional(_traj, x_ref, n, self.N + 1), _optional(_traj, u_ref, m, self.N)
        Q, R, S = _colmajor(Q, (n, n)), _colmajor(R, (m, m)), _optional(_colmajor, S, (m, m))
        P, p_inst = _terminal_weight(P, b, n)
        umin, umax = _vec(umin, m), _vec(umax, m)
        self._check(self.L.almpc_design_ltv_stagewise(self.h, *data, _ptr(xr), _ptr(ur), _ptr(Q), _ptr(R), _ptr(S), _ptr(P), p_inst,
                                                      _ptr(umin), _ptr(umax), 1 if on_device else 0))
        del keep

    def ltv_stagewise_update(self, A_all, B_all, c_all, xbar, ubar, on_device=False):
        """New trajectory data into the design of design_ltv_stagewise (almpc_ltv_stagewise_update): the per-iteration call of a
        caller's outer loop.  With on_device=True nothing is waited for: the arrays must be complete before the call and may be
        overwritten after synchronize().  c_all is None exactly when the design's was."""
        data, keep = self._ltv_stage_data(A_all, B_all, c_all, xbar, ubar, on_device)
        self._check(self.L.almpc_ltv_stagewise_update(self.h, *data, 1 if on_device else 0))
        del keep

    def ltv_stagewise_prepared(self, eq_target=False) -> dict:
        """What k_ltv_stage_prepare left for the current data (almpc_get_ltv_stagewise_prepared): ebar (batch, N, n), qadd (batch, N, m)
        and, when asked for (designs with the terminal equality), eq_target (n,)."""
        b, n, m, N = self.batch, self.n, self.m, self.N
        out = dict(ebar=np.empty((b, N, n)), qadd=np.empty((b, N, m)))
        eq = np.empty(n) if eq_target else None
        self._check(self.L.almpc_get_ltv_stagewise_prepared(self.h, _ptr(out["ebar"]), _ptr(out["qadd"]), _ptr(eq)))
        if eq is not None:
            out["eq_target"] = eq
        return out

    def certificate_ltv(self, want=("cost", "res", "grad", "costate", "x", "e_x")) -> dict:
        """almpc_certificate_ltv + almpc_get_certificate_ltv after design_ltv(keep_stage_models=True) and a step: cost (batch,), res (batch,),
        grad (batch, m, N), costate (batch, n, N+1) (costate[:, :, k+1] = dJ/dc_k), x (batch, n, N+1) the predicted states xbar + dx and
        e_x = x - x_ref, for what `want` names ("x" and "e_x" come together)."""
        mask = _cert_mask(want, CERT_LTV)
        self._check(self.L.almpc_certificate_ltv(self.h, mask))
        b, n, m, N = self.batch, self.n, self.m, self.N
        names = (want,) if isinstance(want, str) else tuple(want)
        sizes = dict(cost=(b,), res=(b,), grad=(b, N, m), costate=(b, N + 1, n), x=(b, N + 1, n), e_x=(b, N + 1, n))
        bufs = {k: (np.empty(sizes[k]) if k in names else None) for k in sizes}
        self._check(self.L.almpc_get_certificate_ltv(self.h, *[_ptr(bufs[k]) for k in ("cost", "res", "grad", "costate", "x", "e_x")]))
        return {k: (v if v.ndim == 1 else v.transpose(0, 2, 1)) for k, v in bufs.items() if v is not None}

    def sensitivity_ltv(self, want=("K0", "dU", "dX"), act_tol=0.0) -> dict:
        """Sensitivities of the last step of a design_ltv(keep_stage_models=True) design in its initial deviation (almpc_sensitivity_ltv +
        almpc_get_sensitivity, k_sens_ltv): the face recursion with the stage models A_k, B_k; shapes as sensitivity_stagewise.  K0 is
        the gain of a real-time iteration: apply clip(u_0 + K0 (x_meas - xbar_0)).  act_tol is relative to the width of the input box
        (0: 1e-7)."""
        return self._sensitivity(self.L.almpc_sensitivity_ltv, want, act_tol)

    def sensitivity_ltv_vjp(self, g_u, g_x=None, act_tol=0.0):
        """sensitivity_vjp of the same step (almpc_sensitivity_ltv_vjp): g_x is a loss gradient on the predicted states xbar + dx of
        certificate_ltv; (g_x0 (batch, n), rows (batch,))."""
        return self._vjp(self.L.almpc_sensitivity_ltv_vjp, g_u, g_x, act_tol)

    def relin_fnn_timing(self):
        a, d, s = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        self._check(self.L.almpc_relin_fnn_timing(self.h, ctypes.byref(a), ctypes.byref(d), ctypes.byref(s)))
        return dict(jacobian_ms=a.value, design_ms=d.value, step_ms=s.value)

    # ---- multi-GPU (RCCL inside the library): one process per GPU, one handle per process
    def comm_init(self, unique_id: bytes, rank: int, world: int):
        if len(unique_id) != 128:
            raise ValueError("the RCCL unique id is 128 bytes (comm_unique_id() on rank 0)")
        self._check(self.L.almpc_comm_init(self.h, unique_id, int(rank), int(world)))
        self._comm_world = int(world)

    def comm_summary(self):
        out = (ctypes.c_int64 * 4)()
        self._check(self.L.almpc_comm_summary(self.h, out))
        return dict(ranks=int(out[0]), unsolved=int(out[1]), admm_iters_max=int(out[2]), polish_iters_max=int(out[3]))

    def comm_allgather_first_input(self):
        """u[:, 1] of every instance of every rank: (world, batch, m)."""
        out = np.empty((self._comm_world, self.batch, self.m))
        self._check(self.L.almpc_comm_allgather_first_input(self.h, _ptr(out), None))
        return out

    def start_from(self, other: "Solver"):
        """Structured handle: the next calculate starts from `other`'s last inputs (same batch, horizon <= this one's): horizon
        continuation / chaining of solvers (almpc_set_start_from)."""
        self._check(self.L.almpc_set_start_from(self.h, other.h))

    def set_step_fusion(self, on: bool):
        """One kernel per step (default) or the two-kernel path whose stage times can be told apart."""
        self._check(self.L.almpc_set_step_fusion(self.h, 1 if on else 0))

    def update_initialization_device(self, dev_ptr: int):
        self._check(self.L.almpc_update_initialization_device(self.h, ctypes.c_void_p(dev_ptr)))

    # ---- host-facing step path: pinned staging, transfers on copy streams (include/almpc.h "Host-facing step path")
    def update_initialization_async(self, x0):
        """x0 (batch, n) -> pinned slot -> upload on the copy-in stream; the next calculate waits for it on the device."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(self.batch, self.n)
        self._check(self.L.almpc_update_initialization_async(self.h, _ptr(x0)))

    def x0_staging(self):
        """Zero-copy input (almpc_x0_staging): a (batch, n) view of the pinned slot the next update_initialization_async will use.
        Fill it in place and pass it to update_initialization_async: no staging copy."""
        ptr = _dp()
        self._check(self.L.almpc_x0_staging(self.h, ctypes.byref(ptr)))
        return np.ctypeslib.as_array(ptr, shape=(self.batch, self.n))

    _results_copy = _Target.get_results_wait

    def get_results_wait(self, ticket, want=("u0", "status"), copy=True):
        """Results of a ticket.  copy=True: fresh arrays (almpc_get_results_wait); copy=False: views of the handle's pinned slot
        (almpc_host_results: zero-copy, valid until two more requests).  Shapes as get_results; u0 (batch, m)."""
        if copy:
            return self._results_copy(ticket, want)
        want = set(want)
        _want_mask(want)
        self._check(self.L.almpc_get_results_wait(self.h, int(ticket), *([None] * 8)))
        ps = [ctypes.c_void_p() for _ in self._results]
        self._check(self.L.almpc_host_results(self.h, int(ticket), *[ctypes.byref(q) for q in ps]))
        bufs = {}
        for k, q in zip(self._results, ps):
            if k in want:
                if not q.value:
                    raise AlmpcError(-1, f"result {k!r} was not part of the request of ticket {ticket}")
                shape, dtype, ptype = self._results[k]
                a = np.ctypeslib.as_array(ctypes.cast(q.value, ptype), shape=(int(np.prod(shape)),)).reshape(shape)
                bufs[k] = a.transpose(0, 2, 1) if len(shape) == 3 else a
        return bufs

    def get_first_input(self):
        """u[:, 1] of every instance, (batch, m): what a receding-horizon caller applies (almpc_get_first_input)."""
        u0 = np.empty((self.batch, self.m))
        self._check(self.L.almpc_get_first_input(self.h, _ptr(u0)))
        return u0

    # ---- device pointers of the last results (valid until the next call that computes them)
    def _device_views(self, call, names):
        ps = [ctypes.c_void_p() for _ in names]
        self._check(call(self.h, *[ctypes.byref(p) for p in ps]))
        return dict(zip(names, [p.value for p in ps]))

    def device_results(self):
        return self._device_views(self.L.almpc_device_results, ("x", "e_x", "u", "e_u"))

    def device_sensitivity(self):
        return self._device_views(self.L.almpc_device_sensitivity, ("K0", "dU", "dX", "rows"))

    def device_certificate(self):
        return self._device_views(self.L.almpc_device_certificate, ("cost", "res", "grad", "costate"))

    def device_certificate_ltv(self):
        return self._device_views(self.L.almpc_device_certificate_ltv, ("cost", "res", "grad", "costate", "x", "e_x"))

    # ---- timing (ALMPC_FLAG_TIMING) and test hooks
    def get_timing(self):
        v = [ctypes.c_float() for _ in range(4)]
        self._check(self.L.almpc_get_timing(self.h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("admm_ms", "polish_ms", "rollout_ms", "total_ms"), [x.value for x in v]))

    def debug_poison_lds(self):
        self._check(self.L.almpc_debug_poison_lds(self.h))

    def timing_set_stride(self, every):
        self._check(self.L.almpc_timing_set_stride(self.h, int(every)))

    def timing_reset(self, reserve_steps=0):
        self._check(self.L.almpc_timing_reset(self.h, int(reserve_steps)))

    def timing_samples(self, cap=4096):
        """Per recorded step its stage times (ms): dict of float32 arrays of length min(cap, steps recorded since the reset)."""
        n = ctypes.c_int()
        a = {k: np.zeros(int(cap), dtype=np.float32) for k in ("admm_ms", "polish_ms", "rollout_ms", "total_ms")}
        self._check(self.L.almpc_timing_samples(self.h, int(cap), ctypes.byref(n), *[a[k].ctypes.data_as(_fp) for k in a]))
        k = min(int(cap), n.value)
        return {key: v[:k] for key, v in a.items()}

    def timing_summary(self):
        n = ctypes.c_int()
        v = [ctypes.c_double() for _ in range(4)]
        self._check(self.L.almpc_timing_summary(self.h, ctypes.byref(n), *[ctypes.byref(x) for x in v]))
        out = dict(zip(("admm_ms", "polish_ms", "rollout_ms", "total_ms"), [x.value for x in v]))
        out["steps"] = n.value
        return out


class _HandleView(Solver):
    """A Solver over a handle owned by a Group (no create / destroy of its own)."""

    def __init__(self, L, h, n, m, N, batch):
        self._bind(L, n, m, N, batch)
        self.h = self._t = h

    def close(self):
        self.h = self._t = None

    __del__ = close


class Group(_Target):
    """One process, several GPUs (almpc_group_*): one handle per entry of `devices` on its contiguous shard of the batch; every call
    fans out over the handles, nothing on the step path synchronises across devices.  Host arrays cover the whole batch."""

    _PREFIX = "almpc_group_"
    _NO_U0 = False

    def __init__(self, n, m, N, batch, devices, timing=False, structured=False, structured_fallback=None):
        self._bind(load(), n, m, N, batch)
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        g = _hp()
        rc = self.L.almpc_group_create(ctypes.byref(g), self.n, self.m, self.N, self.batch, len(devices), devs,
                                       (FLAG_TIMING if timing else 0) | (FLAG_STRUCTURED if structured else 0))
        if rc != ALMPC_OK:
            raise AlmpcError(rc, "almpc_group_create failed (are the devices visible? there is no CPU fallback)")
        self.g = self._t = g
        self.shards = []
        for i in range(len(devices)):
            f, c = ctypes.c_int(), ctypes.c_int()
            self._check(self.L.almpc_group_shard(self.g, i, ctypes.byref(f), ctypes.byref(c)))
            self.shards.append((f.value, c.value))
        self.handles = [_HandleView(self.L, _hp(self.L.almpc_group_handle(self.g, i)), self.n, self.m, self.N, c)
                        for i, (_, c) in enumerate(self.shards)]
        if structured_fallback is not None:
            self._check(self.L.almpc_group_set_structured_fallback(self.g, 1 if structured_fallback else 0))

    def close(self):
        if getattr(self, "g", None):
            for hv in self.handles:
                hv.close()
            self.L.almpc_group_destroy(self.g)
            self.g = self._t = None

    __del__ = close

    # ---- what only the handles have: by shard
    def _shard_of(self, i):
        """(the handle that holds instance i, its index there)"""
        for h, (f, c) in zip(self.handles, self.shards):
            if f <= i < f + c:
                return h, i - f
        raise IndexError(i)

    def model_instance(self, i):
        h, k = self._shard_of(i)
        return h.model_instance(k)

    def terminal_weight_instance(self, i):
        h, k = self._shard_of(i)
        return h.terminal_weight_instance(k)

    def relin_terminal_status(self):
        return np.concatenate([h.relin_terminal_status() for h in self.handles])

    # ---- the step path of a group
    def update_initialization(self, x0, resident=False):
        """x0 (batch, n) to the handles' shards.  Default: almpc_group_update_initialization (pinned slots read in place by the next
        step, no device copy -- the per-step path).  resident=True: a device copy per handle (almpc_update_initialization), for states
        that many steps will read (the pinned slot costs every step its transfer over the link)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(self.batch, self.n)
        if resident:
            for hv, (f, c) in zip(self.handles, self.shards):
                hv.update_initialization(x0[f:f + c])
            return
        self._check(self._f.update_initialization(self._t, _ptr(x0)))

    def x0_staging(self):
        """The handles' pinned x0 slots as numpy views ((count_i, n) each): write the shards' states there, then update_initialization_staged()."""
        slots = (_dp * len(self.handles))()
        self._check(self.L.almpc_group_x0_staging(self.g, slots))
        self._slots = slots
        return [np.ctypeslib.as_array(slots[i], shape=(c, self.n)) for i, (_, c) in enumerate(self.shards)]

    def update_initialization_staged(self):
        self._check(self.L.almpc_group_update_initialization_staged(self.g, self._slots))

    def get_results(self, want=("x", "e_x", "u", "e_u", "status", "iters", "polish_iters")):
        """_Target.get_results with "u0" (batch, m) among the names; a name that is none of WANT is refused."""
        _want_mask(want)
        return _Target.get_results(self, want)
