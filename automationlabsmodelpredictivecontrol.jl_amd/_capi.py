"""ctypes binding of libalmpc.so (include/almpc.h).  The HIP library is the only compute path: if it is
missing or fails to load this module raises -- there is no CPU fallback."""
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


def load():
    """Load libalmpc.so and declare the prototypes of include/almpc.h.  Raises OSError if the
    library has not been built (`make lib` or `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} not found: build the HIP library first (make lib). There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    L.almpc_default_opts.argtypes = [ctypes.POINTER(almpc_opts)]
    L.almpc_default_opts.restype = None
    L.almpc_create.argtypes = [ctypes.POINTER(_hp), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                               ctypes.c_int, ctypes.c_uint32]
    L.almpc_destroy.argtypes = [_hp]
    L.almpc_destroy.restype = None
    L.almpc_last_error.argtypes = [_hp]
    L.almpc_last_error.restype = ctypes.c_char_p
    L.almpc_design_shared.argtypes = [_hp] + [_dp] * 10 + [ctypes.c_double, ctypes.c_double]
    L.almpc_design_batched.argtypes = [_hp] + [_dp] * 6 + [ctypes.c_int, _dp, _dp, ctypes.c_double, ctypes.c_double]
    L.almpc_design_batched.restype = ctypes.c_int
    L.almpc_design_batched_weighted.argtypes = [_hp] + [_dp] * 6 + [ctypes.c_int, _dp, _dp, ctypes.c_double, ctypes.c_double]
    L.almpc_design_batched_weighted.restype = ctypes.c_int
    L.almpc_get_weights_instance.argtypes = [_hp, ctypes.c_int, _dp, _dp, _dp]
    L.almpc_get_weights_instance.restype = ctypes.c_int
    L.almpc_get_design_instance.argtypes = [_hp, ctypes.c_int, _dp, _dp, _dp]
    L.almpc_design_ltv.argtypes = [_hp] + [_dp] * 11 + [ctypes.c_int, _dp, _dp, ctypes.c_double, ctypes.c_double]
    L.almpc_design_ltv.restype = ctypes.c_int
    L.almpc_get_gradient_instance.argtypes = [_hp, ctypes.c_int, _dp]
    L.almpc_get_gradient_instance.restype = ctypes.c_int
    L.almpc_sqp_fnn_setup.argtypes = [_hp, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [_dp] * 10 + [ctypes.c_int, _dp, _dp,
                                                                                                     ctypes.c_double, ctypes.c_double]
    L.almpc_sqp_fnn_setup.restype = ctypes.c_int
    L.almpc_sqp_densenet_setup.argtypes = L.almpc_sqp_fnn_setup.argtypes
    L.almpc_sqp_densenet_setup.restype = ctypes.c_int
    L.almpc_sqp_fnn_start.argtypes = [_hp, _dp, _dp]
    L.almpc_sqp_fnn_start.restype = ctypes.c_int
    L.almpc_sqp_fnn_iterate.argtypes = [_hp, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, _dp, _dp]
    L.almpc_sqp_fnn_iterate.restype = ctypes.c_int
    L.almpc_sqp_fnn_skipped.argtypes = [_hp, _ip]
    L.almpc_sqp_fnn_set_step_rule.argtypes = [_hp, ctypes.c_int]
    L.almpc_sqp_fnn_set_step_rule.restype = ctypes.c_int
    L.almpc_sqp_fnn_skipped.restype = ctypes.c_int
    L.almpc_sqp_fnn_solve.argtypes = [_hp, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, _ip, _ip, _dp]
    L.almpc_sqp_fnn_solve.restype = ctypes.c_int
    L.almpc_sqp_fnn_set_hessian.argtypes = [_hp, ctypes.c_int]
    L.almpc_sqp_fnn_set_hessian.restype = ctypes.c_int
    L.almpc_sqp_fnn_set_row_multipliers.argtypes = [_hp, ctypes.c_int]
    L.almpc_sqp_fnn_set_row_multipliers.restype = ctypes.c_int
    L.almpc_sqp_fnn_state_multipliers.argtypes = [_hp, _dp]
    L.almpc_sqp_fnn_state_multipliers.restype = ctypes.c_int
    L.almpc_get_design_instance.restype = ctypes.c_int
    L.almpc_set_reference.argtypes = [_hp, _dp, _dp, ctypes.c_int]
    L.almpc_set_terminal_equality.argtypes = [_hp, ctypes.c_int]
    L.almpc_set_state_box.argtypes = [_hp, _dp, _dp]
    L.almpc_set_state_box.restype = ctypes.c_int
    L.almpc_sqp_fnn_set_structured.argtypes = [_hp, ctypes.c_int]
    L.almpc_sqp_fnn_set_structured.restype = ctypes.c_int
    L.almpc_set_rho_profile.argtypes = [_hp, ctypes.c_int]
    L.almpc_set_rho_profile.restype = ctypes.c_int
    L.almpc_set_step_fusion.argtypes = [_hp, ctypes.c_int]
    L.almpc_set_step_fusion.restype = ctypes.c_int
    L.almpc_set_terminal_equality.restype = ctypes.c_int
    L.almpc_update_initialization.argtypes = [_hp, _dp]
    L.almpc_update_initialization_device.argtypes = [_hp, ctypes.c_void_p]
    L.almpc_calculate.argtypes = [_hp, ctypes.POINTER(almpc_opts)]
    L.almpc_calculate_async.argtypes = [_hp, ctypes.POINTER(almpc_opts)]
    L.almpc_synchronize.argtypes = [_hp]
    L.almpc_get_results.argtypes = [_hp, _dp, _dp, _dp, _dp, _ip, _ip, _ip]
    L.almpc_get_design.argtypes = [_hp, _dp, _dp, _dp, _dp]
    L.almpc_device_results.argtypes = [_hp] + [ctypes.POINTER(ctypes.c_void_p)] * 4
    L.almpc_get_timing.argtypes = [_hp, _fp, _fp, _fp, _fp]
    L.almpc_timing_reset.argtypes = [_hp, ctypes.c_int]
    L.almpc_timing_set_stride.argtypes = [_hp, ctypes.c_int]
    L.almpc_timing_set_stride.restype = ctypes.c_int
    L.almpc_debug_poison_lds.argtypes = [_hp]
    L.almpc_advance_plant.argtypes = [_hp]
    L.almpc_advance_plant.restype = ctypes.c_int
    L.almpc_dare.argtypes = [ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, _dp, _dp]
    L.almpc_dare.restype = ctypes.c_int
    L.almpc_dare_batched.argtypes = [ctypes.c_int] * 4 + [_dp] * 5 + [_ip]
    L.almpc_dare_batched.restype = ctypes.c_int
    L.almpc_dare_vjp.argtypes = [ctypes.c_int, ctypes.c_int] + [_dp] * 10
    L.almpc_dare_vjp.restype = ctypes.c_int
    L.almpc_dare_vjp_batched.argtypes = [ctypes.c_int] * 4 + [_dp] * 10 + [_ip]
    L.almpc_dare_vjp_batched.restype = ctypes.c_int
    L.almpc_set_terminal_weight.argtypes = [_hp, ctypes.c_int]
    L.almpc_set_terminal_weight.restype = ctypes.c_int
    L.almpc_relin_fnn_terminal_status.argtypes = [_hp, _ip]
    L.almpc_relin_fnn_terminal_status.restype = ctypes.c_int
    L.almpc_get_terminal_weight_instance.argtypes = [_hp, ctypes.c_int, _dp]
    L.almpc_get_terminal_weight_instance.restype = ctypes.c_int
    L.almpc_group_set_terminal_weight.argtypes = [_hp, ctypes.c_int]
    L.almpc_group_set_terminal_weight.restype = ctypes.c_int
    L.almpc_c2d.argtypes = [ctypes.c_int, ctypes.c_int, _dp, _dp, ctypes.c_double, _dp, _dp]
    L.almpc_c2d.restype = ctypes.c_int
    L.almpc_c2d_batched.argtypes = [ctypes.c_int] * 4 + [_dp, _dp, ctypes.c_double, _dp, _dp, _ip]
    L.almpc_c2d_batched.restype = ctypes.c_int
    L.almpc_set_model_time.argtypes = [_hp, ctypes.c_int, ctypes.c_double]
    L.almpc_set_model_time.restype = ctypes.c_int
    L.almpc_get_model_instance.argtypes = [_hp, ctypes.c_int, _dp, _dp]
    L.almpc_get_model_instance.restype = ctypes.c_int
    L.almpc_group_set_model_time.argtypes = [_hp, ctypes.c_int, ctypes.c_double]
    L.almpc_group_set_model_time.restype = ctypes.c_int
    L.almpc_sensitivity.argtypes = [_hp, ctypes.c_uint32, ctypes.c_double]
    L.almpc_get_sensitivity.argtypes = [_hp, _dp, _dp, _dp, _ip]
    L.almpc_device_sensitivity.argtypes = [_hp] + [ctypes.POINTER(ctypes.c_void_p)] * 4
    L.almpc_sensitivity_vjp.argtypes = [_hp, _dp, _dp, ctypes.c_double, _dp, _ip]
    L.almpc_group_sensitivity.argtypes = [_hp, ctypes.c_uint32, ctypes.c_double]
    L.almpc_group_get_sensitivity.argtypes = [_hp, _dp, _dp, _dp, _ip]
    L.almpc_group_sensitivity_vjp.argtypes = [_hp, _dp, _dp, ctypes.c_double, _dp, _ip]
    L.almpc_sensitivity_rows.argtypes = [_hp, ctypes.c_uint32, ctypes.c_double, ctypes.c_double]
    L.almpc_sensitivity_rows_vjp.argtypes = [_hp, _dp, _dp, ctypes.c_double, ctypes.c_double, _dp, _ip]
    L.almpc_group_sensitivity_rows.argtypes = [_hp, ctypes.c_uint32, ctypes.c_double, ctypes.c_double]
    L.almpc_group_sensitivity_rows_vjp.argtypes = [_hp, _dp, _dp, ctypes.c_double, ctypes.c_double, _dp, _ip]
    L.almpc_sensitivity_params_vjp.argtypes = [_hp, _dp, _dp, ctypes.c_double, ctypes.POINTER(almpc_param_grads)]
    L.almpc_group_sensitivity_params_vjp.argtypes = [_hp, _dp, _dp, ctypes.c_double, ctypes.POINTER(almpc_param_grads)]
    L.almpc_sensitivity_params_vjp_dare.argtypes = [_hp, _dp, _dp, ctypes.c_double, ctypes.POINTER(almpc_param_grads), _ip]
    L.almpc_group_sensitivity_params_vjp_dare.argtypes = [_hp, _dp, _dp, ctypes.c_double, ctypes.POINTER(almpc_param_grads), _ip]
    L.almpc_sensitivity_stagewise.argtypes = [_hp, ctypes.c_uint32, ctypes.c_double]
    L.almpc_sensitivity_stagewise_vjp.argtypes = [_hp, _dp, _dp, ctypes.c_double, _dp, _ip]
    L.almpc_group_sensitivity_stagewise.argtypes = [_hp, ctypes.c_uint32, ctypes.c_double]
    L.almpc_group_sensitivity_stagewise_vjp.argtypes = [_hp, _dp, _dp, ctypes.c_double, _dp, _ip]
    L.almpc_sensitivity_stagewise_rate.argtypes = [_hp, ctypes.c_uint32, ctypes.c_double]
    L.almpc_sensitivity_stagewise_rate_vjp.argtypes = [_hp, _dp, _dp, ctypes.c_double, _dp, _ip]
    L.almpc_group_sensitivity_stagewise_rate.argtypes = [_hp, ctypes.c_uint32, ctypes.c_double]
    L.almpc_group_sensitivity_stagewise_rate_vjp.argtypes = [_hp, _dp, _dp, ctypes.c_double, _dp, _ip]
    for nm_ in ("almpc_sensitivity", "almpc_get_sensitivity", "almpc_device_sensitivity", "almpc_sensitivity_vjp",
                "almpc_sensitivity_stagewise", "almpc_sensitivity_stagewise_vjp",
                "almpc_sensitivity_stagewise_rate", "almpc_sensitivity_stagewise_rate_vjp",
                "almpc_group_sensitivity_stagewise_rate", "almpc_group_sensitivity_stagewise_rate_vjp",
                "almpc_group_sensitivity_stagewise", "almpc_group_sensitivity_stagewise_vjp",
                "almpc_sensitivity_params_vjp", "almpc_group_sensitivity_params_vjp",
                "almpc_sensitivity_params_vjp_dare", "almpc_group_sensitivity_params_vjp_dare",
                "almpc_group_sensitivity", "almpc_group_get_sensitivity", "almpc_group_sensitivity_vjp",
                "almpc_sensitivity_rows", "almpc_sensitivity_rows_vjp", "almpc_group_sensitivity_rows", "almpc_group_sensitivity_rows_vjp"):
        getattr(L, nm_).restype = ctypes.c_int
    L.almpc_certificate.argtypes = [_hp, ctypes.c_uint32]
    L.almpc_get_certificate.argtypes = [_hp, _dp, _dp, _dp, _dp]
    L.almpc_device_certificate.argtypes = [_hp] + [ctypes.POINTER(ctypes.c_void_p)] * 4
    L.almpc_group_certificate.argtypes = [_hp, ctypes.c_uint32]
    L.almpc_group_get_certificate.argtypes = [_hp, _dp, _dp, _dp, _dp]
    for nm_ in ("almpc_certificate", "almpc_get_certificate", "almpc_device_certificate", "almpc_group_certificate",
                "almpc_group_get_certificate"):
        getattr(L, nm_).restype = ctypes.c_int
    L.almpc_set_keep_stage_models.argtypes = [_hp, ctypes.c_int]
    L.almpc_certificate_ltv.argtypes = [_hp, ctypes.c_uint32]
    L.almpc_get_certificate_ltv.argtypes = [_hp] + [_dp] * 6
    L.almpc_device_certificate_ltv.argtypes = [_hp] + [ctypes.POINTER(ctypes.c_void_p)] * 6
    L.almpc_relin_fnn_certificate.argtypes = [_hp, ctypes.c_uint32]
    L.almpc_group_relin_fnn_certificate.argtypes = [_hp, ctypes.c_uint32]
    for nm_ in ("almpc_set_keep_stage_models", "almpc_certificate_ltv", "almpc_get_certificate_ltv", "almpc_device_certificate_ltv",
                "almpc_relin_fnn_certificate", "almpc_group_relin_fnn_certificate"):
        getattr(L, nm_).restype = ctypes.c_int
    L.almpc_set_structured_fallback.argtypes = [_hp, ctypes.c_int]
    L.almpc_relin_fnn_setup.argtypes = [_hp, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [_dp] * 12 + [ctypes.c_double, ctypes.c_double]
    L.almpc_relin_fnn_setup.restype = ctypes.c_int
    L.almpc_relin_densenet_setup.argtypes = L.almpc_relin_fnn_setup.argtypes
    L.almpc_relin_densenet_setup.restype = ctypes.c_int
    L.almpc_relin_fnn_step.argtypes = [_hp, ctypes.POINTER(almpc_opts)]
    L.almpc_relin_fnn_step_async.argtypes = [_hp, ctypes.POINTER(almpc_opts)]
    L.almpc_relin_fnn_timing.argtypes = [_hp, _fp, _fp, _fp]
    L.almpc_relin_fnn_advance.argtypes = [_hp]
    L.almpc_comm_unique_id.argtypes = [ctypes.c_char_p]
    L.almpc_comm_init.argtypes = [_hp, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    L.almpc_comm_summary.argtypes = [_hp, ctypes.POINTER(ctypes.c_int64)]
    L.almpc_comm_allgather_first_input.argtypes = [_hp, _dp, ctypes.POINTER(_dp)]
    L.almpc_fnn_linearize.argtypes = [ctypes.c_int] * 6 + [_dp] * 4 + [ctypes.c_int] + [_dp] * 5
    L.almpc_fnn_linearize.restype = ctypes.c_int
    L.almpc_densenet_linearize.argtypes = L.almpc_fnn_linearize.argtypes
    L.almpc_densenet_linearize.restype = ctypes.c_int
    L.almpc_debug_poison_lds.restype = ctypes.c_int
    L.almpc_timing_summary.argtypes = [_hp, ctypes.POINTER(ctypes.c_int)] + [_dp] * 4
    # host-facing step path (pinned staging, copy streams) and one-process multi-GPU groups
    L.almpc_update_initialization_async.argtypes = [_hp, _dp]
    L.almpc_x0_staging.argtypes = [_hp, ctypes.POINTER(_dp)]
    L.almpc_get_results_async.argtypes = [_hp, ctypes.c_uint32]
    L.almpc_get_results_wait.argtypes = [_hp, ctypes.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip]
    L.almpc_host_results.argtypes = [_hp, ctypes.c_int] + [ctypes.POINTER(ctypes.c_void_p)] * 8
    L.almpc_get_first_input.argtypes = [_hp, _dp]
    L.almpc_group_create.argtypes = [ctypes.POINTER(_hp), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.POINTER(ctypes.c_int), ctypes.c_uint32]
    L.almpc_group_destroy.argtypes = [_hp]
    L.almpc_group_destroy.restype = None
    L.almpc_group_last_error.argtypes = [_hp]
    L.almpc_group_last_error.restype = ctypes.c_char_p
    L.almpc_group_size.argtypes = [_hp]
    L.almpc_group_handle.argtypes = [_hp, ctypes.c_int]
    L.almpc_group_handle.restype = _hp
    L.almpc_group_shard.argtypes = [_hp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.almpc_group_design_shared.argtypes = [_hp] + [_dp] * 10 + [ctypes.c_double, ctypes.c_double]
    L.almpc_group_set_reference.argtypes = [_hp, _dp, _dp, ctypes.c_int]
    L.almpc_group_update_initialization.argtypes = [_hp, _dp]
    L.almpc_group_calculate.argtypes = [_hp, ctypes.POINTER(almpc_opts)]
    L.almpc_group_calculate_async.argtypes = [_hp, ctypes.POINTER(almpc_opts)]
    L.almpc_group_synchronize.argtypes = [_hp]
    L.almpc_group_get_results.argtypes = [_hp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip]
    # group forms of everything a handle can do
    for nm_ in ("almpc_group_set_terminal_equality", "almpc_group_set_rho_profile", "almpc_group_set_structured_fallback",
                "almpc_group_sqp_fnn_set_structured", "almpc_group_sqp_fnn_set_step_rule", "almpc_group_sqp_fnn_set_hessian",
                "almpc_group_sqp_fnn_set_row_multipliers"):
        getattr(L, nm_).argtypes = [_hp, ctypes.c_int]
    L.almpc_group_set_state_box.argtypes = [_hp, _dp, _dp]
    L.almpc_group_design_batched.argtypes = [_hp] + [_dp] * 6 + [ctypes.c_int, _dp, _dp, ctypes.c_double, ctypes.c_double]
    L.almpc_group_design_batched_weighted.argtypes = L.almpc_group_design_batched.argtypes
    L.almpc_group_design_batched_weighted.restype = ctypes.c_int
    L.almpc_group_relin_fnn_setup.argtypes = [_hp, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [_dp] * 12 + [ctypes.c_double, ctypes.c_double]
    L.almpc_group_relin_fnn_step.argtypes = [_hp, ctypes.POINTER(almpc_opts)]
    L.almpc_group_relin_fnn_step_async.argtypes = [_hp, ctypes.POINTER(almpc_opts)]
    L.almpc_group_relin_fnn_advance.argtypes = [_hp]
    L.almpc_group_advance_plant.argtypes = [_hp]
    L.almpc_group_sqp_fnn_setup.argtypes = [_hp, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [_dp] * 10 + [ctypes.c_int, _dp, _dp, ctypes.c_double, ctypes.c_double]
    L.almpc_group_relin_densenet_setup.argtypes = L.almpc_group_relin_fnn_setup.argtypes
    L.almpc_group_sqp_densenet_setup.argtypes = L.almpc_group_sqp_fnn_setup.argtypes
    L.almpc_group_sqp_fnn_start.argtypes = [_hp, _dp, _dp]
    L.almpc_group_sqp_fnn_iterate.argtypes = [_hp, ctypes.c_int, ctypes.c_double, ctypes.POINTER(almpc_opts), _dp, _dp]
    L.almpc_group_sqp_fnn_skipped.argtypes = [_hp, _ip]
    L.almpc_group_sqp_fnn_state_multipliers.argtypes = [_hp, _dp]
    L.almpc_group_sqp_fnn_solve.argtypes = [_hp, ctypes.c_int, ctypes.c_double, ctypes.POINTER(almpc_opts), _ip, _ip, _dp]
    L.almpc_group_x0_staging.argtypes = [_hp, ctypes.POINTER(_dp)]
    L.almpc_group_update_initialization_staged.argtypes = [_hp, ctypes.POINTER(_dp)]
    L.almpc_group_get_results_async.argtypes = [_hp, ctypes.c_uint32]
    L.almpc_group_get_results_wait.argtypes = [_hp, ctypes.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip]
    for nm_ in ("almpc_group_set_terminal_equality", "almpc_group_set_rho_profile", "almpc_group_set_structured_fallback", "almpc_group_set_state_box",
                "almpc_group_design_batched", "almpc_group_relin_fnn_setup", "almpc_group_relin_fnn_step", "almpc_group_relin_fnn_step_async",
                "almpc_group_relin_fnn_advance", "almpc_group_advance_plant", "almpc_group_sqp_fnn_set_structured", "almpc_group_sqp_fnn_set_step_rule",
                "almpc_group_sqp_fnn_setup", "almpc_group_relin_densenet_setup", "almpc_group_sqp_densenet_setup", "almpc_group_sqp_fnn_start", "almpc_group_sqp_fnn_iterate", "almpc_group_sqp_fnn_skipped", "almpc_group_sqp_fnn_solve", "almpc_group_sqp_fnn_set_hessian",
                "almpc_group_sqp_fnn_set_row_multipliers", "almpc_group_sqp_fnn_state_multipliers",
                "almpc_group_x0_staging", "almpc_group_update_initialization_staged", "almpc_group_get_results_async", "almpc_group_get_results_wait"):
        getattr(L, nm_).restype = ctypes.c_int
    L.almpc_set_start_from.argtypes = [_hp, _hp]
    L.almpc_set_start_from.restype = ctypes.c_int
    L.almpc_timing_samples.argtypes = [_hp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _fp, _fp, _fp, _fp]
    L.almpc_timing_samples.restype = ctypes.c_int
    for name in ("almpc_x0_staging", "almpc_update_initialization_async", "almpc_get_results_async", "almpc_get_results_wait", "almpc_host_results",
                 "almpc_get_first_input", "almpc_group_create", "almpc_group_size", "almpc_group_shard", "almpc_group_design_shared",
                 "almpc_group_set_reference", "almpc_group_update_initialization", "almpc_group_calculate",
                 "almpc_group_calculate_async", "almpc_group_synchronize", "almpc_group_get_results"):
        getattr(L, name).restype = ctypes.c_int
    for name in ("almpc_create", "almpc_design_shared", "almpc_set_reference", "almpc_update_initialization",
                 "almpc_update_initialization_device", "almpc_calculate", "almpc_calculate_async", "almpc_synchronize",
                 "almpc_get_results", "almpc_get_design", "almpc_device_results", "almpc_get_timing", "almpc_timing_reset",
                 "almpc_timing_summary"):
        getattr(L, name).restype = ctypes.c_int
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


def _weighted_design_args(n, m, b, A_batch, B_batch, Q_batch, R_batch, S_batch, P, umin, umax):
    """((A, B, Q, R, S, P, umin, umax) as the C call takes them: every block column-major, S / P None where not given; P_per_instance)."""
    def blocks(M, r, c):
        return np.ascontiguousarray(np.asarray(M, dtype=np.float64).reshape(b, r, c).transpose(0, 2, 1))
    A, B = blocks(A_batch, n, n), blocks(B_batch, n, m)
    Q, R = blocks(Q_batch, n, n), blocks(R_batch, m, m)
    S = None if S_batch is None else blocks(S_batch, m, m)
    p_inst = 0
    if P is not None:
        P = np.asarray(P, dtype=np.float64)
        if P.ndim == 3:
            P = blocks(P, n, n); p_inst = 1
        else:
            P = _colmajor(P, (n, n))
    umin = np.ascontiguousarray(umin, dtype=np.float64).reshape(m)
    umax = np.ascontiguousarray(umax, dtype=np.float64).reshape(m)
    return (A, B, Q, R, S, P, umin, umax), p_inst


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
    g_u = np.ascontiguousarray(np.asarray(g_u, dtype=np.float64).reshape(b, m, N).transpose(0, 2, 1))
    if g_x is not None:
        g_x = np.ascontiguousarray(np.asarray(g_x, dtype=np.float64).reshape(b, n, N + 1).transpose(0, 2, 1))
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
    g_u = np.ascontiguousarray(np.asarray(g_u, dtype=np.float64).reshape(b, m, N).transpose(0, 2, 1))
    if g_x is not None:
        g_x = np.ascontiguousarray(np.asarray(g_x, dtype=np.float64).reshape(b, n, N + 1).transpose(0, 2, 1))
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
    cm = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))  # column-major blocks
    Q, R = _colmajor(Q, (n, n)), _colmajor(R, (m, m))
    shapes = {"A": (b, n, n), "B": (b, n, m), "Q": (b, n, n), "R": (b, m, m)}
    out = {}
    for k in want:
        out[k] = np.full(shapes[k], np.nan).transpose(0, 2, 1).copy() if init is None or k not in init else \
            cm(np.asarray(init[k], dtype=np.float64).reshape(shapes[k]))
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
    Ac = np.ascontiguousarray(A.transpose(0, 2, 1))  # column-major blocks
    Bc = np.ascontiguousarray(B.transpose(0, 2, 1))
    Q, R = _colmajor(Q, (n, n)), _colmajor(R, (m, m))
    if P_init is None:
        P = np.full((b, n, n), np.nan)
    else:
        P = np.ascontiguousarray(np.asarray(P_init, dtype=np.float64).reshape(b, n, n).transpose(0, 2, 1))
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
    Ac = np.ascontiguousarray(A.transpose(0, 2, 1))  # column-major blocks
    Bc = np.ascontiguousarray(B.transpose(0, 2, 1))
    if out_init is None:
        Ad, Bd = np.full((b, n, n), np.nan), np.full((b, m, n), np.nan)
    else:
        Ad = np.ascontiguousarray(np.asarray(out_init[0], dtype=np.float64).reshape(b, n, n).transpose(0, 2, 1))
        Bd = np.ascontiguousarray(np.asarray(out_init[1], dtype=np.float64).reshape(b, n, m).transpose(0, 2, 1))
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


def fnn_linearize(W_in, W_h, b_h, W_out, x, u, act="relu", device=0, want_f=False, net="fnn"):
    """Batched Jacobians of a network model on the GPU: x (batch, n), u (batch, m) -> A (batch, n, n), B (batch, n, m).
    net: "fnn", "resnet" or "polynet" (NET_KINDS), all in the Fnn weight layout."""
    L = load()
    W_in, W_out = np.asfortranarray(W_in, dtype=np.float64), np.asfortranarray(W_out, dtype=np.float64)
    H, nin = W_in.shape
    n = W_out.shape[0]
    m = nin - n
    nl = len(W_h)
    Wh = np.ascontiguousarray(np.stack([np.asfortranarray(W, dtype=np.float64).T for W in W_h])) if nl else np.zeros((1, 1, 1))
    bh = np.ascontiguousarray(np.stack([np.asarray(b, dtype=np.float64) for b in b_h])) if nl else np.zeros((1, 1))
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
    batch = x.shape[0]
    A = np.empty((batch, n, n)); B = np.empty((batch, m, n)); f = np.empty((batch, n)) if want_f else None
    rc = L.almpc_fnn_linearize(int(device), n, m, H, nl, net_code(net, act), _ptr(W_in), _ptr(Wh), _ptr(bh), _ptr(W_out),
                               batch, _ptr(x), _ptr(u), _ptr(A), _ptr(B), _ptr(f))
    if rc != ALMPC_OK:
        raise AlmpcError(rc, "almpc_fnn_linearize")
    A, B = A.transpose(0, 2, 1), B.transpose(0, 2, 1)  # column-major buffers -> (batch, row, col)
    return (A, B, f) if want_f else (A, B)


def densenet_linearize(W_in, W_h, b_h, W_out, x, u, act="relu", device=0, want_f=False):
    """fnn_linearize for a DenseNet (almpc_densenet_linearize): W_h a list of (H, (l+1) H) blocks, W_out (n, (L+1) H)."""
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
    H, nl, W_in, Wh, bh, W_out = _pack_densenet(W_in, W_h, b_h, W_out, x.shape[1], u.shape[1])
    n, m = x.shape[1], u.shape[1]
    batch = x.shape[0]
    if u.shape[0] != batch:
        raise ValueError("x and u must hold the same number of points")
    code = _densenet_act(act)
    L = load()
    A = np.empty((batch, n, n)); B = np.empty((batch, m, n)); f = np.empty((batch, n)) if want_f else None
    rc = L.almpc_densenet_linearize(int(device), n, m, H, nl, code, _ptr(W_in), _ptr(Wh), _ptr(bh), _ptr(W_out),
                                    batch, _ptr(x), _ptr(u), _ptr(A), _ptr(B), _ptr(f))
    if rc != ALMPC_OK:
        raise AlmpcError(rc, "almpc_densenet_linearize")
    A, B = A.transpose(0, 2, 1), B.transpose(0, 2, 1)
    return (A, B, f) if want_f else (A, B)


class Solver:
    """Thin object wrapper of an almpc_handle: one device, one batch shard."""

    def __init__(self, n, m, N, batch, device=0, timing=False, structured=False, structured_fallback=None):
        """structured: ALMPC_FLAG_STRUCTURED (the stage-wise solve of the multiple-shooting form is the handle's solver: no m*N <= 128
        limit).  structured_fallback: the redo of the instances a condensed step leaves without a certificate by the stage-wise
        solvers -- None: the library default (on wherever they cover the design), True: required, False: off."""
        self.L = load()
        self.n, self.m, self.N, self.batch = int(n), int(m), int(N), int(batch)
        self.nz = self.m * self.N
        h = _hp()
        rc = self.L.almpc_create(ctypes.byref(h), self.n, self.m, self.N, self.batch, int(device),
                                 (FLAG_TIMING if timing else 0) | (FLAG_STRUCTURED if structured else 0))
        if rc != ALMPC_OK:
            raise AlmpcError(rc, "almpc_create failed (is a gfx950 GPU visible? there is no CPU fallback)")
        self.h = h
        if structured_fallback is not None:
            self._check(self.L.almpc_set_structured_fallback(self.h, 1 if structured_fallback else 0))

    def _check(self, rc):
        if rc != ALMPC_OK:
            raise AlmpcError(rc, (self.L.almpc_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.almpc_destroy(self.h)
            self.h = None

    __del__ = close

    def design_shared(self, A, B, Q, R, S=None, P=None, umin=None, umax=None, xmin=None, xmax=None, rho=0.1, sigma=1e-6,
                      terminal="none", rho_profile="scalar"):
        """xmin/xmax: state box (the reference's kw mpc_state_constraint); terminal: "none" | "equality";
        rho_profile: "scalar" (OSQP: rho for every row) | "stiffness" (rho_i = rho / (H'^-1)_ii)."""
        n, m = self.n, self.m
        if terminal not in ("none", "equality"):
            raise ValueError("terminal must be 'none' or 'equality'")
        self._check(self.L.almpc_set_terminal_equality(self.h, 1 if terminal == "equality" else 0))
        self._check(self.L.almpc_set_rho_profile(self.h, {"scalar": 0, "stiffness": 1}[rho_profile]))
        A, B, Q, R = _colmajor(A, (n, n)), _colmajor(B, (n, m)), _colmajor(Q, (n, n)), _colmajor(R, (m, m))
        S = None if S is None else _colmajor(S, (m, m))
        P = None if P is None else _colmajor(P, (n, n))
        umin = np.ascontiguousarray(umin, dtype=np.float64).reshape(m)
        umax = np.ascontiguousarray(umax, dtype=np.float64).reshape(m)
        xmin = None if xmin is None else np.ascontiguousarray(xmin, dtype=np.float64).reshape(n)
        xmax = None if xmax is None else np.ascontiguousarray(xmax, dtype=np.float64).reshape(n)
        self._check(self.L.almpc_design_shared(self.h, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(S), _ptr(P), _ptr(umin),
                                               _ptr(umax), _ptr(xmin), _ptr(xmax), float(rho), float(sigma)))

    def _state_rows(self, xmin, xmax, terminal):
        """State box / terminal equality of the designs without xmin / xmax arguments (almpc_set_state_box, almpc_set_terminal_equality)."""
        if (xmin is None) != (xmax is None):
            raise ValueError("give both xmin and xmax or neither")
        self._check(self.L.almpc_set_terminal_equality(self.h, 1 if terminal == "equality" else 0))
        if xmin is None:
            self._check(self.L.almpc_set_state_box(self.h, None, None))
        else:
            lo = np.ascontiguousarray(xmin, dtype=np.float64).reshape(self.n)
            hi = np.ascontiguousarray(xmax, dtype=np.float64).reshape(self.n)
            self._check(self.L.almpc_set_state_box(self.h, _ptr(lo), _ptr(hi)))

    def design_batched(self, A_batch, B_batch, Q, R, S=None, P=None, umin=None, umax=None, rho=0.1, sigma=1e-6,
                       rho_profile="scalar", xmin=None, xmax=None, terminal="none"):
        """One model per instance: A_batch (batch, n, n), B_batch (batch, n, m).  P: None (DARE per instance), (n, n) shared
        or (batch, n, n).  xmin / xmax: state box (stages 1..N+1); terminal = "equality": e_x[:, N+1] = 0."""
        n, m, b = self.n, self.m, self.batch
        self._state_rows(xmin, xmax, terminal)
        self._check(self.L.almpc_set_rho_profile(self.h, {"scalar": 0, "stiffness": 1}[rho_profile]))
        A = np.ascontiguousarray(np.asarray(A_batch, dtype=np.float64).reshape(b, n, n).transpose(0, 2, 1))  # column-major blocks
        B = np.ascontiguousarray(np.asarray(B_batch, dtype=np.float64).reshape(b, n, m).transpose(0, 2, 1))
        Q, R = _colmajor(Q, (n, n)), _colmajor(R, (m, m))
        S = None if S is None else _colmajor(S, (m, m))
        p_inst = 0
        if P is not None:
            P = np.asarray(P, dtype=np.float64)
            if P.ndim == 3:
                P = np.ascontiguousarray(P.reshape(b, n, n).transpose(0, 2, 1)); p_inst = 1
            else:
                P = _colmajor(P, (n, n))
        umin = np.ascontiguousarray(umin, dtype=np.float64).reshape(m)
        umax = np.ascontiguousarray(umax, dtype=np.float64).reshape(m)
        self._check(self.L.almpc_design_batched(self.h, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(S), _ptr(P), p_inst, _ptr(umin),
                                                _ptr(umax), float(rho), float(sigma)))

    def design_batched_weighted(self, A_batch, B_batch, Q_batch, R_batch, S_batch=None, P=None, umin=None, umax=None, rho=0.1, sigma=1e-6,
                                rho_profile="scalar", xmin=None, xmax=None, terminal="none"):
        """design_batched with one weight set per instance (almpc_design_batched_weighted): Q_batch (batch, n, n), R_batch and
        S_batch (batch, m, m), S_batch None for S = 0 everywhere.  The other arguments are design_batched's."""
        self._state_rows(xmin, xmax, terminal)
        self._check(self.L.almpc_set_rho_profile(self.h, {"scalar": 0, "stiffness": 1}[rho_profile]))
        args, p_inst = _weighted_design_args(self.n, self.m, self.batch, A_batch, B_batch, Q_batch, R_batch, S_batch, P, umin, umax)
        self._check(self.L.almpc_design_batched_weighted(self.h, *[_ptr(a) for a in args[:6]], p_inst, _ptr(args[6]), _ptr(args[7]),
                                                         float(rho), float(sigma)))

    def get_weights_instance(self, i):
        """dict(Q (n, n), R (m, m), S (m, m)): the weights instance i is designed on, as the design kernels read them
        (almpc_get_weights_instance)."""
        Q, R, S = np.empty((self.n, self.n), order="F"), np.empty((self.m, self.m), order="F"), np.empty((self.m, self.m), order="F")
        self._check(self.L.almpc_get_weights_instance(self.h, int(i), _ptr(Q), _ptr(R), _ptr(S)))
        return dict(Q=Q, R=R, S=S)

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
        self._check(self.L.almpc_set_rho_profile(self.h, {"scalar": 0, "stiffness": 1}[rho_profile]))
        A = np.ascontiguousarray(np.asarray(A_all, dtype=np.float64).reshape(b, N, n, n).transpose(0, 1, 3, 2))
        B = np.ascontiguousarray(np.asarray(B_all, dtype=np.float64).reshape(b, N, n, m).transpose(0, 1, 3, 2))
        c = None if c_all is None else np.ascontiguousarray(np.asarray(c_all, dtype=np.float64).reshape(b, N, n))
        xb = np.ascontiguousarray(np.asarray(xbar, dtype=np.float64).reshape(b, n, N + 1).transpose(0, 2, 1))
        ub = np.ascontiguousarray(np.asarray(ubar, dtype=np.float64).reshape(b, m, N).transpose(0, 2, 1))
        xr = None if x_ref is None else np.ascontiguousarray(np.asarray(x_ref, dtype=np.float64).reshape(n, N + 1).T)
        ur = None if u_ref is None else np.ascontiguousarray(np.asarray(u_ref, dtype=np.float64).reshape(m, N).T)
        Q, R = _colmajor(Q, (n, n)), _colmajor(R, (m, m))
        S = None if S is None else _colmajor(S, (m, m))
        P = np.asarray(P, dtype=np.float64)
        p_inst = 0
        if P.ndim == 3:
            P = np.ascontiguousarray(P.reshape(b, n, n).transpose(0, 2, 1)); p_inst = 1
        else:
            P = _colmajor(P, (n, n))
        umin = np.ascontiguousarray(umin, dtype=np.float64).reshape(m)
        umax = np.ascontiguousarray(umax, dtype=np.float64).reshape(m)
        self._check(self.L.almpc_design_ltv(self.h, _ptr(A), _ptr(B), _ptr(c), _ptr(xb), _ptr(ub), _ptr(xr), _ptr(ur), _ptr(Q), _ptr(R),
                                            _ptr(S), _ptr(P), p_inst, _ptr(umin), _ptr(umax), float(rho), float(sigma)))

    def sqp_fnn_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu", rho=0.1,
                      sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none", qp_solver="condensed", net="fnn"):
        """SQP outer loop for a network model (almpc_sqp_fnn_*): network (and net) as in fnn_linearize, x_ref (n, N+1) / u_ref (m, N) or None,
        P (n, n) or (batch, n, n).  qp_solver: "condensed" (default) or "structured" (every QP through k_riccati, no condensed design).  xmin / xmax: the state box of the reference's NLP branch
        (.../fnn/mpc_modeler_implementation_fnn.jl:146-153) as rows of every iteration's QP; terminal = "equality"."""
        W_in, W_out = np.asfortranarray(W_in, dtype=np.float64), np.asfortranarray(W_out, dtype=np.float64)
        H = W_in.shape[0]
        nl = len(W_h)
        Wh = np.ascontiguousarray(np.stack([np.asfortranarray(W, dtype=np.float64).T for W in W_h])) if nl else np.zeros((1, 1, 1))
        bh = np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.float64) for v in b_h])) if nl else np.zeros((1, 1))
        self._sqp_setup(self.L.almpc_sqp_fnn_setup, H, nl, net_code(net, act), W_in, Wh, bh, W_out, x_ref, u_ref, Q, R, S, P, umin, umax,
                        rho, sigma, rho_profile, xmin, xmax, terminal, qp_solver)

    def sqp_densenet_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu",
                           rho=0.1, sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none", qp_solver="condensed"):
        """sqp_fnn_setup for a DenseNet (almpc_sqp_densenet_setup; network as in densenet_linearize); then the sqp_fnn_* calls."""
        H, nl, W_in, Wh, bh, W_out = _pack_densenet(W_in, W_h, b_h, W_out, self.n, self.m)
        self._sqp_setup(self.L.almpc_sqp_densenet_setup, H, nl, _densenet_act(act), W_in, Wh, bh, W_out, x_ref, u_ref, Q, R, S, P, umin,
                        umax, rho, sigma, rho_profile, xmin, xmax, terminal, qp_solver)

    def _sqp_setup(self, setup, H, nl, code, W_in, Wh, bh, W_out, x_ref, u_ref, Q, R, S, P, umin, umax, rho, sigma, rho_profile, xmin,
                   xmax, terminal, qp_solver):
        n, m, N, b = self.n, self.m, self.N, self.batch
        self._state_rows(xmin, xmax, terminal)
        self._check(self.L.almpc_sqp_fnn_set_structured(self.h, 1 if qp_solver == "structured" else 0))
        self._check(self.L.almpc_set_rho_profile(self.h, {"scalar": 0, "stiffness": 1}[rho_profile]))
        xr = None if x_ref is None else np.ascontiguousarray(np.asarray(x_ref, dtype=np.float64).reshape(n, N + 1).T)
        ur = None if u_ref is None else np.ascontiguousarray(np.asarray(u_ref, dtype=np.float64).reshape(m, N).T)
        Q, R = _colmajor(Q, (n, n)), _colmajor(R, (m, m))
        S = None if S is None else _colmajor(S, (m, m))
        P = np.asarray(P, dtype=np.float64)
        p_inst = 0
        if P.ndim == 3:
            P = np.ascontiguousarray(P.reshape(b, n, n).transpose(0, 2, 1)); p_inst = 1
        else:
            P = _colmajor(P, (n, n))
        umin = np.ascontiguousarray(umin, dtype=np.float64).reshape(m)
        umax = np.ascontiguousarray(umax, dtype=np.float64).reshape(m)
        self._check(setup(self.h, H, nl, code, _ptr(W_in), _ptr(Wh), _ptr(bh), _ptr(W_out), _ptr(xr), _ptr(ur), _ptr(Q), _ptr(R), _ptr(S),
                          _ptr(P), p_inst, _ptr(umin), _ptr(umax), float(rho), float(sigma)))

    def relin_fnn_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu", rho=0.1,
                        sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none", net="fnn"):
        """Device-resident per-step re-linearisation of a network model (almpc_relin_fnn_*, BASELINE configs[3]): network (and net)
        as in fnn_linearize, shared x_ref (n, N+1) / u_ref (m, N) or None, shared P (n, n); xmin / xmax / terminal as in design_batched."""
        W_in, W_out = np.asfortranarray(W_in, dtype=np.float64), np.asfortranarray(W_out, dtype=np.float64)
        H = W_in.shape[0]
        nl = len(W_h)
        Wh = np.ascontiguousarray(np.stack([np.asfortranarray(W, dtype=np.float64).T for W in W_h])) if nl else np.zeros((1, 1, 1))
        bh = np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.float64) for v in b_h])) if nl else np.zeros((1, 1))
        self._relin_setup(self.L.almpc_relin_fnn_setup, H, nl, net_code(net, act), W_in, Wh, bh, W_out, x_ref, u_ref, Q, R, S, P, umin,
                          umax, rho, sigma, rho_profile, xmin, xmax, terminal)

    def relin_densenet_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu",
                             rho=0.1, sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none"):
        """relin_fnn_setup for a DenseNet (almpc_relin_densenet_setup; network as in densenet_linearize); then the relin_fnn_* calls."""
        H, nl, W_in, Wh, bh, W_out = _pack_densenet(W_in, W_h, b_h, W_out, self.n, self.m)
        self._relin_setup(self.L.almpc_relin_densenet_setup, H, nl, _densenet_act(act), W_in, Wh, bh, W_out, x_ref, u_ref, Q, R, S, P,
                          umin, umax, rho, sigma, rho_profile, xmin, xmax, terminal)

    def _relin_setup(self, setup, H, nl, code, W_in, Wh, bh, W_out, x_ref, u_ref, Q, R, S, P, umin, umax, rho, sigma, rho_profile, xmin,
                     xmax, terminal):
        n, m, N = self.n, self.m, self.N
        self._state_rows(xmin, xmax, terminal)
        self._check(self.L.almpc_set_rho_profile(self.h, {"scalar": 0, "stiffness": 1}[rho_profile]))
        xr = None if x_ref is None else np.ascontiguousarray(np.asarray(x_ref, dtype=np.float64).reshape(n, N + 1).T)
        ur = None if u_ref is None else np.ascontiguousarray(np.asarray(u_ref, dtype=np.float64).reshape(m, N).T)
        Q, R = _colmajor(Q, (n, n)), _colmajor(R, (m, m))
        S = None if S is None else _colmajor(S, (m, m))
        P = _colmajor(P, (n, n))
        umin = np.ascontiguousarray(umin, dtype=np.float64).reshape(m)
        umax = np.ascontiguousarray(umax, dtype=np.float64).reshape(m)
        self._check(setup(self.h, H, nl, code, _ptr(W_in), _ptr(Wh), _ptr(bh), _ptr(W_out), _ptr(xr), _ptr(ur), _ptr(Q), _ptr(R), _ptr(S),
                          _ptr(P), _ptr(umin), _ptr(umax), float(rho), float(sigma)))

    def relin_fnn_step(self, opts: almpc_opts | None = None, sync=True):
        fn = self.L.almpc_relin_fnn_step if sync else self.L.almpc_relin_fnn_step_async
        self._check(fn(self.h, ctypes.byref(opts) if opts is not None else None))

    def relin_fnn_advance(self):
        """x0 <- fnn(x0, u[:,1]) on the device (closed loop of the black-box model)."""
        self._check(self.L.almpc_relin_fnn_advance(self.h))

    def relin_fnn_certificate(self, want=("cost", "res", "grad", "costate")) -> dict:
        """almpc_relin_fnn_certificate + almpc_get_certificate: `certificate` of the last relin_fnn_step, with that step's own models,
        terminal weights and weights."""
        self._check(self.L.almpc_relin_fnn_certificate(self.h, _cert_mask(want)))
        return _cert_read(self.L.almpc_get_certificate, self.h, self._check, want, self.batch, self.n, self.m, self.N)

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

    def sqp_fnn_start(self, x0, u_guess=None):
        """x0 (batch, n); u_guess (batch, m, N) or None."""
        x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(self.batch, self.n))
        ug = None if u_guess is None else np.ascontiguousarray(np.asarray(u_guess, dtype=np.float64).reshape(self.batch, self.m, self.N).transpose(0, 2, 1))
        self._check(self.L.almpc_sqp_fnn_start(self.h, _ptr(x0), _ptr(ug)))

    def sqp_fnn_iterate(self, iters, step_scale=1.0, opts=None, step_rule="fixed"):
        """-> (step_inf[iters], defect_inf[iters]); raises AlmpcError(ALMPC_ERR_NUMERIC) when an instance had to skip an iteration
        (the histories are still filled: see .sqp_last).  step_rule: "fixed" | "merit" (l1 merit-function safeguard)."""
        self._check(self.L.almpc_sqp_fnn_set_step_rule(self.h, {"fixed": 0, "merit": 1}[step_rule]))
        st, de = np.zeros(int(iters)), np.zeros(int(iters))
        self.sqp_last = (st, de)
        self._check(self.L.almpc_sqp_fnn_iterate(self.h, int(iters), float(step_scale), ctypes.byref(opts) if opts is not None else None,
                                                 _ptr(st), _ptr(de)))
        return st, de

    def sqp_fnn_solve(self, max_iters, tol, opts=None, step_rule="merit"):
        """Solve to a tolerance (almpc_sqp_fnn_solve): at most max_iters iterations, each instance frozen once its iterate passes the
        first-order test (zero defects, projected adjoint-gradient residual <= tol).  -> dict(status (batch,) int32: 0 converged,
        1 iteration limit, 2 skipped, 3 infeasible QP; iters (batch,) int32; kkt (batch,) residual of the last test).
        The step rule is a setting of the handle and stays in force: a later sqp_fnn_iterate sets its own (default "fixed")."""
        self._check(self.L.almpc_sqp_fnn_set_step_rule(self.h, {"fixed": 0, "merit": 1}[step_rule]))
        st, it, kk = np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch)
        self._check(self.L.almpc_sqp_fnn_solve(self.h, int(max_iters), float(tol), ctypes.byref(opts) if opts is not None else None,
                                               st.ctypes.data_as(_ip), it.ctypes.data_as(_ip), _ptr(kk)))
        return dict(status=st, iters=it, kkt=kk)

    def sqp_fnn_set_hessian(self, mode):
        """Hessian of the loop's QPs: "gauss_newton" (default) or "exact" (almpc_sqp_fnn_set_hessian); stays in force."""
        self._check(self.L.almpc_sqp_fnn_set_hessian(self.h, SQP_HESSIANS[mode]))

    def sqp_fnn_set_row_multipliers(self, on):
        """State rows (state box, terminal equality) in the loop's stopping test and exact Hessian: the finishes hand the row multipliers
        of every iteration's QP out (almpc_sqp_fnn_set_row_multipliers; default off, stays in force)."""
        self._check(self.L.almpc_sqp_fnn_set_row_multipliers(self.h, 1 if on else 0))

    def sqp_fnn_state_multipliers(self):
        """-> (batch, n, N): multiplier of the row of x_{k+1}[i] at [:, i, k] in each instance's last solved QP (> 0 upper bound, < 0 lower
        bound, free on a terminal-equality row, 0 outside the working set); zeros with the switch off or without state rows."""
        mu = np.zeros((self.batch, self.N, self.n))
        self._check(self.L.almpc_sqp_fnn_state_multipliers(self.h, _ptr(mu)))
        return np.ascontiguousarray(mu.transpose(0, 2, 1))

    def sqp_fnn_skipped(self):
        out = np.zeros(self.batch, dtype=np.int32)
        self._check(self.L.almpc_sqp_fnn_skipped(self.h, out.ctypes.data_as(_ip)))
        return out

    def get_gradient_instance(self, i):
        q = np.empty(self.nz)
        self._check(self.L.almpc_get_gradient_instance(self.h, int(i), _ptr(q)))
        return q

    def get_design_instance(self, i):
        n, nz = self.n, self.nz
        H = np.empty((nz, nz), order="F"); F = np.empty((nz, n), order="F"); d = np.empty(nz)
        self._check(self.L.almpc_get_design_instance(self.h, int(i), _ptr(H), _ptr(F), _ptr(d)))
        return dict(H=H, F=F, d=d)

    def set_terminal_weight(self, mode):
        """Before a design: "given" / 0 (default) or "dare_device" / 1 -- design_batched(P=None) and every relin_fnn step take each
        instance's terminal weight from the DARE of its own model, solved on the device (almpc_set_terminal_weight)."""
        self._check(self.L.almpc_set_terminal_weight(self.h, _terminal_mode(mode)))

    def relin_terminal_status(self):
        """(batch,) int32 of the last relin_fnn step with the mode on: 0 = the instance's own DARE solution, 1 = the setup's P."""
        out = np.zeros(self.batch, dtype=np.int32)
        self._check(self.L.almpc_relin_fnn_terminal_status(self.h, out.ctypes.data_as(_ip)))
        return out

    def terminal_weight_instance(self, i):
        """(n, n) terminal weight instance i was designed with (almpc_get_terminal_weight_instance)."""
        P = np.empty((self.n, self.n), order="F")
        self._check(self.L.almpc_get_terminal_weight_instance(self.h, int(i), _ptr(P)))
        return P

    def set_model_time(self, mode, Ts=0.0):
        """Before a design: "discrete" / 0 (default) or "continuous" / 1 with the sample time Ts -- the models given to design_shared and
        design_batched, and the network of the relin_fnn pipeline, are continuous-time and are discretised by zero-order hold at Ts
        (almpc_set_model_time)."""
        self._check(self.L.almpc_set_model_time(self.h, _model_time_mode(mode), float(Ts)))

    def model_instance(self, i):
        """(A (n, n), B (n, m)): the DISCRETE model instance i is designed on (almpc_get_model_instance)."""
        A, B = np.empty((self.n, self.n), order="F"), np.empty((self.n, self.m), order="F")
        self._check(self.L.almpc_get_model_instance(self.h, int(i), _ptr(A), _ptr(B)))
        return A, B

    def start_from(self, other: "Solver"):
        """Structured handle: the next calculate starts from `other`'s last inputs (same batch, horizon <= this one's): horizon
        continuation / chaining of solvers (almpc_set_start_from)."""
        self._check(self.L.almpc_set_start_from(self.h, other.h))

    def set_step_fusion(self, on: bool):
        """One kernel per step (default) or the two-kernel path whose stage times can be told apart."""
        self._check(self.L.almpc_set_step_fusion(self.h, 1 if on else 0))

    def set_reference(self, x_ref, u_ref, per_instance=False):
        """x_ref (n, N+1) / u_ref (m, N), or with per_instance (batch, n, N+1) / (batch, m, N)."""
        n, m, N = self.n, self.m, self.N
        x_ref, u_ref = np.asarray(x_ref, dtype=np.float64), np.asarray(u_ref, dtype=np.float64)
        if per_instance:
            xr = np.ascontiguousarray(x_ref.reshape(self.batch, n, N + 1).transpose(0, 2, 1))
            ur = np.ascontiguousarray(u_ref.reshape(self.batch, m, N).transpose(0, 2, 1))
        else:
            xr = np.ascontiguousarray(x_ref.reshape(n, N + 1).T)
            ur = np.ascontiguousarray(u_ref.reshape(m, N).T)
        self._check(self.L.almpc_set_reference(self.h, _ptr(xr), _ptr(ur), 1 if per_instance else 0))

    def update_initialization(self, x0):
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(self.batch, self.n)
        self._check(self.L.almpc_update_initialization(self.h, _ptr(x0)))

    def update_initialization_device(self, dev_ptr: int):
        self._check(self.L.almpc_update_initialization_device(self.h, ctypes.c_void_p(dev_ptr)))

    def calculate(self, opts: almpc_opts | None = None, sync=True):
        fn = self.L.almpc_calculate if sync else self.L.almpc_calculate_async
        self._check(fn(self.h, None if opts is None else ctypes.byref(opts)))

    def synchronize(self):
        self._check(self.L.almpc_synchronize(self.h))

    def get_results(self, want=("x", "e_x", "u", "e_u", "status", "iters", "polish_iters")):
        b, n, m, N = self.batch, self.n, self.m, self.N
        bufs = {}
        if "x" in want: bufs["x"] = np.empty((b, N + 1, n))
        if "e_x" in want: bufs["e_x"] = np.empty((b, N + 1, n))
        if "u" in want: bufs["u"] = np.empty((b, N, m))
        if "e_u" in want: bufs["e_u"] = np.empty((b, N, m))
        for k in ("status", "iters", "polish_iters"):
            if k in want: bufs[k] = np.empty(b, dtype=np.int32)
        ip = lambda k: bufs[k].ctypes.data_as(_ip) if k in bufs else None
        self._check(self.L.almpc_get_results(self.h, _ptr(bufs.get("x")), _ptr(bufs.get("e_x")), _ptr(bufs.get("u")),
                                             _ptr(bufs.get("e_u")), ip("status"), ip("iters"), ip("polish_iters")))
        # Julia-shaped views: (batch, n, N+1) and (batch, m, N)
        for k in ("x", "e_x", "u", "e_u"):
            if k in bufs: bufs[k] = bufs[k].transpose(0, 2, 1)
        return bufs

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

    def get_results_async(self, want=("u0", "status")) -> int:
        """Ask for results of the last enqueued step (names of WANT; "u0" = u[:, 1] of every instance); returns a ticket."""
        t = self.L.almpc_get_results_async(self.h, _want_mask(want))
        if t < 0:
            self._check(t)
        return t

    def get_results_wait(self, ticket, want=("u0", "status"), copy=True):
        """Results of a ticket.  copy=True: fresh arrays (almpc_get_results_wait); copy=False: views of the handle's pinned slot
        (almpc_host_results: zero-copy, valid until two more requests).  Shapes as get_results; u0 (batch, m)."""
        b, n, m, N = self.batch, self.n, self.m, self.N
        shapes = {"x": (b, N + 1, n), "e_x": (b, N + 1, n), "u": (b, N, m), "e_u": (b, N, m), "u0": (b, m),
                  "status": (b,), "iters": (b,), "polish_iters": (b,)}
        order = ("x", "e_x", "u", "e_u", "u0", "status", "iters", "polish_iters")
        want = set(want)
        _want_mask(want)
        if copy:
            bufs = {k: np.empty(shapes[k], dtype=np.int32 if k in ("status", "iters", "polish_iters") else np.float64) for k in want}
            args = [(bufs[k].ctypes.data_as(_ip if bufs[k].dtype == np.int32 else _dp) if k in bufs else None) for k in order]
            self._check(self.L.almpc_get_results_wait(self.h, int(ticket), *args))
        else:
            self._check(self.L.almpc_get_results_wait(self.h, int(ticket), *([None] * 8)))
            ps = [ctypes.c_void_p() for _ in order]
            self._check(self.L.almpc_host_results(self.h, int(ticket), *[ctypes.byref(q) for q in ps]))
            bufs = {}
            for k, q in zip(order, ps):
                if k in want:
                    if not q.value:
                        raise AlmpcError(-1, f"result {k!r} was not part of the request of ticket {ticket}")
                    ct = ctypes.c_int32 if k in ("status", "iters", "polish_iters") else ctypes.c_double
                    cnt = int(np.prod(shapes[k]))
                    bufs[k] = np.ctypeslib.as_array(ctypes.cast(q.value, ctypes.POINTER(ct)), shape=(cnt,)).reshape(shapes[k])
        for k in ("x", "e_x", "u", "e_u"):
            if k in bufs: bufs[k] = bufs[k].transpose(0, 2, 1)
        return bufs

    # ---- sensitivities of the last step to x0 (include/almpc.h "Sensitivities"; an extension beyond the reference's surface)
    def sensitivity(self, want=("K0", "dU", "dX"), act_tol=0.0) -> dict:
        """almpc_sensitivity + almpc_get_sensitivity: K0 (batch, m, n) = du[:,1]/dx0, dU (batch, m, N, n), dX (batch, n, N+1, n),
        each [b, i, k, c] = d(entry i of stage k) / d x0[c], and rows (batch,) = rows at a bound (-1: instance not solved, zeros).
        act_tol <= 0: 1e-9 (in units of the row's Jacobi scale)."""
        self._check(self.L.almpc_sensitivity(self.h, _sens_mask(want), float(act_tol)))
        return _sens_read(self.L.almpc_get_sensitivity, self.h, self._check, want, self.batch, self.n, self.m, self.N)

    def device_sensitivity(self):
        ps = [ctypes.c_void_p() for _ in range(4)]
        self._check(self.L.almpc_device_sensitivity(self.h, *[ctypes.byref(p) for p in ps]))
        return dict(zip(("K0", "dU", "dX", "rows"), [p.value for p in ps]))

    # ---- certificate of the last step (include/almpc.h "Certificate of the last step")
    def certificate(self, want=("cost", "res", "grad", "costate")) -> dict:
        """almpc_certificate + almpc_get_certificate: cost (batch,) the objective value, res (batch,) the KKT residual of the returned
        inputs, grad (batch, m, N) the gradient of the objective in the inputs, costate (batch, n, N+1) (costate[:, :, 0] = dJ/dx0).
        From the returned trajectories alone: every instance is certified whatever its status."""
        self._check(self.L.almpc_certificate(self.h, _cert_mask(want)))
        return _cert_read(self.L.almpc_get_certificate, self.h, self._check, want, self.batch, self.n, self.m, self.N)

    def device_certificate(self):
        ps = [ctypes.c_void_p() for _ in range(4)]
        self._check(self.L.almpc_device_certificate(self.h, *[ctypes.byref(p) for p in ps]))
        return dict(zip(("cost", "res", "grad", "costate"), [p.value for p in ps]))

    # ---- ... of a step of a time-varying design (include/almpc.h "Certificate of a step of a time-varying design")
    def certificate_ltv(self, want=("cost", "res", "grad", "costate", "x", "e_x")) -> dict:
        """almpc_certificate_ltv + almpc_get_certificate_ltv after design_ltv(keep_stage_models=True) and a step: cost (batch,), res (batch,),
        grad (batch, m, N), costate (batch, n, N+1) (costate[:, :, k+1] = dJ/dc_k), x (batch, n, N+1) the predicted states xbar + dx and
        e_x = x - x_ref, for what `want` names ("x" and "e_x" come together)."""
        mask = _cert_mask(want, CERT_LTV)
        self._check(self.L.almpc_certificate_ltv(self.h, mask))
        b, n, m, N = self.batch, self.n, self.m, self.N
        names = (want,) if isinstance(want, str) else tuple(want)
        shapes = dict(cost=(b,), res=(b,), grad=(b, N, m), costate=(b, N + 1, n), x=(b, N + 1, n), e_x=(b, N + 1, n))
        bufs = {k: (np.empty(shapes[k]) if k in names else None) for k in shapes}
        self._check(self.L.almpc_get_certificate_ltv(self.h, *[_ptr(bufs[k]) for k in ("cost", "res", "grad", "costate", "x", "e_x")]))
        return {k: (v if v.ndim == 1 else v.transpose(0, 2, 1)) for k, v in bufs.items() if v is not None}

    def device_certificate_ltv(self):
        ps = [ctypes.c_void_p() for _ in range(6)]
        self._check(self.L.almpc_device_certificate_ltv(self.h, *[ctypes.byref(p) for p in ps]))
        return dict(zip(("cost", "res", "grad", "costate", "x", "e_x"), [p.value for p in ps]))

    def sensitivity_vjp(self, g_u, g_x=None, act_tol=0.0):
        """dL/dx0 (batch, n) for a loss with gradients g_u (batch, m, N) and g_x (batch, n, N+1) or None on the returned
        trajectories (almpc_sensitivity_vjp: no Jacobian is formed); also returns rows (batch,)."""
        return _sens_vjp(self.L.almpc_sensitivity_vjp, self.h, self._check, g_u, g_x, act_tol, self.batch, self.n, self.m, self.N)

    def sensitivity_stagewise(self, want=("K0", "dU", "dX"), act_tol=0.0) -> dict:
        """sensitivity on a structured handle (almpc_sensitivity_stagewise + almpc_get_sensitivity): the Riccati recursion on the face
        where the inputs at a bound are held; input box only, S = 0.  act_tol is relative to the width of the input box (0: 1e-7)."""
        self._check(self.L.almpc_sensitivity_stagewise(self.h, _sens_mask(want), float(act_tol)))
        return _sens_read(self.L.almpc_get_sensitivity, self.h, self._check, want, self.batch, self.n, self.m, self.N)

    def sensitivity_stagewise_vjp(self, g_u, g_x=None, act_tol=0.0):
        """sensitivity_vjp on a structured handle (almpc_sensitivity_stagewise_vjp): (g_x0 (batch, n), rows (batch,))."""
        return _sens_vjp(self.L.almpc_sensitivity_stagewise_vjp, self.h, self._check, g_u, g_x, act_tol, self.batch, self.n, self.m, self.N)

    def sensitivity_stagewise_rate(self, want=("K0", "dU", "dX"), act_tol=0.0) -> dict:
        """sensitivity_stagewise for every structured input-box design, with or without an input-rate weight S
        (almpc_sensitivity_stagewise_rate + almpc_get_sensitivity): with S the recursion runs in the stage state [dx_k; du_(k-1)]
        (k_sens_face_rate), without it the call is sensitivity_stagewise to the byte."""
        self._check(self.L.almpc_sensitivity_stagewise_rate(self.h, _sens_mask(want), float(act_tol)))
        return _sens_read(self.L.almpc_get_sensitivity, self.h, self._check, want, self.batch, self.n, self.m, self.N)

    def sensitivity_stagewise_rate_vjp(self, g_u, g_x=None, act_tol=0.0):
        """sensitivity_stagewise_vjp for designs with or without S (almpc_sensitivity_stagewise_rate_vjp): (g_x0 (batch, n), rows (batch,))."""
        return _sens_vjp(self.L.almpc_sensitivity_stagewise_rate_vjp, self.h, self._check, g_u, g_x, act_tol, self.batch, self.n, self.m,
                         self.N)

    def sensitivity_params_vjp(self, g_u, g_x=None, want=PARAM_GROUPS, act_tol=0.0, terminal="data") -> dict:
        """Gradients of the loss of sensitivity_vjp in the problem data, per instance (almpc_sensitivity_params_vjp): x0, the QP's
        linear term f, u_ref, the input box, the weights Q, P, R, S and the model A, B -- what `want` names -- and rows.  For a shared
        design the caller sums over the batch.  terminal="data": P is data; "dare" (almpc_sensitivity_params_vjp_dare): P_i =
        DARE(A_i, B_i, Q, R) is followed into Q, R, A, B, and the dict also carries dare_status (batch,): 0 followed, else the
        instance keeps its P-as-data values (its P is not the stabilising DARE solution of the design's model)."""
        dare = _terminal_gradient(terminal)
        call = self.L.almpc_sensitivity_params_vjp_dare if dare else self.L.almpc_sensitivity_params_vjp
        return _sens_params_vjp(call, self.h, self._check, g_u, g_x, want, act_tol, self.batch, self.n, self.m, self.N, dare)

    def sensitivity_rows(self, want=("K0", "dU", "dX"), act_tol_u=0.0, act_tol_x=0.0) -> dict:
        """sensitivity for shared designs with a state box and / or the terminal equality as well (almpc_sensitivity_rows +
        almpc_get_sensitivity): rows counts input, state-box and terminal-equality rows at a bound; act_tol_x is the state rows'
        threshold (0: 1e-7, relative to max(1, |bound|)).  Without state rows it is sensitivity(want, act_tol_u), bit for bit."""
        self._check(self.L.almpc_sensitivity_rows(self.h, _sens_mask(want), float(act_tol_u), float(act_tol_x)))
        return _sens_read(self.L.almpc_get_sensitivity, self.h, self._check, want, self.batch, self.n, self.m, self.N)

    def sensitivity_rows_vjp(self, g_u, g_x=None, act_tol_u=0.0, act_tol_x=0.0):
        """sensitivity_vjp in the rows form (almpc_sensitivity_rows_vjp): (g_x0 (batch, n), rows (batch,))."""
        return _sens_vjp(self.L.almpc_sensitivity_rows_vjp, self.h, self._check, g_u, g_x, (act_tol_u, act_tol_x), self.batch, self.n,
                         self.m, self.N)

    def get_first_input(self):
        """u[:, 1] of every instance, (batch, m): what a receding-horizon caller applies (almpc_get_first_input)."""
        u0 = np.empty((self.batch, self.m))
        self._check(self.L.almpc_get_first_input(self.h, _ptr(u0)))
        return u0

    def get_design(self):
        n, nz = self.n, self.nz
        H = np.empty((nz, nz), order="F"); F = np.empty((nz, n), order="F"); P = np.empty((n, n), order="F"); d = np.empty(nz)
        self._check(self.L.almpc_get_design(self.h, _ptr(H), _ptr(F), _ptr(P), _ptr(d)))
        return dict(H=H, F=F, P=P, d=d)

    def device_results(self):
        ps = [ctypes.c_void_p() for _ in range(4)]
        self._check(self.L.almpc_device_results(self.h, *[ctypes.byref(p) for p in ps]))
        return dict(zip(("x", "e_x", "u", "e_u"), [p.value for p in ps]))

    def get_timing(self):
        v = [ctypes.c_float() for _ in range(4)]
        self._check(self.L.almpc_get_timing(self.h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("admm_ms", "polish_ms", "rollout_ms", "total_ms"), [x.value for x in v]))

    def advance_plant(self):
        self._check(self.L.almpc_advance_plant(self.h))

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
        self.L, self.h = L, h
        self.n, self.m, self.N, self.batch = n, m, N, batch
        self.nz = m * N

    def close(self):
        self.h = None

    __del__ = close


class Group:
    """One process, several GPUs (almpc_group_*): one handle per entry of `devices` on its contiguous shard of the batch; every call
    fans out over the handles, nothing on the step path synchronises across devices.  Host arrays cover the whole batch."""

    def __init__(self, n, m, N, batch, devices, timing=False, structured=False, structured_fallback=None):
        self.L = load()
        self.n, self.m, self.N, self.batch = int(n), int(m), int(N), int(batch)
        self.nz = self.m * self.N
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        g = _hp()
        rc = self.L.almpc_group_create(ctypes.byref(g), self.n, self.m, self.N, self.batch, len(devices), devs,
                                       (FLAG_TIMING if timing else 0) | (FLAG_STRUCTURED if structured else 0))
        if rc != ALMPC_OK:
            raise AlmpcError(rc, "almpc_group_create failed (are the devices visible? there is no CPU fallback)")
        self.g = g
        self.shards = []
        for i in range(len(devices)):
            f, c = ctypes.c_int(), ctypes.c_int()
            self._check(self.L.almpc_group_shard(self.g, i, ctypes.byref(f), ctypes.byref(c)))
            self.shards.append((f.value, c.value))
        self.handles = [_HandleView(self.L, _hp(self.L.almpc_group_handle(self.g, i)), self.n, self.m, self.N, c)
                        for i, (_, c) in enumerate(self.shards)]
        if structured_fallback is not None:
            self._check(self.L.almpc_group_set_structured_fallback(self.g, 1 if structured_fallback else 0))

    def _check(self, rc):
        if rc != ALMPC_OK:
            raise AlmpcError(rc, (self.L.almpc_group_last_error(self.g) or b"").decode())

    def set_terminal_weight(self, mode):
        """Solver.set_terminal_weight on every handle (almpc_group_set_terminal_weight)."""
        self._check(self.L.almpc_group_set_terminal_weight(self.g, _terminal_mode(mode)))

    def set_model_time(self, mode, Ts=0.0):
        """Solver.set_model_time on every handle (almpc_group_set_model_time)."""
        self._check(self.L.almpc_group_set_model_time(self.g, _model_time_mode(mode), float(Ts)))

    def model_instance(self, i):
        for h, (f, c) in zip(self.handles, self.shards):
            if f <= i < f + c:
                return h.model_instance(i - f)
        raise IndexError(i)

    def relin_terminal_status(self):
        return np.concatenate([h.relin_terminal_status() for h in self.handles])

    def terminal_weight_instance(self, i):
        for h, (f, c) in zip(self.handles, self.shards):
            if f <= i < f + c:
                return h.terminal_weight_instance(i - f)
        raise IndexError(i)

    def _state_rows(self, xmin, xmax, terminal):
        if (xmin is None) != (xmax is None):
            raise ValueError("give both xmin and xmax or neither")
        self._check(self.L.almpc_group_set_terminal_equality(self.g, 1 if terminal == "equality" else 0))
        lo = None if xmin is None else np.ascontiguousarray(xmin, dtype=np.float64).reshape(self.n)
        hi = None if xmax is None else np.ascontiguousarray(xmax, dtype=np.float64).reshape(self.n)
        self._check(self.L.almpc_group_set_state_box(self.g, _ptr(lo), _ptr(hi)))

    def design_batched(self, A_batch, B_batch, Q, R, S=None, P=None, umin=None, umax=None, rho=0.1, sigma=1e-6, rho_profile="scalar",
                       xmin=None, xmax=None, terminal="none"):
        """almpc_group_design_batched: arguments of Solver.design_batched for the whole batch."""
        n, m, b = self.n, self.m, self.batch
        self._state_rows(xmin, xmax, terminal)
        self._check(self.L.almpc_group_set_rho_profile(self.g, {"scalar": 0, "stiffness": 1}[rho_profile]))
        A = np.ascontiguousarray(np.asarray(A_batch, dtype=np.float64).reshape(b, n, n).transpose(0, 2, 1))
        B = np.ascontiguousarray(np.asarray(B_batch, dtype=np.float64).reshape(b, n, m).transpose(0, 2, 1))
        Q, R = _colmajor(Q, (n, n)), _colmajor(R, (m, m))
        S = None if S is None else _colmajor(S, (m, m))
        p_inst = 0
        if P is not None:
            P = np.asarray(P, dtype=np.float64)
            if P.ndim == 3:
                P = np.ascontiguousarray(P.reshape(b, n, n).transpose(0, 2, 1)); p_inst = 1
            else:
                P = _colmajor(P, (n, n))
        umin = np.ascontiguousarray(umin, dtype=np.float64).reshape(m)
        umax = np.ascontiguousarray(umax, dtype=np.float64).reshape(m)
        self._check(self.L.almpc_group_design_batched(self.g, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(S), _ptr(P), p_inst, _ptr(umin),
                                                      _ptr(umax), float(rho), float(sigma)))

    def design_batched_weighted(self, A_batch, B_batch, Q_batch, R_batch, S_batch=None, P=None, umin=None, umax=None, rho=0.1, sigma=1e-6,
                                rho_profile="scalar", xmin=None, xmax=None, terminal="none"):
        """almpc_group_design_batched_weighted: arguments of Solver.design_batched_weighted for the whole batch."""
        self._state_rows(xmin, xmax, terminal)
        self._check(self.L.almpc_group_set_rho_profile(self.g, {"scalar": 0, "stiffness": 1}[rho_profile]))
        args, p_inst = _weighted_design_args(self.n, self.m, self.batch, A_batch, B_batch, Q_batch, R_batch, S_batch, P, umin, umax)
        self._check(self.L.almpc_group_design_batched_weighted(self.g, *[_ptr(a) for a in args[:6]], p_inst, _ptr(args[6]), _ptr(args[7]),
                                                               float(rho), float(sigma)))

    def _fnn_args(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S, P, umin, umax, act, p_batched, net="fnn"):
        n, m, N = self.n, self.m, self.N
        W_in = np.asarray(W_in, dtype=np.float64)
        H = W_in.shape[0]
        if net == "densenet":   # (the DenseNet layout and a bare activation: the *_densenet_setup calls)
            H, nl, W_in, Wh, bh, W_out = _pack_densenet(W_in, W_h, b_h, W_out, n, m)
        else:
            W_h = [np.asarray(w, dtype=np.float64) for w in W_h]
            nl = len(W_h)
            Wh = np.ascontiguousarray(np.stack([w.T for w in W_h])) if nl else None
            bh = np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.float64) for v in b_h])) if nl else None
        xr = np.ascontiguousarray(np.asarray(x_ref, dtype=np.float64).reshape(n, N + 1).T)
        ur = np.ascontiguousarray(np.asarray(u_ref, dtype=np.float64).reshape(m, N).T)
        P = np.asarray(P, dtype=np.float64)
        p_inst = 0
        if p_batched and P.ndim == 3:
            P = np.ascontiguousarray(P.reshape(self.batch, n, n).transpose(0, 2, 1)); p_inst = 1
        else:
            P = _colmajor(P, (n, n))
        arrs = [_colmajor(W_in, (H, n + m)), Wh, bh, _colmajor(W_out, (n, H * (nl + 1 if net == "densenet" else 1))), xr, ur, _colmajor(Q, (n, n)), _colmajor(R, (m, m)),
                None if S is None else _colmajor(S, (m, m)), P,
                np.ascontiguousarray(umin, dtype=np.float64).reshape(m), np.ascontiguousarray(umax, dtype=np.float64).reshape(m)]
        return H, nl, _densenet_act(act) if net == "densenet" else net_code(net, act), arrs, p_inst

    def relin_fnn_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu", rho=0.1,
                        sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none", net="fnn"):
        self._state_rows(xmin, xmax, terminal)
        self._check(self.L.almpc_group_set_rho_profile(self.g, {"scalar": 0, "stiffness": 1}[rho_profile]))
        H, nl, a, arrs, _ = self._fnn_args(W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S, P, umin, umax, act, False, net)
        self._keep = arrs
        self._check(self.L.almpc_group_relin_fnn_setup(self.g, H, nl, a, *[_ptr(v) for v in arrs], float(rho), float(sigma)))

    def relin_densenet_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu",
                             rho=0.1, sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none"):
        """almpc_group_relin_densenet_setup: Solver.relin_densenet_setup on every device."""
        self._state_rows(xmin, xmax, terminal)
        self._check(self.L.almpc_group_set_rho_profile(self.g, {"scalar": 0, "stiffness": 1}[rho_profile]))
        H, nl, a, arrs, _ = self._fnn_args(W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S, P, umin, umax, act, False, "densenet")
        self._keep = arrs
        self._check(self.L.almpc_group_relin_densenet_setup(self.g, H, nl, a, *[_ptr(v) for v in arrs], float(rho), float(sigma)))

    def relin_fnn_step(self, opts: almpc_opts | None = None, sync=True):
        fn = self.L.almpc_group_relin_fnn_step if sync else self.L.almpc_group_relin_fnn_step_async
        self._check(fn(self.g, None if opts is None else ctypes.byref(opts)))

    def relin_fnn_advance(self):
        self._check(self.L.almpc_group_relin_fnn_advance(self.g))

    def advance_plant(self):
        self._check(self.L.almpc_group_advance_plant(self.g))

    def sqp_fnn_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu", rho=0.1,
                      sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none", qp_solver="condensed", net="fnn"):
        self._state_rows(xmin, xmax, terminal)
        self._check(self.L.almpc_group_set_rho_profile(self.g, {"scalar": 0, "stiffness": 1}[rho_profile]))
        self._check(self.L.almpc_group_sqp_fnn_set_structured(self.g, 1 if qp_solver == "structured" else 0))
        H, nl, a, arrs, p_inst = self._fnn_args(W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S, P, umin, umax, act, True, net)
        self._keep = arrs
        ptrs = [_ptr(v) for v in arrs]
        self._check(self.L.almpc_group_sqp_fnn_setup(self.g, H, nl, a, *ptrs[:10], p_inst, ptrs[10], ptrs[11], float(rho), float(sigma)))

    def sqp_densenet_setup(self, W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S=None, P=None, umin=None, umax=None, act="relu",
                           rho=0.1, sigma=1e-6, rho_profile="scalar", xmin=None, xmax=None, terminal="none", qp_solver="condensed"):
        """almpc_group_sqp_densenet_setup: Solver.sqp_densenet_setup on every device."""
        self._state_rows(xmin, xmax, terminal)
        self._check(self.L.almpc_group_set_rho_profile(self.g, {"scalar": 0, "stiffness": 1}[rho_profile]))
        self._check(self.L.almpc_group_sqp_fnn_set_structured(self.g, 1 if qp_solver == "structured" else 0))
        H, nl, a, arrs, p_inst = self._fnn_args(W_in, W_h, b_h, W_out, x_ref, u_ref, Q, R, S, P, umin, umax, act, True, "densenet")
        self._keep = arrs
        ptrs = [_ptr(v) for v in arrs]
        self._check(self.L.almpc_group_sqp_densenet_setup(self.g, H, nl, a, *ptrs[:10], p_inst, ptrs[10], ptrs[11], float(rho),
                                                          float(sigma)))

    def sqp_fnn_start(self, x0, u_guess=None):
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(self.batch, self.n)
        ug = None if u_guess is None else np.ascontiguousarray(np.asarray(u_guess, dtype=np.float64).reshape(self.batch, self.m, self.N).transpose(0, 2, 1))
        self._check(self.L.almpc_group_sqp_fnn_start(self.g, _ptr(x0), _ptr(ug)))

    def sqp_fnn_iterate(self, iters, step_scale=1.0, opts=None, step_rule="fixed"):
        self._check(self.L.almpc_group_sqp_fnn_set_step_rule(self.g, {"fixed": 0, "merit": 1}[step_rule]))
        st, de = np.zeros(int(iters)), np.zeros(int(iters))
        self._check(self.L.almpc_group_sqp_fnn_iterate(self.g, int(iters), float(step_scale), None if opts is None else ctypes.byref(opts),
                                                       _ptr(st), _ptr(de)))
        return st, de

    def sqp_fnn_solve(self, max_iters, tol, opts=None, step_rule="merit"):
        self._check(self.L.almpc_group_sqp_fnn_set_step_rule(self.g, {"fixed": 0, "merit": 1}[step_rule]))
        st, it, kk = np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch)
        self._check(self.L.almpc_group_sqp_fnn_solve(self.g, int(max_iters), float(tol), None if opts is None else ctypes.byref(opts),
                                                     st.ctypes.data_as(_ip), it.ctypes.data_as(_ip), _ptr(kk)))
        return dict(status=st, iters=it, kkt=kk)

    def sqp_fnn_set_hessian(self, mode):
        self._check(self.L.almpc_group_sqp_fnn_set_hessian(self.g, SQP_HESSIANS[mode]))

    def sqp_fnn_set_row_multipliers(self, on):
        self._check(self.L.almpc_group_sqp_fnn_set_row_multipliers(self.g, 1 if on else 0))

    def sqp_fnn_state_multipliers(self):
        mu = np.zeros((self.batch, self.N, self.n))
        self._check(self.L.almpc_group_sqp_fnn_state_multipliers(self.g, _ptr(mu)))
        return np.ascontiguousarray(mu.transpose(0, 2, 1))

    def sqp_fnn_skipped(self):
        sk = np.zeros(self.batch, dtype=np.int32)
        self._check(self.L.almpc_group_sqp_fnn_skipped(self.g, sk.ctypes.data_as(_ip)))
        return sk

    def x0_staging(self):
        """The handles' pinned x0 slots as numpy views ((count_i, n) each): write the shards' states there, then update_initialization_staged()."""
        slots = (_dp * len(self.handles))()
        self._check(self.L.almpc_group_x0_staging(self.g, slots))
        self._slots = slots
        return [np.ctypeslib.as_array(slots[i], shape=(c, self.n)) for i, (_, c) in enumerate(self.shards)]

    def update_initialization_staged(self):
        self._check(self.L.almpc_group_update_initialization_staged(self.g, self._slots))

    def get_results_async(self, want=("u0", "status")) -> int:
        t = self.L.almpc_group_get_results_async(self.g, _want_mask(want))
        if t < 0:
            self._check(t)
        return t

    def get_results_wait(self, ticket, want=("u0", "status")):
        b, n, m, N = self.batch, self.n, self.m, self.N
        shapes = {"x": (b, N + 1, n), "e_x": (b, N + 1, n), "u": (b, N, m), "e_u": (b, N, m), "u0": (b, m),
                  "status": (b,), "iters": (b,), "polish_iters": (b,)}
        order = ("x", "e_x", "u", "e_u", "u0", "status", "iters", "polish_iters")
        bufs = {k: np.empty(shapes[k], dtype=np.int32 if k in ("status", "iters", "polish_iters") else np.float64) for k in set(want)}
        args = [(bufs[k].ctypes.data_as(_ip if bufs[k].dtype == np.int32 else _dp) if k in bufs else None) for k in order]
        self._check(self.L.almpc_group_get_results_wait(self.g, int(ticket), *args))
        for k in ("x", "e_x", "u", "e_u"):
            if k in bufs: bufs[k] = bufs[k].transpose(0, 2, 1)
        return bufs

    def close(self):
        if getattr(self, "g", None):
            for hv in self.handles:
                hv.close()
            self.L.almpc_group_destroy(self.g)
            self.g = None

    __del__ = close

    def design_shared(self, A, B, Q, R, S=None, P=None, umin=None, umax=None, xmin=None, xmax=None, rho=0.1, sigma=1e-6,
                      terminal="none", rho_profile="scalar"):
        n, m = self.n, self.m
        for hv in self.handles:   # per-handle options go through the handles (almpc_group_handle)
            hv._check(self.L.almpc_set_terminal_equality(hv.h, 1 if terminal == "equality" else 0))
            hv._check(self.L.almpc_set_rho_profile(hv.h, {"scalar": 0, "stiffness": 1}[rho_profile]))
        A, B, Q, R = _colmajor(A, (n, n)), _colmajor(B, (n, m)), _colmajor(Q, (n, n)), _colmajor(R, (m, m))
        S = None if S is None else _colmajor(S, (m, m))
        P = None if P is None else _colmajor(P, (n, n))
        umin = np.ascontiguousarray(umin, dtype=np.float64).reshape(m)
        umax = np.ascontiguousarray(umax, dtype=np.float64).reshape(m)
        xmin = None if xmin is None else np.ascontiguousarray(xmin, dtype=np.float64).reshape(n)
        xmax = None if xmax is None else np.ascontiguousarray(xmax, dtype=np.float64).reshape(n)
        self._check(self.L.almpc_group_design_shared(self.g, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(S), _ptr(P), _ptr(umin),
                                                     _ptr(umax), _ptr(xmin), _ptr(xmax), float(rho), float(sigma)))

    def set_reference(self, x_ref, u_ref, per_instance=False):
        n, m, N = self.n, self.m, self.N
        x_ref, u_ref = np.asarray(x_ref, dtype=np.float64), np.asarray(u_ref, dtype=np.float64)
        if per_instance:
            xr = np.ascontiguousarray(x_ref.reshape(self.batch, n, N + 1).transpose(0, 2, 1))
            ur = np.ascontiguousarray(u_ref.reshape(self.batch, m, N).transpose(0, 2, 1))
        else:
            xr = np.ascontiguousarray(x_ref.reshape(n, N + 1).T)
            ur = np.ascontiguousarray(u_ref.reshape(m, N).T)
        self._check(self.L.almpc_group_set_reference(self.g, _ptr(xr), _ptr(ur), 1 if per_instance else 0))

    def update_initialization(self, x0, resident=False):
        """x0 (batch, n) to the handles' shards.  Default: almpc_group_update_initialization (pinned slots read in place by the next
        step, no device copy -- the per-step path).  resident=True: a device copy per handle (almpc_update_initialization), for states
        that many steps will read (the pinned slot costs every step its transfer over the link)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(self.batch, self.n)
        if resident:
            for hv, (f, c) in zip(self.handles, self.shards):
                hv.update_initialization(x0[f:f + c])
            return
        self._check(self.L.almpc_group_update_initialization(self.g, _ptr(x0)))

    def calculate(self, opts: almpc_opts | None = None, sync=True):
        fn = self.L.almpc_group_calculate if sync else self.L.almpc_group_calculate_async
        self._check(fn(self.g, None if opts is None else ctypes.byref(opts)))

    def synchronize(self):
        self._check(self.L.almpc_group_synchronize(self.g))

    def sensitivity(self, want=("K0", "dU", "dX"), act_tol=0.0) -> dict:
        """Solver.sensitivity for the whole batch (almpc_group_sensitivity + almpc_group_get_sensitivity)."""
        self._check(self.L.almpc_group_sensitivity(self.g, _sens_mask(want), float(act_tol)))
        return _sens_read(self.L.almpc_group_get_sensitivity, self.g, self._check, want, self.batch, self.n, self.m, self.N)

    def certificate(self, want=("cost", "res", "grad", "costate")) -> dict:
        """Solver.certificate for the whole batch (almpc_group_certificate + almpc_group_get_certificate)."""
        self._check(self.L.almpc_group_certificate(self.g, _cert_mask(want)))
        return _cert_read(self.L.almpc_group_get_certificate, self.g, self._check, want, self.batch, self.n, self.m, self.N)

    def relin_fnn_certificate(self, want=("cost", "res", "grad", "costate")) -> dict:
        """Solver.relin_fnn_certificate for the whole batch (almpc_group_relin_fnn_certificate + almpc_group_get_certificate)."""
        self._check(self.L.almpc_group_relin_fnn_certificate(self.g, _cert_mask(want)))
        return _cert_read(self.L.almpc_group_get_certificate, self.g, self._check, want, self.batch, self.n, self.m, self.N)

    def sensitivity_vjp(self, g_u, g_x=None, act_tol=0.0):
        """Solver.sensitivity_vjp for the whole batch (almpc_group_sensitivity_vjp)."""
        return _sens_vjp(self.L.almpc_group_sensitivity_vjp, self.g, self._check, g_u, g_x, act_tol, self.batch, self.n, self.m, self.N)

    def sensitivity_stagewise(self, want=("K0", "dU", "dX"), act_tol=0.0) -> dict:
        """Solver.sensitivity_stagewise for the whole batch (almpc_group_sensitivity_stagewise + almpc_group_get_sensitivity)."""
        self._check(self.L.almpc_group_sensitivity_stagewise(self.g, _sens_mask(want), float(act_tol)))
        return _sens_read(self.L.almpc_group_get_sensitivity, self.g, self._check, want, self.batch, self.n, self.m, self.N)

    def sensitivity_stagewise_vjp(self, g_u, g_x=None, act_tol=0.0):
        """Solver.sensitivity_stagewise_vjp for the whole batch (almpc_group_sensitivity_stagewise_vjp)."""
        return _sens_vjp(self.L.almpc_group_sensitivity_stagewise_vjp, self.g, self._check, g_u, g_x, act_tol, self.batch, self.n, self.m,
                         self.N)

    def sensitivity_stagewise_rate(self, want=("K0", "dU", "dX"), act_tol=0.0) -> dict:
        """Solver.sensitivity_stagewise_rate for the whole batch (almpc_group_sensitivity_stagewise_rate + almpc_group_get_sensitivity)."""
        self._check(self.L.almpc_group_sensitivity_stagewise_rate(self.g, _sens_mask(want), float(act_tol)))
        return _sens_read(self.L.almpc_group_get_sensitivity, self.g, self._check, want, self.batch, self.n, self.m, self.N)

    def sensitivity_stagewise_rate_vjp(self, g_u, g_x=None, act_tol=0.0):
        """Solver.sensitivity_stagewise_rate_vjp for the whole batch (almpc_group_sensitivity_stagewise_rate_vjp)."""
        return _sens_vjp(self.L.almpc_group_sensitivity_stagewise_rate_vjp, self.g, self._check, g_u, g_x, act_tol, self.batch, self.n,
                         self.m, self.N)

    def sensitivity_params_vjp(self, g_u, g_x=None, want=PARAM_GROUPS, act_tol=0.0, terminal="data") -> dict:
        """Solver.sensitivity_params_vjp for the whole batch (almpc_group_sensitivity_params_vjp, almpc_group_sensitivity_params_vjp_dare)."""
        dare = _terminal_gradient(terminal)
        call = self.L.almpc_group_sensitivity_params_vjp_dare if dare else self.L.almpc_group_sensitivity_params_vjp
        return _sens_params_vjp(call, self.g, self._check, g_u, g_x, want, act_tol, self.batch, self.n, self.m, self.N, dare)

    def sensitivity_rows(self, want=("K0", "dU", "dX"), act_tol_u=0.0, act_tol_x=0.0) -> dict:
        """Solver.sensitivity_rows for the whole batch (almpc_group_sensitivity_rows + almpc_group_get_sensitivity)."""
        self._check(self.L.almpc_group_sensitivity_rows(self.g, _sens_mask(want), float(act_tol_u), float(act_tol_x)))
        return _sens_read(self.L.almpc_group_get_sensitivity, self.g, self._check, want, self.batch, self.n, self.m, self.N)

    def sensitivity_rows_vjp(self, g_u, g_x=None, act_tol_u=0.0, act_tol_x=0.0):
        """Solver.sensitivity_rows_vjp for the whole batch (almpc_group_sensitivity_rows_vjp)."""
        return _sens_vjp(self.L.almpc_group_sensitivity_rows_vjp, self.g, self._check, g_u, g_x, (act_tol_u, act_tol_x), self.batch, self.n,
                         self.m, self.N)

    def get_results(self, want=("x", "e_x", "u", "e_u", "status", "iters", "polish_iters")):
        b, n, m, N = self.batch, self.n, self.m, self.N
        shapes = {"x": (b, N + 1, n), "e_x": (b, N + 1, n), "u": (b, N, m), "e_u": (b, N, m), "u0": (b, m),
                  "status": (b,), "iters": (b,), "polish_iters": (b,)}
        order = ("x", "e_x", "u", "e_u", "u0", "status", "iters", "polish_iters")
        _want_mask(want)
        bufs = {k: np.empty(shapes[k], dtype=np.int32 if k in ("status", "iters", "polish_iters") else np.float64) for k in set(want)}
        args = [(bufs[k].ctypes.data_as(_ip if bufs[k].dtype == np.int32 else _dp) if k in bufs else None) for k in order]
        self._check(self.L.almpc_group_get_results(self.g, *args))
        for k in ("x", "e_x", "u", "e_u"):
            if k in bufs: bufs[k] = bufs[k].transpose(0, 2, 1)
        return bufs
