"""Host-side behaviour of the per-instance terminal-weight calls (include/almpc.h: almpc_dare_batched, almpc_set_terminal_weight,
almpc_relin_fnn_terminal_status, almpc_get_terminal_weight_instance) and of the mirror's kw mpc_terminal_weight: what must hold
without a GPU.  The numerical tests are tests/test_gpu_dare.py."""
import ctypes

import numpy as np
import pytest

ERR_INVALID, ERR_NO_DEVICE = -1, -2


def test_dare_batched_has_no_cpu_path(capi):
    """Without a usable device the call returns ALMPC_ERR_NO_DEVICE and writes nothing: never a host computation.  (Device 0 exists
    on a GPU machine and the call then computes; a device id past the last one is refused on every machine.)"""
    rng = np.random.default_rng(0)
    A, B = 0.5 * rng.standard_normal((3, 4, 4)), rng.standard_normal((3, 4, 2))
    L = capi.load()
    Ac, Bc = np.ascontiguousarray(A.transpose(0, 2, 1)), np.ascontiguousarray(B.transpose(0, 2, 1))
    Q, R = 100.0 * np.eye(4), 0.1 * np.eye(2)
    codes = []
    for device in (0, 1 << 20):
        P = np.full(3 * 16, 7.25)
        st = np.full(3, -9, dtype=np.int32)
        rc = L.almpc_dare_batched(device, 4, 2, 3, capi._ptr(Ac), capi._ptr(Bc), capi._ptr(Q), capi._ptr(R), capi._ptr(P),
                                  st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        codes.append(rc)
        if rc == ERR_NO_DEVICE:
            assert np.all(P == 7.25) and np.all(st == -9)
        else:
            assert rc == 0 and np.all(st == 0) and np.all(P != 7.25)
    assert codes[1] == ERR_NO_DEVICE and codes[0] in (0, ERR_NO_DEVICE)
    if codes[0] == ERR_NO_DEVICE:
        with pytest.raises(capi.AlmpcError) as e:
            capi.dare_batched(A, B, Q, R)
        assert e.value.code == ERR_NO_DEVICE


def test_dare_batched_argument_checks(capi):
    L = capi.load()
    A, B, Q, R, P = np.eye(2).ravel(), np.ones(2), np.eye(2).ravel(), np.ones(1), np.zeros(4)
    st = np.zeros(1, dtype=np.int32)
    ip = st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert L.almpc_dare_batched(0, 2, 1, 1, None, capi._ptr(B), capi._ptr(Q), capi._ptr(R), capi._ptr(P), ip) == ERR_INVALID
    assert L.almpc_dare_batched(0, 2, 1, 0, capi._ptr(A), capi._ptr(B), capi._ptr(Q), capi._ptr(R), capi._ptr(P), ip) == ERR_INVALID
    assert L.almpc_dare_batched(0, 2, 1, 1, capi._ptr(A), capi._ptr(B), capi._ptr(Q), capi._ptr(R), capi._ptr(P), None) == ERR_INVALID
    with pytest.raises(ValueError):
        capi.dare_batched(np.zeros((3, 4, 4)), np.zeros((2, 4, 2)), np.eye(4), np.eye(2))


def test_null_handle_calls_are_refused(capi):
    L = capi.load()
    st = np.zeros(4, dtype=np.int32)
    P = np.zeros(16)
    assert L.almpc_set_terminal_weight(None, 1) == ERR_INVALID
    assert L.almpc_relin_fnn_terminal_status(None, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == ERR_INVALID
    assert L.almpc_get_terminal_weight_instance(None, 0, capi._ptr(P)) == ERR_INVALID
    assert L.almpc_group_set_terminal_weight(None, 1) == ERR_INVALID
    with pytest.raises(ValueError):
        capi._terminal_mode("sometimes")


def test_controller_rejects_a_bad_terminal_weight_mode(pkg, mo):
    """mpc_terminal_weight is "reference" or "step", and "step" only with mpc_linearization = "step" (checked before any GPU call)."""
    f = mo.synthetic_fnn()
    bb = pkg.ConstrainedBlackBoxControlDiscreteSystem(pkg.Fnn(f.W_in, f.W_h, f.b_h, f.W_out, f.act), 4, 2,
                                                      pkg.Hyperrectangle([-10] * 4, [10] * 4), pkg.Hyperrectangle([-1, -1], [1, 1]))
    x_ref, u_ref = [0.2, -0.1, 0.05, 0.0], [0.1, -0.2]
    with pytest.raises(ValueError, match="mpc_terminal_weight"):
        pkg.proceed_controller(bb, "model_predictive_control", 10, 1, x_ref, u_ref, mpc_linearization="step", mpc_terminal_weight="always")
    with pytest.raises(ValueError, match="mpc_terminal_weight"):
        pkg.proceed_controller(bb, "model_predictive_control", 10, 1, x_ref, u_ref, mpc_terminal_weight="step")
    with pytest.raises(ValueError, match="mpc_terminal_weight"):
        pkg.proceed_controller(bb, "model_predictive_control", 10, 1, x_ref, u_ref, mpc_linearization="reference", mpc_terminal_weight="step")
    p = mo.double_integrator()
    lin = pkg.ConstrainedLinearControlDiscreteSystem(p.A, p.B, pkg.Hyperrectangle([-10, -10], [10, 10]), pkg.Hyperrectangle(p.u_min, p.u_max))
    with pytest.raises(ValueError, match="mpc_terminal_weight"):
        pkg.proceed_controller(lin, "model_predictive_control", 10, 1, [0.0, 0.0], [0.0], mpc_terminal_weight="step")
