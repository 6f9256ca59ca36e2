"""Host side of the continuous-time models (include/almpc.h: almpc_c2d, almpc_c2d_batched, almpc_set_model_time,
almpc_get_model_instance, almpc_group_set_model_time; controller.py: the continuous system types): what must hold without a GPU.
The device tests are tests/test_gpu_c2d.py; shared definitions in tests/c2d_ref.py."""
import ctypes
import importlib

import numpy as np
import pytest

import c2d_ref as cr

ERR_INVALID, ERR_NO_DEVICE, ERR_NUMERIC = -1, -2, -6


@pytest.mark.parametrize("n,m", cr.SHAPES)
def test_host_c2d_matches_scipy(capi, n, m):
    """almpc_c2d (hm::c2d) against scipy's expm of the augmented matrix, 67 models per shape at three sample times, and the numpy
    restatement of the same algorithm beside it.  Measured: the largest error of both over all shapes and sample times is 5.4e-13
    ((1, 1) at Ts = 5, six doublings of exp(-Ts a) with a near 2); the bound is 1e-10."""
    A, B = cr.models(n, m)
    for Ts in cr.SAMPLE_TIMES:
        Ad_t, Bd_t = cr.truth(n, m, Ts)
        worst = worst_ref = 0.0
        for i in range(cr.BATCH):
            Ad, Bd = capi.c2d(A[i], B[i], Ts)
            worst = max(worst, cr.c2d_error(Ad, Bd, Ad_t[i], Bd_t[i]))
            r = cr.c2d_ref(A[i], B[i], Ts)
            worst_ref = max(worst_ref, cr.c2d_error(r[0], r[1], Ad_t[i], Bd_t[i]))
            assert cr.c2d_error(Ad, Bd, r[0], r[1]) <= 1e-12   # the restatement and the library follow the same steps
        print(f"n {n} m {m} Ts {Ts}: almpc_c2d {worst:.3e}, numpy restatement {worst_ref:.3e}")
        assert worst <= cr.TOL and worst_ref <= cr.TOL


def test_quadrotor_and_double_integrator(capi, pkg):
    wl = importlib.import_module(pkg.__name__ + ".workloads")
    Ac, Bc = wl.quadrotor_continuous_model()
    Ad, Bd = capi.c2d(Ac, Bc, 0.1)
    A, B = wl.quadrotor_model()
    err = cr.c2d_error(Ad, Bd, A, B)
    print(f"quadrotor, Ts 0.1: {err:.3e}")
    assert err <= cr.TOL
    # a singular A needs no special case; every operation of this one is exact
    Ad, Bd = capi.c2d([[0.0, 1.0], [0.0, 0.0]], [[0.0], [1.0]], 1.0)
    assert np.array_equal(Ad, [[1.0, 1.0], [0.0, 1.0]]) and np.array_equal(Bd, [[0.5], [1.0]])


def test_bad_arguments_leave_the_outputs_untouched(capi):
    L = capi.load()
    A, B = np.array([[0.0, 1.0], [0.0, 0.0]], order="F"), np.array([[0.0], [1.0]], order="F")
    Anan = A.copy(order="F")
    Anan[1, 0] = np.nan
    for Am, Ts, code in ((A, 0.0, ERR_INVALID), (A, -1.0, ERR_INVALID), (A, np.nan, ERR_INVALID), (A, np.inf, ERR_INVALID),
                         (Anan, 1.0, ERR_NUMERIC), (1e300 * A, 1.0, ERR_NUMERIC)):
        Ad, Bd = np.full(4, 7.25), np.full(2, 7.25)
        assert L.almpc_c2d(2, 1, capi._ptr(Am), capi._ptr(B), Ts, capi._ptr(Ad), capi._ptr(Bd)) == code, (Ts, code)
        assert np.all(Ad == 7.25) and np.all(Bd == 7.25)
    Ad, Bd = np.zeros(4), np.zeros(2)
    assert L.almpc_c2d(2, 1, None, capi._ptr(B), 1.0, capi._ptr(Ad), capi._ptr(Bd)) == ERR_INVALID
    assert L.almpc_c2d(2, 1, capi._ptr(A), capi._ptr(B), 1.0, None, capi._ptr(Bd)) == ERR_INVALID
    assert L.almpc_c2d(0, 1, capi._ptr(A), capi._ptr(B), 1.0, capi._ptr(Ad), capi._ptr(Bd)) == ERR_INVALID
    with pytest.raises(capi.AlmpcError) as e:
        capi.c2d(Anan, B, 1.0)
    assert e.value.code == ERR_NUMERIC
    assert cr.c2d_ref(Anan, B, 1.0) is None and cr.c2d_ref(1e300 * A, B, 1.0) is None


def test_c2d_batched_has_no_cpu_path(capi):
    """Without a usable device the call returns ALMPC_ERR_NO_DEVICE and writes nothing: never a host computation.  (Device 0 exists
    on a GPU machine and the call then computes; a device id past the last one is refused on every machine.)"""
    A, B = cr.models(4, 2, 3)
    L = capi.load()
    Ac, Bc = np.ascontiguousarray(A.transpose(0, 2, 1)), np.ascontiguousarray(B.transpose(0, 2, 1))
    ip = ctypes.POINTER(ctypes.c_int32)
    codes = []
    for device in (0, 1 << 20):
        Ad, Bd = np.full(3 * 16, 7.25), np.full(3 * 8, 7.25)
        st = np.full(3, -9, dtype=np.int32)
        rc = L.almpc_c2d_batched(device, 4, 2, 3, capi._ptr(Ac), capi._ptr(Bc), 0.5, capi._ptr(Ad), capi._ptr(Bd), st.ctypes.data_as(ip))
        codes.append(rc)
        if rc == ERR_NO_DEVICE:
            assert np.all(Ad == 7.25) and np.all(Bd == 7.25) and np.all(st == -9)
        else:
            assert rc == 0 and np.all(st == 0) and np.all(Ad != 7.25) and np.all(Bd != 7.25)
    assert codes[1] == ERR_NO_DEVICE and codes[0] in (0, ERR_NO_DEVICE)
    if codes[0] == ERR_NO_DEVICE:
        with pytest.raises(capi.AlmpcError) as e:
            capi.c2d_batched(A, B, 0.5)
        assert e.value.code == ERR_NO_DEVICE


def test_c2d_batched_argument_checks(capi):
    L = capi.load()
    A, B, Ad, Bd = np.eye(2).ravel(), np.ones(2), np.zeros(4), np.zeros(2)
    st = np.zeros(1, dtype=np.int32)
    ip = st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    p = capi._ptr
    assert L.almpc_c2d_batched(0, 2, 1, 1, None, p(B), 1.0, p(Ad), p(Bd), ip) == ERR_INVALID
    assert L.almpc_c2d_batched(0, 2, 1, 0, p(A), p(B), 1.0, p(Ad), p(Bd), ip) == ERR_INVALID
    assert L.almpc_c2d_batched(0, 2, 1, 1, p(A), p(B), 1.0, p(Ad), p(Bd), None) == ERR_INVALID
    assert L.almpc_c2d_batched(0, 2, 1, 1, p(A), p(B), 0.0, p(Ad), p(Bd), ip) == ERR_INVALID
    assert L.almpc_c2d_batched(0, 2, 1, 1, p(A), p(B), np.nan, p(Ad), p(Bd), ip) == ERR_INVALID
    with pytest.raises(ValueError):
        capi.c2d_batched(np.zeros((3, 4, 4)), np.zeros((2, 4, 2)), 1.0)


def test_null_handle_calls_are_refused(capi):
    L = capi.load()
    A, B = np.zeros(16), np.zeros(8)
    assert L.almpc_set_model_time(None, 1, 0.1) == ERR_INVALID
    assert L.almpc_get_model_instance(None, 0, capi._ptr(A), capi._ptr(B)) == ERR_INVALID
    assert L.almpc_group_set_model_time(None, 1, 0.1) == ERR_INVALID
    with pytest.raises(ValueError):
        capi._model_time_mode("sometimes")
    assert capi._model_time_mode("continuous") == 1 and capi._model_time_mode("discrete") == 0


def test_continuous_system_types_validate_as_their_discrete_twins(pkg):
    X, U = pkg.Hyperrectangle([-1, -1], [1, 1]), pkg.Hyperrectangle([-1], [1])
    s = pkg.ConstrainedLinearControlContinuousSystem([[0.0, 1.0], [0.0, 0.0]], [[0.0], [1.0]], X, U)
    assert s.A.dtype == np.float64 and s.B.shape == (2, 1)
    assert not isinstance(s, pkg.ConstrainedLinearControlDiscreteSystem)
    with pytest.raises(ValueError, match="Continuous"):
        pkg.ConstrainedLinearControlContinuousSystem(np.zeros((3, 3)), [[0.0], [1.0]], X, U)
    with pytest.raises(ValueError):
        pkg.ConstrainedLinearControlContinuousSystem(np.zeros((2, 2)), [[0.0], [1.0]], X, pkg.Hyperrectangle([-1, -1], [1, 1]))


def test_controller_rejects_non_linear_with_a_continuous_black_box_system(pkg, mo):
    """mpc_programming_type = "non_linear" has no continuous-time form (the NLP would need an integrator): NotImplementedError before any
    GPU call."""
    f = mo.synthetic_fnn()
    bb = pkg.ConstrainedBlackBoxControlContinuousSystem(pkg.Fnn(f.W_in, f.W_h, f.b_h, f.W_out, f.act), 4, 2,
                                                        pkg.Hyperrectangle([-10] * 4, [10] * 4), pkg.Hyperrectangle([-1, -1], [1, 1]))
    with pytest.raises(NotImplementedError, match="continuous"):
        pkg.proceed_controller(bb, "model_predictive_control", 10, 1, [0.2, -0.1, 0.05, 0.0], [0.1, -0.2], mpc_programming_type="non_linear")
