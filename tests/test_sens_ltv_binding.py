"""Solver.sensitivity_ltv and Solver.sensitivity_ltv_vjp through the recording stand-in for libalmpc.so of tests/capi_trace.py: the C calls
they make (symbols, scalars, the size and the bytes of every buffer) and the shapes, strides and contents of what they return.  No GPU
and no library are needed.  (The stand-in fills every output buffer with the element index in memory order plus 1000 times the
argument's position.)"""
import contextlib

import numpy as np
import pytest

import capi_trace

n, m, N, b = 3, 2, 4, 7   # no two extents equal


@contextlib.contextmanager
def recorded(capi):
    log = []
    lib = capi_trace.RecordingLib(log)
    before, capi._lib = capi._lib, lib
    try:
        s = capi.Solver(n, m, N, b)
        del log[:]
        yield s, lib, log
    finally:
        capi._lib = before


def _c_calls(log):
    return [ln for ln in log if ln.startswith("C ")]


def test_prototypes_are_those_of_the_header(pkg):
    capi = pkg._capi
    decl, table = capi_trace.declarations(), capi.prototypes()
    assert [t for t, _ in decl["almpc_sensitivity_ltv"][1]] == ["almpc_handle *", "uint32_t", "double"]
    assert [t for t, _ in decl["almpc_sensitivity_ltv_vjp"][1]] == ["almpc_handle *", "const double *", "const double *", "double", "double *", "int32_t *"]
    assert table["almpc_sensitivity_ltv"] == table["almpc_sensitivity_stagewise"]
    assert table["almpc_sensitivity_ltv_vjp"] == table["almpc_sensitivity_stagewise_vjp"]
    assert "almpc_group_sensitivity_ltv" not in table and "almpc_group_sensitivity_ltv" not in decl


def test_jacobians_are_marshalled_and_shaped_like_the_stagewise_form(pkg):
    capi = pkg._capi
    with recorded(capi) as (s, lib, log):
        out = s.sensitivity_ltv()
        calls = _c_calls(log)
        assert calls == [f"C almpc_sensitivity_ltv(h=H0, want=7, act_tol=0.0)",
                         f"C almpc_get_sensitivity(h=H0, K0=f8[{8 * b * n * m}], dU=f8[{8 * b * n * N * m}], dX=f8[{8 * b * n * (N + 1) * n}], rows=i4[{4 * b}])"]
        assert out["K0"].shape == (b, m, n) and out["dU"].shape == (b, m, N, n) and out["dX"].shape == (b, n, N + 1, n) and out["rows"].shape == (b,)
        # the C layouts [batch][n][m], [batch][n][N][m], [batch][n][N+1][n], seen Julia-shaped: [b, i, k, c] = d(entry i of stage k) / d x0[c]
        assert np.array_equal(out["K0"], (1000 + np.arange(b * n * m)).reshape(b, n, m).transpose(0, 2, 1))
        assert np.array_equal(out["dU"], (2000 + np.arange(b * n * N * m)).reshape(b, n, N, m).transpose(0, 3, 2, 1))
        assert np.array_equal(out["dX"], (3000 + np.arange(b * n * (N + 1) * n)).reshape(b, n, N + 1, n).transpose(0, 3, 2, 1))
        assert out["rows"].dtype == np.int32 and np.array_equal(out["rows"], 4000 + np.arange(b))
        twin = s.sensitivity_stagewise()
        for k in out:
            assert capi_trace.describe(out[k]) == capi_trace.describe(twin[k]), k
        del log[:]
        part = s.sensitivity_ltv(("K0",), act_tol=1e-8)
        assert _c_calls(log) == ["C almpc_sensitivity_ltv(h=H0, want=1, act_tol=1e-08)",
                                 f"C almpc_get_sensitivity(h=H0, K0=f8[{8 * b * n * m}], dU=NULL, dX=NULL, rows=i4[{4 * b}])"]
        assert set(part) == {"K0", "rows"}
        del log[:]
        assert set(s.sensitivity_ltv("dX", 1)) == {"dX", "rows"}
        assert _c_calls(log)[0] == "C almpc_sensitivity_ltv(h=H0, want=4, act_tol=1.0)"
        for bad in ((), ("K0", "dV")):
            del log[:]
            with pytest.raises(ValueError):
                s.sensitivity_ltv(bad)
            assert not _c_calls(log)
        lib.fail_next = -4
        with pytest.raises(capi.AlmpcError) as e:
            s.sensitivity_ltv()
        assert e.value.code == -4 and "the stand-in's error text" in str(e.value)


def test_vjp_is_marshalled_and_shaped_like_the_stagewise_form(pkg):
    capi = pkg._capi
    rng = np.random.default_rng(5)
    g_u, g_x = rng.standard_normal((b, m, N)), rng.standard_normal((b, n, N + 1))
    with recorded(capi) as (s, lib, log):
        g_x0, rows = s.sensitivity_ltv_vjp(g_u, g_x)
        ltv = _c_calls(log)
        del log[:]
        twin = s.sensitivity_stagewise_vjp(g_u, g_x)
        assert ltv == [ln.replace("almpc_sensitivity_stagewise_vjp", "almpc_sensitivity_ltv_vjp") for ln in _c_calls(log)] and len(ltv) == 1
        # the loss gradients go down stage-major: [batch][N][m] and [batch][N+1][n]
        hu = capi_trace._h(np.ascontiguousarray(g_u.transpose(0, 2, 1)).tobytes())
        hx = capi_trace._h(np.ascontiguousarray(g_x.transpose(0, 2, 1)).tobytes())
        assert ltv[0] == (f"C almpc_sensitivity_ltv_vjp(h=H0, g_u=f8[{8 * b * N * m}]:{hu}, g_x=f8[{8 * b * (N + 1) * n}]:{hx}, act_tol=0.0, "
                          f"g_x0=f8[{8 * b * n}], rows=i4[{4 * b}])")
        assert g_x0.shape == (b, n) and rows.shape == (b,) and rows.dtype == np.int32
        assert np.array_equal(g_x0, (4000 + np.arange(b * n)).reshape(b, n)) and np.array_equal(rows, 5000 + np.arange(b))
        assert capi_trace.describe((g_x0, rows)) == capi_trace.describe(twin)
        del log[:]
        s.sensitivity_ltv_vjp(g_u, None, act_tol=1e-8)
        assert _c_calls(log) == [f"C almpc_sensitivity_ltv_vjp(h=H0, g_u=f8[{8 * b * N * m}]:{hu}, g_x=NULL, act_tol=1e-08, g_x0=f8[{8 * b * n}], rows=i4[{4 * b}])"]
        del log[:]
        with pytest.raises(ValueError):
            s.sensitivity_ltv_vjp(g_u[:, :, :-1])
        assert not _c_calls(log)
        lib.fail_next = -1
        with pytest.raises(capi.AlmpcError) as e:
            s.sensitivity_ltv_vjp(g_u)
        assert e.value.code == -1
