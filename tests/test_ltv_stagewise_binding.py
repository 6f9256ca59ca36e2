"""Solver.design_ltv_stagewise, Solver.ltv_stagewise_update and Solver.ltv_stagewise_prepared through the recording stand-in for
libalmpc.so of tests/capi_trace.py: the C calls they make (symbols, scalars, the size and the bytes of every buffer) in the host form and
in the device form.  No GPU and no library are needed."""
import contextlib

import numpy as np
import pytest

import capi_trace

n, m, N, b = 3, 2, 4, 5   # no two extents equal


@contextlib.contextmanager
def recorded(capi):
    log = []
    lib = capi_trace.RecordingLib(log)
    before, capi._lib = capi._lib, lib
    try:
        s = capi.Solver(n, m, N, b, structured=True)
        del log[:]
        yield s, lib, log
    finally:
        capi._lib = before


def _c_calls(log):
    return [ln for ln in log if ln.startswith("C ")]


def _data(seed=0):
    rng = np.random.default_rng(seed)
    return dict(A_all=rng.standard_normal((b, N, n, n)), B_all=rng.standard_normal((b, N, n, m)), c_all=rng.standard_normal((b, N, n)),
                xbar=rng.standard_normal((b, n, N + 1)), ubar=rng.standard_normal((b, m, N)), x_ref=rng.standard_normal((n, N + 1)),
                u_ref=rng.standard_normal((m, N)), Q=rng.standard_normal((n, n)), R=rng.standard_normal((m, m)),
                S=rng.standard_normal((m, m)), P=rng.standard_normal((n, n)), umin=-np.ones(m), umax=np.ones(m))


def _f8(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return f"f8[{a.nbytes}]:{capi_trace._h(a.tobytes())}"


def _trajectory_args(d):
    """the five arrays as the C call must see them: column-major blocks [batch][N][.], stage-major trajectories"""
    return (f"A_all={_f8(d['A_all'].transpose(0, 1, 3, 2))}, B_all={_f8(d['B_all'].transpose(0, 1, 3, 2))}, "
            f"c_all={'NULL' if d['c_all'] is None else _f8(d['c_all'])}, xbar={_f8(d['xbar'].transpose(0, 2, 1))}, ubar={_f8(d['ubar'].transpose(0, 2, 1))}")


def test_prototypes_are_those_of_the_header(pkg):
    capi = pkg._capi
    decl, table = capi_trace.declarations(), capi.prototypes()
    dp, i = "const double *", "int"
    assert [t for t, _ in decl["almpc_design_ltv_stagewise"][1]] == ["almpc_handle *"] + [dp] * 11 + [i, dp, dp, i]
    assert [t for t, _ in decl["almpc_ltv_stagewise_update"][1]] == ["almpc_handle *"] + [dp] * 5 + [i]
    assert [t for t, _ in decl["almpc_get_ltv_stagewise_prepared"][1]] == ["almpc_handle *"] + ["double *"] * 3
    # the design call is almpc_design_ltv's with on_device in the place of rho, sigma; the update call is its first five arrays
    assert [nm for _, nm in decl["almpc_design_ltv_stagewise"][1]][:15] == [nm for _, nm in decl["almpc_design_ltv"][1]][:15]
    assert [nm for _, nm in decl["almpc_ltv_stagewise_update"][1]][:6] == [nm for _, nm in decl["almpc_design_ltv"][1]][:6]
    assert table["almpc_design_ltv_stagewise"][:15] == table["almpc_design_ltv"][:15] and len(table["almpc_design_ltv_stagewise"]) == 16
    for sym in ("almpc_design_ltv_stagewise", "almpc_ltv_stagewise_update", "almpc_get_ltv_stagewise_prepared"):
        assert sym in table and sym.replace("almpc_", "almpc_group_") not in table and sym.replace("almpc_", "almpc_group_") not in decl


def test_host_form(pkg):
    capi = pkg._capi
    d = _data()
    with recorded(capi) as (s, lib, log):
        s.design_ltv_stagewise(d["A_all"], d["B_all"], d["c_all"], d["xbar"], d["ubar"], d["x_ref"], d["u_ref"], d["Q"], d["R"], d["S"], d["P"],
                               d["umin"], d["umax"], xmin=-np.ones(n), xmax=2 * np.ones(n), terminal="equality")
        calls = _c_calls(log)
        assert calls[0] == "C almpc_set_terminal_equality(h=H0, on=1)"
        assert calls[1] == f"C almpc_set_state_box(h=H0, xmin={_f8(-np.ones(n))}, xmax={_f8(2 * np.ones(n))})"
        assert calls[2] == (f"C almpc_design_ltv_stagewise(h=H0, {_trajectory_args(d)}, xref={_f8(d['x_ref'].T)}, uref={_f8(d['u_ref'].T)}, "
                            f"Q={_f8(d['Q'].T)}, R={_f8(d['R'].T)}, S={_f8(d['S'].T)}, P={_f8(d['P'].T)}, P_per_instance=0, "
                            f"umin={_f8(d['umin'])}, umax={_f8(d['umax'])}, on_device=0)")
        assert len(calls) == 3
        del log[:]
        d2 = _data(1)
        s.ltv_stagewise_update(d2["A_all"], d2["B_all"], d2["c_all"], d2["xbar"], d2["ubar"])
        assert _c_calls(log) == [f"C almpc_ltv_stagewise_update(h=H0, {_trajectory_args(d2)}, on_device=0)"]
        del log[:]
        d2["c_all"] = None
        s.ltv_stagewise_update(d2["A_all"], d2["B_all"], None, d2["xbar"], d2["ubar"])
        assert _c_calls(log) == [f"C almpc_ltv_stagewise_update(h=H0, {_trajectory_args(d2)}, on_device=0)"]
        # no references, no S, one terminal weight per instance, no state rows
        del log[:]
        Pb = np.random.default_rng(2).standard_normal((b, n, n))
        s.design_ltv_stagewise(d["A_all"], d["B_all"], None, d["xbar"], d["ubar"], None, None, d["Q"], d["R"], None, Pb, d["umin"], d["umax"])
        calls = _c_calls(log)
        assert calls[:2] == ["C almpc_set_terminal_equality(h=H0, on=0)", "C almpc_set_state_box(h=H0, xmin=NULL, xmax=NULL)"]
        assert ", c_all=NULL, " in calls[2] and ", xref=NULL, uref=NULL, " in calls[2] and ", S=NULL, " in calls[2]
        assert f"P={_f8(Pb.transpose(0, 2, 1))}, P_per_instance=1, " in calls[2]
        lib.fail_next = -4
        with pytest.raises(capi.AlmpcError) as e:
            s.ltv_stagewise_update(d["A_all"], d["B_all"], None, d["xbar"], d["ubar"])
        assert e.value.code == -4 and "the stand-in's error text" in str(e.value)
        with pytest.raises(ValueError):   # a wrong shape never reaches the library
            del log[:]
            s.ltv_stagewise_update(d["A_all"][:, :-1], d["B_all"], None, d["xbar"], d["ubar"])
        assert not _c_calls(log)


def test_device_form(pkg):
    capi = pkg._capi
    d = _data()
    with recorded(capi) as (s, lib, log):
        s.design_ltv_stagewise(0x1000, 0x2000, None, 0x3000, 0x4000, d["x_ref"], None, d["Q"], d["R"], None, d["P"], d["umin"], d["umax"],
                               on_device=True)
        call = _c_calls(log)[2]
        assert call.startswith("C almpc_design_ltv_stagewise(h=H0, A_all=LP_c_double, B_all=LP_c_double, c_all=NULL, xbar=LP_c_double, "
                               f"ubar=LP_c_double, xref={_f8(d['x_ref'].T)}, uref=NULL, ")
        assert call.endswith(", on_device=1)")
        del log[:]
        s.ltv_stagewise_update(0x1000, 0x2000, np.int64(0x5000), 0x3000, 0x4000, on_device=True)
        assert _c_calls(log) == ["C almpc_ltv_stagewise_update(h=H0, A_all=LP_c_double, B_all=LP_c_double, c_all=LP_c_double, xbar=LP_c_double, "
                                 "ubar=LP_c_double, on_device=1)"]
        for bad in ((d["A_all"], 0x2000, None, 0x3000, 0x4000), (0x1000, 0x2000, None, 0, 0x4000), (0x1000, 0x2000, d["c_all"], 0x3000, 0x4000)):
            del log[:]
            with pytest.raises(TypeError):   # an array (or a null address) where the device form takes an address
                s.ltv_stagewise_update(*bad, on_device=True)
            assert not _c_calls(log)


def test_the_addresses_reach_the_library(pkg):
    """What the device form hands down IS the address it was given (the stand-in records only the type)."""
    import ctypes
    capi = pkg._capi
    s = capi.Solver.__new__(capi.Solver)
    s.n, s.m, s.N, s.batch = n, m, N, b
    ptrs, keep = s._ltv_stage_data(0x1000, 0x2000, None, 0x3000, 0x4008, True)
    assert keep is None and ptrs[2] is None
    assert [ctypes.cast(p, ctypes.c_void_p).value for p in ptrs if p is not None] == [0x1000, 0x2000, 0x3000, 0x4008]


def test_prepared_read_back(pkg):
    capi = pkg._capi
    with recorded(capi) as (s, lib, log):
        out = s.ltv_stagewise_prepared()
        assert _c_calls(log) == [f"C almpc_get_ltv_stagewise_prepared(h=H0, ebar=f8[{8 * b * N * n}], qadd=f8[{8 * b * N * m}], eq_target=NULL)"]
        assert set(out) == {"ebar", "qadd"} and out["ebar"].shape == (b, N, n) and out["qadd"].shape == (b, N, m)
        assert np.array_equal(out["ebar"], (1000 + np.arange(b * N * n)).reshape(b, N, n))
        assert np.array_equal(out["qadd"], (2000 + np.arange(b * N * m)).reshape(b, N, m))
        del log[:]
        out = s.ltv_stagewise_prepared(eq_target=True)
        assert _c_calls(log)[0].endswith(f"eq_target=f8[{8 * n}])") and np.array_equal(out["eq_target"], 3000 + np.arange(n))
