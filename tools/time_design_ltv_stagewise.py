"""Time time-varying designs on the stage-wise solvers (almpc_design_ltv_stagewise, almpc_ltv_stagewise_update: k_ltv_stage_prepare,
k_ltv_stage_finish around k_riccati_t / k_sgains + k_sdual) in one run on one device:
    python tools/time_design_ltv_stagewise.py [reps=10]
  1. shapes both routes serve, (4, 2, 50) x 256 and (12, 4, 30) x 4096, input box: one outer iteration (data in -> u out) by
     almpc_design_ltv + almpc_calculate on a condensed handle beside almpc_ltv_stagewise_update + almpc_calculate on a structured one, in
     the host form and in the device form;
  2. a shape only the new route serves, (12, 4, 50) x 4096, with an input box, with S = 0.05 I and with a state box: the step alone, and
     the update alone in the device form (copies + k_ltv_stage_prepare) beside the bytes it moves over the achievable HBM rate.
Host clocks around calls that end in a wait for the handle's stream (best and median after a warm-up call).  The device arrays come from
the HIP runtime the library is linked against (ctypes on the libamdhip64 mapped into the process)."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402
import almpc_loader  # noqa: E402

capi = almpc_loader.load_package()._capi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
HBM = 6.3e12   # bytes / s a streaming kernel reaches on an MI355X (8 TB/s on paper)


def clock(call):
    call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def show(name, t, ref=None):
    print(f"    {name:46s} {1e3 * t[0]:9.3f} ms best, {1e3 * t[1]:9.3f} ms median" + ("" if ref is None else f"; {ref[0] / t[0]:6.2f} x"), flush=True)


def hip():
    with open("/proc/self/maps") as f:
        lib = ctypes.CDLL(next(ln.split()[-1] for ln in f if "libamdhip64" in ln))
    lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.hipFree.argtypes = [ctypes.c_void_p]
    return lib


def on_device(s, d):
    """the five arrays in the C layout in device memory: (addresses, bytes); never freed (a tool)"""
    n, m, N, b = s.n, s.m, s.N, s.batch
    host = [capi._blocks(d["A_all"], b * N, n, n), capi._blocks(d["B_all"], b * N, n, m), np.ascontiguousarray(d["c_all"]),
            capi._traj_batch(d["xbar"], b, n, N + 1), capi._traj_batch(d["ubar"], b, m, N)]
    h, out = hip(), []
    for a in host:
        p = ctypes.c_void_p()
        assert h.hipMalloc(ctypes.byref(p), a.nbytes) == 0 and h.hipMemcpy(p.value, a.ctypes.data, a.nbytes, 1) == 0
        out.append(p.value)
    return out, sum(a.nbytes for a in host)


def data(n, m, N, b, xs=1.0):
    rng = np.random.default_rng(100 * n + N)
    A1 = np.stack([0.9 * np.eye(n) + 0.15 * rng.standard_normal((n, n)) / np.sqrt(n / 4.0) for _ in range(N)])
    d = dict(A_all=np.broadcast_to(A1, (b, N, n, n)) + 0.01 * rng.standard_normal((b, 1, n, n)), B_all=rng.standard_normal((b, N, n, m)),
             c_all=0.1 * rng.standard_normal((b, N, n)), xbar=xs * rng.standard_normal((b, n, N + 1)),
             ubar=np.clip(0.3 * rng.standard_normal((b, m, N)), -0.6, 0.8))
    w = dict(x_ref=0.2 * rng.standard_normal((n, N + 1)), u_ref=0.1 * rng.standard_normal((m, N)), Q=10.0 * np.eye(n), R=np.eye(m),
             P=25.0 * np.eye(n) + 0.2 * np.ones((n, n)), umin=-0.6 * np.ones(m), umax=0.8 * np.ones(m))
    return d, w


def five(d):
    return d["A_all"], d["B_all"], d["c_all"], d["xbar"], d["ubar"]


def both_routes(n, m, N, b):
    d, w = data(n, m, N, b)
    print(f"({n}, {m}, {N}) x {b}, input box: one outer iteration, data in -> u out", flush=True)
    c = capi.Solver(n, m, N, b)

    def condensed():
        c.design_ltv(*five(d), w["x_ref"], w["u_ref"], w["Q"], w["R"], None, w["P"], w["umin"], w["umax"])
        c.update_initialization(d["xbar"][:, :, 0])
        c.calculate()
    t_c = clock(condensed)
    uc = c.get_results(want=("u", "status"))
    c.close()
    s = capi.Solver(n, m, N, b, structured=True)
    s.design_ltv_stagewise(*five(d), w["x_ref"], w["u_ref"], w["Q"], w["R"], None, w["P"], w["umin"], w["umax"])

    def host():
        s.ltv_stagewise_update(*five(d))
        s.calculate()
    t_h = clock(host)
    ptrs, _ = on_device(s, d)

    def dev():
        s.ltv_stagewise_update(*ptrs, on_device=True)
        s.calculate()
    t_d = clock(dev)
    us = s.get_results(want=("u", "status"))
    s.close()
    ok = (uc["status"] == 0) & (us["status"] == 0)
    print(f"    solved on both routes: {int(ok.sum())} of {b}; max |u_condensed - u_stagewise| on them {np.abs(uc['u'][ok] - us['u'][ok]).max():.2e}")
    show("almpc_design_ltv + calculate (condensed)", t_c)
    show("ltv_stagewise_update (host form) + calculate", t_h, t_c)
    show("ltv_stagewise_update (device form) + calculate", t_d, t_c)


def new_route_only(n, m, N, b):
    for name, S, box in (("input box", None, None), ("S = 0.05 I", 0.05 * np.eye(m), None), ("state box +-0.9", None, 0.9)):
        d, w = data(n, m, N, b, xs=0.3 if box else 1.0)
        s = capi.Solver(n, m, N, b, structured=True)
        kw = {} if box is None else dict(xmin=-box * np.ones(n), xmax=box * np.ones(n))
        s.design_ltv_stagewise(*five(d), w["x_ref"], w["u_ref"], w["Q"], w["R"], S, w["P"], w["umin"], w["umax"], **kw)
        ptrs, nbytes = on_device(s, d)
        s.calculate()
        st = s.get_results(want=("status",))["status"]
        print(f"({n}, {m}, {N}) x {b}, {name}: status {np.bincount(st, minlength=4).tolist()}", flush=True)

        def step():
            s.calculate(sync=False)
            s.synchronize()

        def upd():
            s.ltv_stagewise_update(*ptrs, on_device=True)
            s.synchronize()
        show("step (almpc_calculate)", clock(step))
        t_u = clock(upd)
        xu = 8 * b * ((N + 1) * n + N * m)
        moved = 2 * (nbytes - xu) + 3 * xu   # A, B, c read and written once; xbar, ubar read, copied and turned into ebar, qadd
        show("update alone (device form)", t_u)
        print(f"    it moves {moved / 1e6:.0f} MB: {1e3 * moved / HBM:.3f} ms at {HBM / 1e12:.1f} TB/s; measured / floor {t_u[0] * HBM / moved:.2f}", flush=True)
        s.close()


both_routes(4, 2, 50, 256)
both_routes(12, 4, 30, 4096)
new_route_only(12, 4, 50, 4096)
