"""Time the sensitivities of a step of a time-varying design (almpc_sensitivity_ltv, almpc_sensitivity_ltv_vjp: k_sens_ltv) beside the step
and the certificate of the same handle, in one run, at (n, m, N) x batch = (4, 2, 50) x 256 and (12, 4, 30) x 4096, each with the
input-rate weight S (the recursion in [dx_k; du_(k-1)]) and without it.
    python tools/time_sensitivity_ltv.py [reps=50]
Per handle: the step, almpc_certificate_ltv with all its outputs, K0 alone (one backward sweep), all three Jacobians (the sweep, the gains
of every stage through the scratch, the forward pass) and the VJP (which includes the upload of g_u and g_x and the copy back of g_x0) --
each a host clock around a call that ends in a wait for the handle's stream (best and median after a warm-up call; the Jacobians stay on
the device), with its ratio to the step's best time.  Kernel times of k_sens_ltv: run the script under `rocprofv3 --kernel-trace --stats --
python tools/time_sensitivity_ltv.py` in a run of its own (tracing slows the host clocks)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402
import almpc_loader  # noqa: E402

capi = almpc_loader.load_package()._capi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
CERT_ALL = capi.CERT_LTV["cost"] | capi.CERT_LTV["res"] | capi.CERT_LTV["grad"] | capi.CERT_LTV["costate"] | capi.CERT_LTV["x"]
K0, JAC = capi.SENS["K0"], capi.SENS["K0"] | capi.SENS["dU"] | capi.SENS["dX"]


def clock(call):
    call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def ltv(n, m, N, b, with_S):
    rng = np.random.default_rng(100 * n + N)
    A_all = np.stack([[0.85 * np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n) for _ in range(N)] for _ in range(b)])
    B_all = rng.standard_normal((b, N, n, m))
    c_all = 0.05 * rng.standard_normal((b, N, n))
    xbar = rng.standard_normal((b, n, N + 1)); ubar = 0.2 * rng.standard_normal((b, m, N))
    x_ref = 0.2 * rng.standard_normal((n, N + 1)); u_ref = 0.1 * rng.standard_normal((m, N))
    Q, R, S, P = 10.0 * np.eye(n), 1.0 * np.eye(m), 0.3 * np.eye(m), 25.0 * np.eye(n) + 0.2 * np.ones((n, n))
    s = capi.Solver(n, m, N, b)
    s.design_ltv(A_all, B_all, c_all, xbar, ubar, x_ref, u_ref, Q, R, S if with_S else None, P, -0.5 * np.ones(m), 0.6 * np.ones(m),
                 keep_stage_models=True)
    s.update_initialization(xbar[:, :, 0])
    s.calculate()
    st = s.get_results(want=("status",))["status"]
    rows = s.sensitivity_ltv(("K0",))["rows"]
    print(f"LTV ({n}, {m}, {N}) x {b}, {'S != 0' if with_S else 'S = 0'}: status {np.bincount(st, minlength=4).tolist()}; rows at a bound "
          f"{rows.min()} .. {rows.max()} of {m * N}; gain scratch {b * N * m * (n + (m if with_S else 0)) * 8 / 1e6:.1f} MB", flush=True)

    def step():
        s.calculate(sync=False)
        s.synchronize()
    g_u, g_x = rng.standard_normal((b, m, N)), rng.standard_normal((b, n, N + 1))
    t_step = clock(step)
    for name, call in (("step", None),
                       ("certificate_ltv, all outputs", lambda: s._check(s.L.almpc_certificate_ltv(s.h, CERT_ALL))),
                       ("sensitivity_ltv K0", lambda: s._check(s.L.almpc_sensitivity_ltv(s.h, K0, 0.0))),
                       ("sensitivity_ltv K0 | dU | dX", lambda: s._check(s.L.almpc_sensitivity_ltv(s.h, JAC, 0.0))),
                       ("sensitivity_ltv_vjp", lambda: s.sensitivity_ltv_vjp(g_u, g_x))):
        t = t_step if call is None else clock(call)
        print(f"    {name:30s} {1e6 * t[0]:9.1f} us best, {1e6 * t[1]:9.1f} us median; {t[0] / t_step[0]:5.2f} steps", flush=True)
    s.close()


for shape in ((4, 2, 50, 256), (12, 4, 30, 4096)):
    for with_S in (True, False):
        ltv(*shape, with_S)
