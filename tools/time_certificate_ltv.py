"""Time the certificate of a step of a time-varying design (almpc_certificate_ltv, k_cert_ltv) beside the step of the same handle, in one
run, at (n, m, N) x batch = (4, 2, 50) x 256 and (12, 4, 30) x 4096, and almpc_relin_fnn_certificate beside almpc_relin_fnn_step at the
shape of BASELINE configs[3] (synthetic Fnn, 4-2, N = 20, 1024 instances).
    python tools/time_certificate_ltv.py [reps=50]
Per handle: the step, the certificate with COST | RES, with all six outputs -- each a host clock around a call that ends in a wait for the
handle's stream (best and median after a warm-up call; the results stay on the device), the bytes one launch moves, computed from the
shapes, and the fraction of HBM rate (HBM_GBS below: the MI355X's 8 TB/s) the best time works out to.  Kernel times of k_cert_ltv and of
the step's kernels: run the script under `rocprofv3 --kernel-trace --stats -- python tools/time_certificate_ltv.py` in a run of its
own (tracing slows the host clocks)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402
import almpc_loader  # noqa: E402
import mpc_oracle as mo  # noqa: E402

capi = almpc_loader.load_package()._capi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
HBM_GBS = 8000.0
COST_RES = capi.CERT_LTV["cost"] | capi.CERT_LTV["res"]
ALL = COST_RES | capi.CERT_LTV["grad"] | capi.CERT_LTV["costate"] | capi.CERT_LTV["x"]


def clock(call):
    call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def fmt(t):
    return f"{1e6 * t[0]:9.1f} us best, {1e6 * t[1]:9.1f} us median"


def bytes_moved(n, m, N, b, want):
    """what one launch reads and writes: the stage models and defects of every instance once per sweep it runs, xbar, e_u and u, and the
    outputs asked for (the shared operands are not counted)"""
    back = bool(want & 15)
    rd = b * 8 * ((1 + back) * N * n * (n + m) + N * n + (N + 1) * n + N * m * (1 + back))
    wr = b * 8 * (bool(want & 1) + bool(want & 2) + (N * m if want & 4 else 0) + ((N + 1) * n if want & 8 else 0) + (2 * (N + 1) * n if want & 16 else 0))
    return rd, wr


def ltv(n, m, N, b):
    rng = np.random.default_rng(100 * n + N)
    A_all = np.stack([[0.85 * np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n) for _ in range(N)] for _ in range(b)])
    B_all = rng.standard_normal((b, N, n, m))
    c_all = 0.05 * rng.standard_normal((b, N, n))
    xbar = rng.standard_normal((b, n, N + 1)); ubar = 0.2 * rng.standard_normal((b, m, N))
    x_ref = 0.2 * rng.standard_normal((n, N + 1)); u_ref = 0.1 * rng.standard_normal((m, N))
    Q, R, S, P = 10.0 * np.eye(n), 1.0 * np.eye(m), 0.3 * np.eye(m), 25.0 * np.eye(n) + 0.2 * np.ones((n, n))
    s = capi.Solver(n, m, N, b)
    s.design_ltv(A_all, B_all, c_all, xbar, ubar, x_ref, u_ref, Q, R, S, P, -0.5 * np.ones(m), 0.6 * np.ones(m), keep_stage_models=True)
    s.update_initialization(xbar[:, :, 0])
    s.calculate()
    st = s.get_results(want=("status",))["status"]
    print(f"LTV ({n}, {m}, {N}) x {b}: status {np.bincount(st, minlength=4).tolist()}; stage models {b * N * n * (n + m + 1) * 8 / 1e6:.1f} MB kept", flush=True)

    def step():
        s.calculate(sync=False)
        s.synchronize()
    print(f"    step                        {fmt(clock(step))}", flush=True)
    for name, want in (("certificate_ltv COST | RES ", COST_RES), ("certificate_ltv all six    ", ALL), ("certificate_ltv STATES     ", 16)):
        rd, wr = bytes_moved(n, m, N, b, want)
        t = clock(lambda: s._check(s.L.almpc_certificate_ltv(s.h, want)))
        print(f"    {name} {fmt(t)};  reads {rd / 1e6:.2f} MB, writes {wr / 1e6:.2f} MB: {100 * (rd + wr) / t[0] / 1e9 / HBM_GBS:.1f} % of HBM rate", flush=True)
    c = s.certificate_ltv()
    rel = c["res"] / np.maximum(1.0, np.abs(c["grad"]).max(axis=(1, 2)))
    print(f"    res / max(1, |g|_inf): median {np.median(rel):.2e}, max {rel.max():.2e}; cost median {np.median(c['cost']):.4g}", flush=True)
    s.close()


def relin():
    f = mo.synthetic_fnn(act="tanh")
    b, N, n, m = 1024, 20, 4, 2
    x_ref = np.array([0.2, -0.1, 0.05, 0.0])[:, None] * np.ones((n, N + 1))
    u_ref = np.array([0.1, -0.2])[:, None] * np.ones((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    P = capi.dare(*f.jacobian(x_ref[:, -1], u_ref[:, -1]), Q, R)
    X0 = x_ref[:, 0][None, :] + 0.5 * mo.splitmix_normal(0x5EED0004, 21, b, n)
    s = capi.Solver(n, m, N, b)
    s.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act="tanh")
    s.update_initialization(X0)
    s.relin_fnn_step(capi.default_opts())
    st = s.get_results(want=("status",))["status"]
    print(f"relin ({n}, {m}, {N}) x {b}: status {np.bincount(st, minlength=4).tolist()}", flush=True)
    print(f"    relin_fnn_step (cold)       {fmt(clock(lambda: s.relin_fnn_step(capi.default_opts())))}", flush=True)
    for name, want in (("relin_fnn_certificate COST | RES", 3), ("relin_fnn_certificate all four  ", 15)):
        print(f"    {name} {fmt(clock(lambda: s._check(s.L.almpc_relin_fnn_certificate(s.h, want))))}", flush=True)
    s.close()


ltv(4, 2, 50, 256)
ltv(12, 4, 30, 4096)
relin()
