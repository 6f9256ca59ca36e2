"""k_dare_vjp (csrc/almpc_dare_vjp.hip.h) beside k_dare, on one GPU:
    batched  almpc_dare_vjp_batched beside almpc_dare_batched on the same models, (n, m) x batch = (4, 2) x 1024, (12, 4) x 4096,
             (48, 16) x 4096: wall clock of the C call into arrays the caller keeps (uploads, kernel, read-back), and the doublings
             the adjoint's Lyapunov loop and the DARE need (host restatements of the two loops, 64 of the models)
    handle   almpc_sensitivity_params_vjp_dare beside almpc_sensitivity_params_vjp on the 4096-instance quadrotor batch of
             tools/time_sensitivity.py (every group, host arrays kept by the caller)
medians over `reps` repetitions after a warm-up, with minimum and maximum.  Nothing is promised: the adjoint does one m x m LU and a
handful of doublings of three products each, k_dare an n x n LU per doubling, so the supposition is that it costs less.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/time_dare_vjp.py` for the kernels' own times.
    python tools/time_dare_vjp.py [reps=10] [parts=batched,handle]"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import almpc_loader  # noqa: E402
import mpc_oracle as mo  # noqa: E402

pkg = almpc_loader.load_package()
capi = pkg._capi
wl = importlib.import_module(pkg.__name__ + ".workloads")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
parts = sys.argv[2].split(",") if len(sys.argv) > 2 else ["batched", "handle"]


def clock(fn, scale=1e3, fmt=".2f"):
    t = []
    for rep in range(reps + 2):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if rep >= 2:
            t.append(t1 - t0)
    return f"{scale * np.median(t):{fmt}} (min {scale * min(t):{fmt}}, max {scale * max(t):{fmt}})"


def dare_doublings(A, B, Q, R):
    """Doublings hm::dare / k_dare need for one model (the same loop and stopping test in numpy)."""
    G, H, Ak = B @ np.linalg.solve(R, B.T), Q.copy(), A.copy()
    for it in range(1, 201):
        W = np.eye(A.shape[0]) + G @ H
        WA, WG = np.linalg.solve(W, Ak), np.linalg.solve(W, G)
        G1, H1, Ak = G + Ak @ WG @ Ak.T, H + Ak.T @ H @ WA, Ak @ WA
        G1, H1 = 0.5 * (G1 + G1.T), 0.5 * (H1 + H1.T)
        done = np.abs(H1 - H).max() <= 1e-13 * max(1.0, np.abs(H1).max())
        G, H = G1, H1
        if done:
            return it
    return 200


def vjp_doublings(A, B, R, P, gP):
    """Doublings hm::dare_vjp / k_dare_vjp need (the same loop and stopping test in numpy)."""
    Aj = A - B @ np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A)
    X = gP.copy()
    for it in range(1, 65):
        D = Aj @ X @ Aj.T
        X = 0.5 * ((X + D) + (X + D).T)
        Aj = Aj @ Aj
        if np.abs(D).max() <= 1e-13 * max(1.0, np.abs(X).max()):
            return it
    return 64


def batched():
    print("| shape x batch | `almpc_dare_batched`, ms per call: median (min, max) | `almpc_dare_vjp_batched`, ms per call | "
          "doublings of the DARE (min / median / max of 64) | doublings of the adjoint |")
    print("|---|---|---|---|---|")
    for n, m, b in ((4, 2, 1024), (12, 4, 4096), (48, 16, 4096)):
        rng = np.random.default_rng(1000 + n)
        A = rng.standard_normal((b, n, n)) / np.sqrt(n) * rng.uniform(0.6, 1.3, (b, 1, 1))
        B = rng.standard_normal((b, n, m))
        Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
        gP = rng.standard_normal((b, n, n))
        gP = 0.5 * (gP + gP.transpose(0, 2, 1))
        P, st = capi.dare_batched(A, B, Q, R)
        P[st != 0] = np.eye(n)   # (refused by the adjoint as well: status 3)
        # the C calls alone on column-major arrays the caller keeps (the wrappers' transposes and fresh arrays cost more than the calls)
        cm = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))
        Ac, Bc, Pc, gPc, Qc, Rc = cm(A), cm(B), cm(P), cm(gP), np.asfortranarray(Q), np.asfortranarray(R)
        Po, gA, gB, gQ, gR = np.zeros((b, n, n)), np.zeros((b, n, n)), np.zeros((b, m, n)), np.zeros((b, n, n)), np.zeros((b, m, m))
        so, sv = np.zeros(b, dtype=np.int32), np.zeros(b, dtype=np.int32)
        ptr, ip = capi._ptr, lambda a: a.ctypes.data_as(capi._ip)
        L = capi.load()
        t_dare = clock(lambda: L.almpc_dare_batched(0, n, m, b, ptr(Ac), ptr(Bc), ptr(Qc), ptr(Rc), ptr(Po), ip(so)))
        t_vjp = clock(lambda: L.almpc_dare_vjp_batched(0, n, m, b, ptr(Ac), ptr(Bc), ptr(Qc), ptr(Rc), ptr(Pc), ptr(gPc), ptr(gA), ptr(gB),
                                                        ptr(gQ), ptr(gR), ip(sv)))
        ok = [i for i in range(b) if st[i] == 0 and sv[i] == 0][:64]
        d1 = [dare_doublings(A[i], B[i], Q, R) for i in ok]
        d2 = [vjp_doublings(A[i], B[i], R, P[i], gP[i]) for i in ok]
        print(f"| n {n}, m {m} x {b} ({int((st != 0).sum())} without a solution, {int((sv != 0).sum())} refused by the adjoint) | {t_dare} | "
              f"{t_vjp} | {min(d1)} / {int(np.median(d1))} / {max(d1)} | {min(d2)} / {int(np.median(d2))} / {max(d2)} |", flush=True)


def handle(batch=4096):
    p = mo.quadrotor()
    amplitudes = np.array((0.3, 1.0, 3.0))   # bench.py
    X0 = wl.splitmix_normal(0x5EED0002, 0, batch, p.n) * wl.QUADROTOR_X0_SCALE[None, :] * amplitudes[np.arange(batch) % 3][:, None]
    s = capi.Solver(p.n, p.m, p.N, batch)
    s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=45.0, rho_profile="stiffness")
    s.set_reference(p.x_ref, p.u_ref)
    s.update_initialization(X0)
    s.calculate(capi.default_opts(rho=45.0, max_iter=6, check_every=6, keep_warm_state=False))
    rng = np.random.default_rng(1)
    gu_c = np.ascontiguousarray(rng.normal(size=(batch, p.m, p.N)).transpose(0, 2, 1))
    gx_c = np.ascontiguousarray(rng.normal(size=(batch, p.n, p.N + 1)).transpose(0, 2, 1))
    per = {"x0": p.n, "f": p.nz, "u_ref": p.nz, "u_min": p.m, "u_max": p.m, "Q": p.n * p.n, "P": p.n * p.n, "A": p.n * p.n, "R": p.m * p.m,
           "S": p.m * p.m, "B": p.n * p.m}
    kept = {k: np.zeros((batch, v)) for k, v in per.items()}
    rows, dst = np.zeros(batch, dtype=np.int32), np.zeros(batch, dtype=np.int32)
    out = capi.almpc_param_grads(**{k: capi._ptr(v) for k, v in kept.items()}, rows=rows.ctypes.data_as(capi._ip))
    print(f"| {batch} quadrotors, N {p.N}, every group, host arrays kept by the caller | us per call: median (min, max) |")
    print("|---|---|")
    t = clock(lambda: s._check(s.L.almpc_sensitivity_params_vjp(s.h, capi._ptr(gu_c), capi._ptr(gx_c), 0.0, out)), 1e6, ".0f")
    print(f"| `almpc_sensitivity_params_vjp` | {t} |")
    t = clock(lambda: s._check(s.L.almpc_sensitivity_params_vjp_dare(s.h, capi._ptr(gu_c), capi._ptr(gx_c), 0.0, out, dst.ctypes.data_as(capi._ip))),
              1e6, ".0f")
    print(f"| `almpc_sensitivity_params_vjp_dare` ({int((dst != 0).sum())} instances not followed, {int((rows < 0).sum())} unsolved) | {t} |", flush=True)
    s.close()


for part in parts:
    {"batched": batched, "handle": handle}[part]()
    print()
