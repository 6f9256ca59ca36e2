"""Cold-start tolerance solve (almpc_sqp_fnn_solve) at the benchmark shape (256 instances, Fnn 4-2-16x2 tanh, N 50, merit rule),
against the fixed-count loop, with the Gauss-Newton and with the exact Hessian: iterations to convergence p50 / p99 / max, ms per
iteration, ms per solve.
    python tools/time_sqp_solve.py [max_iters=40] [tol=1e-6] [reps=5]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import almpc_loader  # noqa: E402
import sqp_solve_ref as ref  # noqa: E402

capi = almpc_loader.load_package()._capi
max_iters = int(sys.argv[1]) if len(sys.argv) > 1 else 40
tol = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-6
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
f, kw, X0 = ref.bench_setup()
b, N = X0.shape[0], kw["u_ref"].shape[1]
s = capi.Solver(4, 2, N, b)
s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"],
                act="tanh")
for mode in ("gauss_newton", "exact"):
    s.sqp_fnn_set_hessian(mode)
    t_fix, t_solve = [], []
    for rep in range(reps + 1):   # (the first repetition warms up)
        s.sqp_fnn_start(X0)
        t0 = time.perf_counter()
        s.sqp_fnn_iterate(max_iters, step_rule="merit")
        t1 = time.perf_counter()
        s.sqp_fnn_start(X0)
        t2 = time.perf_counter()
        out = s.sqp_fnn_solve(max_iters, tol)
        t3 = time.perf_counter()
        if rep:
            t_fix.append(t1 - t0); t_solve.append(t3 - t2)
    st, it = out["status"], out["iters"]
    conv = it[st == 0]
    print(f"[{mode}] batch {b}, N {N}, max_iters {max_iters}, tol {tol:g}")
    print(f"  converged {int((st == 0).sum())} / {b}; status counts {np.bincount(st, minlength=4).tolist()}; unconverged {np.nonzero(st)[0].tolist()}")
    if conv.size:
        print(f"  iterations of the converged: p50 {np.percentile(conv, 50):.0f}  p99 {np.percentile(conv, 99):.1f}  max {conv.max()}")
    print(f"  fixed-count loop: {1e3 * np.median(t_fix) / max_iters:.3f} ms per iteration ({1e3 * np.median(t_fix):.2f} ms for {max_iters})")
    print(f"  tolerance solve: {1e3 * np.median(t_solve):.2f} ms per solve (iterations run: {it.max()})")
s.close()
