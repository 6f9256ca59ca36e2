"""State-row multipliers of the Fnn SQP loop (almpc_sqp_fnn_set_row_multipliers) at 256 instances: the state-box problem of
tests/test_gpu_sqp.py::test_sqp_with_state_box (Fnn 4-2-16x2 tanh, N 20, same box, the seeds continued), cold start.
  - the fixed-count Gauss-Newton loop with the switch off and on (ms per iteration, ms per loop; the overhead of the switch),
  - the tolerance solve with the switch on, Gauss-Newton and exact Hessian: verdicts, iterations p50 / p99 / max, ms per solve.
    python tools/time_sqp_rows.py [iters=25] [max_iters=40] [tol=1e-6] [reps=7]
Kernel times of k_sqp_kkt, k_polish_gen*, k_sdual: run the script under `rocprofv3 --kernel-trace --stats -- python tools/time_sqp_rows.py`."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import almpc_loader  # noqa: E402
import sqp_rows_ref as rr  # noqa: E402

capi = almpc_loader.load_package()._capi
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 25
max_iters = int(sys.argv[2]) if len(sys.argv) > 2 else 40
tol = float(sys.argv[3]) if len(sys.argv) > 3 else 1e-6
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
b, N = 256, 20
f, kw, xlo, xhi, X0 = rr.state_box_fixture(b=b)
s = capi.Solver(4, 2, N, b)
s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"],
                act="tanh", xmin=xlo, xmax=xhi)


def fixed(on):
    """one cold fixed-count loop; infeasible instances are named by ALMPC_ERR_NUMERIC after the others have finished"""
    s.sqp_fnn_set_row_multipliers(on)
    s.sqp_fnn_start(X0)
    t0 = time.perf_counter()
    try:
        s.sqp_fnn_iterate(iters, step_rule="merit")
    except capi.AlmpcError as e:
        if e.code != -6:
            raise
    return time.perf_counter() - t0


# the two settings alternate within one run, so that drift of the clocks hits both alike
t = {False: [], True: []}
for rep in range(reps + 1):   # (the first repetition warms up)
    for on in (False, True):
        dt = fixed(on)
        if rep:
            t[on].append(dt)
off, on = np.median(t[False]), np.median(t[True])
skipped = int(np.count_nonzero(s.sqp_fnn_skipped()))
print(f"[gauss_newton, fixed count] batch {b}, N {N}, {iters} iterations, {skipped} instances with an infeasible QP")
print(f"  switch off: {1e3 * off / iters:.4f} ms per iteration ({1e3 * off:.2f} ms per loop; min {1e3 * min(t[False]):.2f} max {1e3 * max(t[False]):.2f})")
print(f"  switch on : {1e3 * on / iters:.4f} ms per iteration ({1e3 * on:.2f} ms per loop; min {1e3 * min(t[True]):.2f} max {1e3 * max(t[True]):.2f})")
print(f"  overhead of the switch: {100.0 * (on / off - 1.0):+.2f} %")
s.sqp_fnn_set_row_multipliers(True)
for mode in ("gauss_newton", "exact"):
    s.sqp_fnn_set_hessian(mode)
    ts = []
    for rep in range(reps + 1):
        s.sqp_fnn_start(X0)
        t0 = time.perf_counter()
        out = s.sqp_fnn_solve(max_iters, tol)
        if rep:
            ts.append(time.perf_counter() - t0)
    st, it = out["status"], out["iters"]
    conv = it[st == 0]
    print(f"[{mode}, tolerance solve, switch on] max_iters {max_iters}, tol {tol:g}")
    print(f"  status counts (converged, limit, skipped, infeasible) {np.bincount(st, minlength=4).tolist()}")
    if conv.size:
        print(f"  iterations of the converged: p50 {np.percentile(conv, 50):.0f}  p99 {np.percentile(conv, 99):.1f}  max {conv.max()}")
    print(f"  {1e3 * np.median(ts):.2f} ms per solve (min {1e3 * min(ts):.2f} max {1e3 * max(ts):.2f})")
s.close()
if on > 1.10 * off:   # the one bound of this measurement: the kernel trace says where the time goes
    sys.exit("the switch costs more than 10 % of a fixed-count Gauss-Newton iteration")
