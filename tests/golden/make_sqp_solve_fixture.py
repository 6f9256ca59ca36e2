"""Writes fnn_sqp_solve_gn.json and fnn_sqp_solve_exact.json: the per-instance outcome of the restatements tests/sqp_solve_ref.py::
sqp_solve (Gauss-Newton, at most 40 iterations) and tests/sqp_exact_ref.py::sqp_solve_exact (exact Hessian, at most 30) on the
benchmark batch (256 instances, Fnn 4-2-16x2 tanh, N 50; merit rule, tol 1e-6): status (0 converged, 1 iteration limit), QP
iterations taken, residual of the last test (exact: also the Gauss-Newton fallbacks).  Run from the repository root:
    python tests/golden/make_sqp_solve_fixture.py [processes]"""
import json
import os
import sys
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")]
import sqp_exact_ref as ex  # noqa: E402
import sqp_solve_ref as ref  # noqa: E402

MAX_ITERS, MAX_ITERS_EXACT, TOL = 40, 30, 1e-6
f, kw, X0 = ref.bench_setup()
ARGS = (kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"])


def one(i):
    r = ref.sqp_solve(f, X0[i], *ARGS, MAX_ITERS, TOL)
    return int(r["status"]), int(r["iters"]), float(r["kkt"])


def one_exact(i):
    r = ex.sqp_solve_exact(f, X0[i], *ARGS, MAX_ITERS_EXACT, TOL)
    return int(r["status"]), int(r["iters"]), float(r["kkt"]), int(r["gn_fallbacks"])


if __name__ == "__main__":
    with Pool(int(sys.argv[1]) if len(sys.argv) > 1 else 4) as p:
        res = p.map(one, range(X0.shape[0]))
        rex = p.map(one_exact, range(X0.shape[0]))
    out = dict(max_iters=MAX_ITERS, tol=TOL, status=[r[0] for r in res], iters=[r[1] for r in res], kkt=[r[2] for r in res])
    with open(os.path.join(HERE, "fnn_sqp_solve_gn.json"), "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")
    out = dict(max_iters=MAX_ITERS_EXACT, tol=TOL, status=[r[0] for r in rex], iters=[r[1] for r in rex], kkt=[r[2] for r in rex],
               gn_fallbacks=[r[3] for r in rex])
    with open(os.path.join(HERE, "fnn_sqp_solve_exact.json"), "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")
