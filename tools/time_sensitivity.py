"""k_sens (csrc/almpc_sens.hip.h) at the benchmark batch, on one GPU: 4096 quadrotors (n 12, m 4, N 30), the three amplitude classes of
bench.py interleaved, the benchmark's operating point (stiffness profile rho 45, 6 ADMM iterations, cold start).  Prints the table of
DESIGN.md section 4 ("Sensitivities"):
    step        almpc_calculate (synchronous), for scale
    K0 / K0+dU / K0+dU+dX   almpc_sensitivity alone: host clock around the synchronous call (it ends in a device synchronise; no
                read-back), and the same through Solver.sensitivity, which also copies the arrays to the host
    VJP         almpc_sensitivity_vjp with and without g_x: host pointers, so the call includes the upload of the loss gradients and
                the read-back of g_x0
    params      almpc_sensitivity_params_vjp beside it (Solver.sensitivity_params_vjp: the same upload, the read-back of the wanted
                groups): the groups of the first kernel alone, every group, and every group through the C call into host arrays
                that stay
    rows form   the same batch with a tight state box (+-3 (1, 1, 1, .5, .5, .5, .1, ..., .1), x0 clipped to 0.99 of it) and the terminal
                equality, the library's default step: almpc_sensitivity_rows (K0; K0 + dU + dX) and almpc_sensitivity_rows_vjp
medians over `reps` repetitions after a warm-up, with minimum and maximum.  There is no threshold: nothing exists to compare against.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/time_sensitivity.py` for the kernels' own times.
    python tools/time_sensitivity.py [reps=20] [batch=4096]"""
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
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
AMPLITUDES = (0.3, 1.0, 3.0)   # bench.py


def clock(fn):
    t = []
    for rep in range(reps + 2):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if rep >= 2:
            t.append(t1 - t0)
    return f"{1e6 * np.median(t):.0f} (min {1e6 * min(t):.0f}, max {1e6 * max(t):.0f})"


p = mo.quadrotor()
X0 = wl.splitmix_normal(0x5EED0002, 0, batch, p.n) * wl.QUADROTOR_X0_SCALE[None, :] * np.array(AMPLITUDES)[np.arange(batch) % 3][:, None]
s = capi.Solver(p.n, p.m, p.N, batch)
s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=45.0, rho_profile="stiffness")
s.set_reference(p.x_ref, p.u_ref)
s.update_initialization(X0)
opts = capi.default_opts(rho=45.0, max_iter=6, check_every=6, keep_warm_state=False)
t_step = clock(lambda: s.calculate(opts))
st = s.get_results(want=("status",))["status"]
rows = s.sensitivity(("K0",))["rows"]
print(f"{batch} quadrotors, N {p.N}: {int((st != 0).sum())} unsolved; rows at a bound min {rows.min()} / median {int(np.median(rows))} / max {rows.max()}, "
      f"{int((rows > 32).sum())} instances beyond the first tier's 32 rows")
print()
print("| call | us per call of the whole batch: median (min, max) | with the read-back to host arrays |")
print("|---|---|---|")
print(f"| `almpc_calculate` (the step, for scale) | {t_step} | |")
for want in (("K0",), ("K0", "dU"), ("K0", "dU", "dX")):
    mask = capi._sens_mask(want)
    bare = clock(lambda: s._check(s.L.almpc_sensitivity(s.h, mask, 0.0)))
    full = clock(lambda: s.sensitivity(want))
    print(f"| `almpc_sensitivity`, {' + '.join(want)} | {bare} | {full} |", flush=True)
rng = np.random.default_rng(1)
g_u, g_x = rng.normal(size=(batch, p.m, p.N)), rng.normal(size=(batch, p.n, p.N + 1))
print(f"| `almpc_sensitivity_vjp`, g_u only | | {clock(lambda: s.sensitivity_vjp(g_u))} |")
print(f"| `almpc_sensitivity_vjp`, g_u and g_x | | {clock(lambda: s.sensitivity_vjp(g_u, g_x))} |")
# the parameter gradients: the same upload, k_sens_pz in place of k_sens<VJP>, k_sens_params behind it where a group needs it
print(f"| `almpc_sensitivity_params_vjp`, x0, f, u_min, u_max (no second kernel) | | "
      f"{clock(lambda: s.sensitivity_params_vjp(g_u, g_x, want=('x0', 'f', 'u_min', 'u_max')))} |")
print(f"| `almpc_sensitivity_params_vjp`, every group (fresh host arrays per call) | | {clock(lambda: s.sensitivity_params_vjp(g_u, g_x))} |")
# ... and the C call alone into host arrays that stay (what a training loop does): the wrapper's fresh arrays are first touched by the
# read-back, which can cost more than the call
gu_c, gx_c = np.ascontiguousarray(g_u.transpose(0, 2, 1)), np.ascontiguousarray(g_x.transpose(0, 2, 1))
per = {"x0": p.n, "f": p.nz, "u_ref": p.nz, "u_min": p.m, "u_max": p.m, "Q": p.n * p.n, "P": p.n * p.n, "A": p.n * p.n, "R": p.m * p.m,
       "S": p.m * p.m, "B": p.n * p.m}
kept = {k: np.zeros((batch, v)) for k, v in per.items()}
kept_rows = np.zeros(batch, dtype=np.int32)
out = capi.almpc_param_grads(**{k: capi._ptr(v) for k, v in kept.items()}, rows=kept_rows.ctypes.data_as(capi._ip))
t_kept = clock(lambda: s._check(s.L.almpc_sensitivity_params_vjp(s.h, capi._ptr(gu_c), capi._ptr(gx_c), 0.0, out)))
print(f"| `almpc_sensitivity_params_vjp`, every group, host arrays kept by the caller | | {t_kept} |", flush=True)
s.close()

# the state-row leg
XBOX = 3.0 * np.array([1, 1, 1, .5, .5, .5, .1, .1, .1, .1, .1, .1])
s = capi.Solver(p.n, p.m, p.N, batch)
s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, xmin=-XBOX, xmax=XBOX, terminal="equality")
s.set_reference(p.x_ref, p.u_ref)
s.update_initialization(np.clip(X0, -0.99 * XBOX, 0.99 * XBOX))
t_step = clock(lambda: s.calculate())
st = s.get_results(want=("status",))["status"]
rows = s.sensitivity_rows(("K0",))["rows"]
ok = rows[rows >= 0]
print()
print(f"state box and terminal equality: {int((st != 0).sum())} of {batch} not solved (infeasible); rows min {ok.min()} / median {int(np.median(ok))} / "
      f"max {ok.max()}, {int((ok - p.n > 32).sum())} instances beyond the first tier (the {p.n} equality rows are projected out)")
print()
print("| call | us per call of the whole batch: median (min, max) | with the read-back to host arrays |")
print("|---|---|---|")
print(f"| `almpc_calculate` (state rows, default options; for scale) | {t_step} | |")
for want in (("K0",), ("K0", "dU", "dX")):
    mask = capi._sens_mask(want)
    bare = clock(lambda: s._check(s.L.almpc_sensitivity_rows(s.h, mask, 0.0, 0.0)))
    full = clock(lambda: s.sensitivity_rows(want))
    print(f"| `almpc_sensitivity_rows`, {' + '.join(want)} | {bare} | {full} |", flush=True)
print(f"| `almpc_sensitivity_rows_vjp`, g_u and g_x | | {clock(lambda: s.sensitivity_rows_vjp(g_u, g_x))} |")
s.close()
