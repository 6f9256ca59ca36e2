"""Fnn against ResNet, PolyNet and DenseNet at the same shape (4-2-16x2 tanh, weights of the synthetic Fnn, tests/net_ref.py::synthetic_net;
the DenseNet's from tests/densenet_ref.py::synthetic_densenet, its hidden layers 16 x 16 and 16 x 32):
    relin   one cold almpc_relin_fnn_step at the configs[3] shape (1024 instances, N 20): wall time and its three stages
    gn      one Gauss-Newton SQP iteration at the benchmark shape (256 instances, N 50, fixed step)
    exact   one exact-Hessian SQP iteration at the same shape
medians over `reps` repetitions after one warm-up.
    python tools/time_net_models.py [reps=20] [kinds=fnn,resnet,polynet,densenet]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import almpc_loader  # noqa: E402
import densenet_ref as dn  # noqa: E402
import mpc_oracle as mo  # noqa: E402
import net_ref  # noqa: E402
import sqp_solve_ref as sref  # noqa: E402

capi = almpc_loader.load_package()._capi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ITERS = 10


def model(kind):
    return dn.synthetic_densenet(act="tanh") if kind == "densenet" else net_ref.synthetic_net(kind, act="tanh")


def relin(kind):
    f = model(kind)
    batch, N, n, m = 1024, 20, 4, 2
    x_ref = np.array([0.2, -0.1, 0.05, 0.0])[:, None] * np.ones((n, N + 1))
    u_ref = np.array([0.1, -0.2])[:, None] * np.ones((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    P = capi.dare(*f.jacobian(x_ref[:, -1], u_ref[:, -1]), Q, R)
    X0 = x_ref[:, 0][None, :] + 0.5 * mo.splitmix_normal(0x5EED0004, 21, batch, n)
    s = capi.Solver(n, m, N, batch, timing=True)
    if kind == "densenet":
        s.relin_densenet_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act="tanh")
    else:
        s.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act="tanh", net=kind)
    s.update_initialization(X0)
    opts = capi.default_opts()
    wall, st = [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        s.relin_fnn_step(opts)
        t1 = time.perf_counter()
        if rep:
            wall.append(t1 - t0); st.append(list(s.relin_fnn_timing().values()))
    s.close()
    st = np.median(np.array(st), axis=0)
    return 1e3 * np.median(wall), st


def sqp(kind, mode):
    _, kw, X0 = sref.bench_setup()
    f = model(kind)
    b, N = X0.shape[0], kw["u_ref"].shape[1]
    s = capi.Solver(4, 2, N, b)
    args = (f.W_in, f.W_h, f.b_h, f.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"])
    if kind == "densenet":
        s.sqp_densenet_setup(*args, act="tanh")
    else:
        s.sqp_fnn_setup(*args, act="tanh", net=kind)
    s.sqp_fnn_set_hessian(mode)
    t = []
    for rep in range(max(3, reps // 4) + 1):
        s.sqp_fnn_start(X0)
        t0 = time.perf_counter()
        try:
            s.sqp_fnn_iterate(ITERS)
        except capi.AlmpcError:   # (an instance skipped an iteration: timing is still what it is)
            pass
        t1 = time.perf_counter()
        if rep:
            t.append(t1 - t0)
    s.close()
    return 1e3 * np.median(t) / ITERS


print("| model | relin step, 1024 x N 20 (ms) | jacobian / design / step (ms) | SQP GN iteration, 256 x N 50 (ms) | SQP exact iteration (ms) |")
print("|---|---|---|---|---|")
for kind in (sys.argv[2].split(",") if len(sys.argv) > 2 else ("fnn", "resnet", "polynet", "densenet")):
    w, st = relin(kind)
    print(f"| {kind} | {w:.3f} | {st[0]:.3f} / {st[1]:.3f} / {st[2]:.3f} | {sqp(kind, 'gauss_newton'):.3f} | {sqp(kind, 'exact'):.3f} |",
          flush=True)
