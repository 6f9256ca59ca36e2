"""k_dare (csrc/almpc_dare.hip.h) and what it changes, on one GPU:
    design  almpc_design_batched(P = NULL) for 4096 perturbed quadrotor models (n 12, m 4, N 30), wall clock of the call, with the
            host DARE loop (almpc_set_terminal_weight 0, the default) and with k_dare (1)
    dare    almpc_dare_batched alone at 4096 instances, (n, m) = (4, 2), (12, 4), (48, 16): wall clock of the call (uploads, kernel,
            read-back) and the doublings the models need (host restatement of the same loop)
    relin   the configs[3]-shaped re-linearisation step (1024 instances, N 20, synthetic Fnn, tanh), cold and warm, mode off and on:
            host clock around `steps` asynchronous steps and one synchronise, and the stages of the last step (device events)
medians over `reps` repetitions after a warm-up.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/time_dare.py` for the
kernel's own time.  A library without almpc_set_terminal_weight (an older commit) gets the mode-off rows only.
    python tools/time_dare.py [reps=5] [steps=300] [parts=design,dare,relin]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import almpc_loader  # noqa: E402
import mpc_oracle as mo  # noqa: E402

capi = almpc_loader.load_package()._capi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 300
parts = sys.argv[3].split(",") if len(sys.argv) > 3 else ["design", "dare", "relin"]
HAS_MODE = hasattr(capi.Solver, "set_terminal_weight")
MODES = ("given", "dare_device") if HAS_MODE else ("given",)


def doublings(A, B, Q, R):
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


def design():
    p = mo.quadrotor()
    b, N = 4096, 30
    rng = np.random.default_rng(7)
    A = p.A[None] * (1.0 + 0.05 * rng.standard_normal((b, 12, 12)))
    B = p.B[None] * (1.0 + 0.05 * rng.standard_normal((b, 12, 4)))
    print("| design_batched(P = NULL), 4096 quadrotor-size models, N 30 | wall clock of the call (ms) |")
    print("|---|---|")
    for mode in MODES:
        s = capi.Solver(12, 4, N, b)
        if HAS_MODE:
            s.set_terminal_weight(mode)
        t = []
        for rep in range(max(2, reps // 2) + 1):
            t0 = time.perf_counter()
            s.design_batched(A, B, p.Q, p.R, None, None, p.u_min, p.u_max)
            t1 = time.perf_counter()
            if rep:
                t.append(t1 - t0)
        t0 = time.perf_counter()
        s.design_batched(A, B, p.Q, p.R, None, np.repeat(p.P[None], b, 0), p.u_min, p.u_max)   # the same design with every P given
        tg = time.perf_counter() - t0
        s.close()
        print(f"| terminal weight {mode} | {1e3 * np.median(t):.1f} (with P given: {1e3 * tg:.1f}) |", flush=True)


def dare():
    if not hasattr(capi, "dare_batched"):
        print("almpc_dare_batched: not in this library")
        return
    print("| almpc_dare_batched, 4096 instances | wall clock of the call (ms) | host almpc_dare, 64 of them (ms each) | doublings (min / median / max of 64) |")
    print("|---|---|---|---|")
    for n, m in ((4, 2), (12, 4), (48, 16)):
        b = 4096
        rng = np.random.default_rng(1000 + n)
        A = rng.standard_normal((b, n, n)) / np.sqrt(n) * rng.uniform(0.6, 1.3, (b, 1, 1))
        B = rng.standard_normal((b, n, m))
        Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
        t = []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            P, st = capi.dare_batched(A, B, Q, R)
            t1 = time.perf_counter()
            if rep:
                t.append(t1 - t0)
        t0 = time.perf_counter()
        for i in range(64):
            capi.dare(A[i], B[i], Q, R)
        th = (time.perf_counter() - t0) / 64
        d = [doublings(A[i], B[i], Q, R) for i in range(64)]
        print(f"| n {n}, m {m} ({int((st != 0).sum())} without a solution) | {1e3 * np.median(t):.2f} | {1e3 * th:.2f} | "
              f"{min(d)} / {int(np.median(d))} / {max(d)} |", flush=True)


def relin():
    f = mo.synthetic_fnn(act="tanh")
    batch, N, n, m = 1024, 20, 4, 2
    x_ref = np.array([0.2, -0.1, 0.05, 0.0])[:, None] * np.ones((n, N + 1))
    u_ref = np.array([0.1, -0.2])[:, None] * np.ones((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    P = capi.dare(*f.jacobian(x_ref[:, -1], u_ref[:, -1]), Q, R)
    X0 = x_ref[:, 0][None, :] + 0.5 * mo.splitmix_normal(0x5EED0004, 21, batch, n)
    print(f"| relin step, 1024 x N 20, synthetic Fnn (tanh) | us per step over {steps} steps (host clock, one synchronise) | "
          "jacobian / design / step of the last step (ms, device events) | own DARE / setup's P |")
    print("|---|---|---|---|")
    for mode in MODES:
        for warm in (0, 1):
            s = capi.Solver(n, m, N, batch, timing=True)
            if HAS_MODE:
                s.set_terminal_weight(mode)
            s.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, [-1, -1], [1, 1], act="tanh")
            s.update_initialization(X0)
            opts = capi.default_opts(warm_start=warm)
            s.relin_fnn_step(capi.default_opts())
            t = []
            for rep in range(reps + 1):
                t0 = time.perf_counter()
                for _ in range(steps):
                    s.relin_fnn_step(opts, sync=False)
                s.synchronize()
                t1 = time.perf_counter()
                if rep:
                    t.append((t1 - t0) / steps)
            st = s.relin_fnn_timing()
            own = ""
            if HAS_MODE and mode == "dare_device":
                ts = s.relin_terminal_status()
                own = f"{int((ts == 0).sum())} / {int((ts != 0).sum())}"
            r = s.get_results(want=("status",))
            s.close()
            print(f"| terminal weight {mode}, {'warm' if warm else 'cold'} ({int((r['status'] != 0).sum())} unsolved) | {1e6 * np.median(t):.1f} | "
                  f"{st['jacobian_ms']:.3f} / {st['design_ms']:.3f} / {st['step_ms']:.3f} | {own} |", flush=True)


for part in parts:
    {"design": design, "dare": dare, "relin": relin}[part]()
    print()
