"""k_c2d (csrc/almpc_c2d.hip.h) and what it changes, on one GPU:
    c2d     almpc_c2d_batched alone at 1024 x (4, 2), 4096 x (12, 4), 4096 x (48, 16), 256 x (64, 16): wall clock of the call (uploads,
            kernel, read-back), the squarings s the models need and the launch geometry (waves per workgroup, workgroups, LDS)
    design  almpc_design_batched for 4096 perturbed continuous quadrotors (n 12, m 4, N 30, P given): wall clock of the call with
            almpc_set_model_time on, against the route without it: 4096 host scipy.linalg.expm calls + the design on discrete models
    relin   the configs[3]-shaped re-linearisation step (1024 instances, N 20, synthetic Fnn, tanh), cold and warm, mode off and on:
            host clock around `steps` asynchronous steps and one synchronise, and the stages of the last step (device events)
medians over `reps` repetitions after a warm-up.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/time_c2d.py` for the
kernel's own time.  A library without almpc_set_model_time (an older commit) gets the mode-off rows only.
    python tools/time_c2d.py [reps=5] [steps=300] [parts=c2d,design,relin]"""
import os
import sys
import time

import numpy as np
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import almpc_loader  # noqa: E402
import mpc_oracle as mo  # noqa: E402

capi = almpc_loader.load_package()._capi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 300
parts = sys.argv[3].split(",") if len(sys.argv) > 3 else ["c2d", "design", "relin"]
HAS_MODE = hasattr(capi.Solver, "set_model_time")
MODES = ("discrete", "continuous") if HAS_MODE else ("discrete",)
TS_RELIN = 0.25


def squarings(A, Ts):
    nrm, s = Ts * np.abs(A).sum(axis=0).max(), 0
    while nrm > 0.5:
        nrm *= 0.5
        s += 1
    return s


def geometry(n, m, batch):
    """hm / k_c2d's own arithmetic: LDS doubles per wave, waves per workgroup (at most 4, while they fit 160 KB), workgroups."""
    per_wave = 8 * ((3 * (n | 1) * (n + m) + 1) & ~1)
    waves = 4
    while waves > 1 and per_wave * waves > 160 * 1024:
        waves -= 1
    return waves, (batch + waves - 1) // waves, per_wave * waves


def zoh(A, B, Ts):
    n, m = B.shape
    M = np.zeros((n + m, n + m))
    M[:n, :n], M[:n, n:] = A, B
    E = sla.expm(M * Ts)
    return E[:n, :n], E[:n, n:]


def quadrotor_continuous():
    Ac, Bc = np.zeros((12, 12)), np.zeros((12, 4))
    Ac[0:3, 3:6] = np.eye(3); Ac[3, 7] = 9.81; Ac[4, 6] = -9.81; Ac[6:9, 9:12] = np.eye(3)
    Bc[5, 0] = 2.0; Bc[9, 1] = 250.0; Bc[10, 2] = 250.0; Bc[11, 3] = 125.0
    return Ac, Bc


def c2d():
    if not hasattr(capi, "c2d_batched"):
        print("almpc_c2d_batched: not in this library")
        return
    print("| almpc_c2d_batched | Ts | s (min / median / max) | waves per workgroup x workgroups, LDS per workgroup | wall clock of the call (ms) | host almpc_c2d, 64 of them (ms each) |")
    print("|---|---|---|---|---|---|")
    for batch, n, m in ((1024, 4, 2), (4096, 12, 4), (4096, 48, 16), (256, 64, 16)):
        rng = np.random.default_rng(2000 + n)
        A = rng.standard_normal((batch, n, n)) / np.sqrt(n) * rng.uniform(0.3, 3.0, (batch, 1, 1)) - rng.uniform(0.0, 2.0, (batch, 1, 1)) * np.eye(n)
        B = rng.standard_normal((batch, n, m))
        Ts = 1.0
        t = []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            Ad, Bd, st = capi.c2d_batched(A, B, Ts)
            t1 = time.perf_counter()
            if rep:
                t.append(t1 - t0)
        t0 = time.perf_counter()
        for i in range(64):
            capi.c2d(A[i], B[i], Ts)
        th = (time.perf_counter() - t0) / 64
        s = [squarings(A[i], Ts) for i in range(batch)]
        w, g, lds = geometry(n, m, batch)
        print(f"| {batch} x ({n}, {m}) ({int((st != 0).sum())} failed) | {Ts} | {min(s)} / {int(np.median(s))} / {max(s)} | {w} x {g}, {lds / 1024:.1f} KB | "
              f"{1e3 * np.median(t):.2f} | {1e3 * th:.3f} |", flush=True)


def design():
    p = mo.quadrotor()
    b, N = 4096, 30
    Ac, Bc = quadrotor_continuous()
    rng = np.random.default_rng(7)
    A = Ac[None] * (1.0 + rng.uniform(-0.05, 0.05, (b, 12, 12)))
    B = Bc[None] * (1.0 + rng.uniform(-0.05, 0.05, (b, 12, 4)))
    P = np.repeat(p.P[None], b, 0)
    print("| design_batched, 4096 continuous quadrotors, N 30, P given | wall clock (ms) |")
    print("|---|---|")
    t0 = time.perf_counter()
    D = [zoh(A[i], B[i], 0.1) for i in range(b)]
    t_expm = time.perf_counter() - t0
    Ad, Bd = np.stack([d[0] for d in D]), np.stack([d[1] for d in D])
    for mode in MODES:
        s = capi.Solver(12, 4, N, b)
        if HAS_MODE:
            s.set_model_time(mode, 0.1)
        t = []
        for rep in range(max(2, reps // 2) + 1):
            t0 = time.perf_counter()
            if mode == "continuous":
                s.design_batched(A, B, p.Q, p.R, None, P, p.u_min, p.u_max)
            else:
                s.design_batched(Ad, Bd, p.Q, p.R, None, P, p.u_min, p.u_max)
            t1 = time.perf_counter()
            if rep:
                t.append(t1 - t0)
        s.close()
        if mode == "continuous":
            print(f"| model time continuous: the call | {1e3 * np.median(t):.1f} |", flush=True)
        else:
            print(f"| model time discrete: 4096 host scipy.linalg.expm + the call | {1e3 * t_expm:.1f} + {1e3 * np.median(t):.1f} |", flush=True)


def relin():
    f = mo.synthetic_fnn(act="tanh")
    batch, N, n, m = 1024, 20, 4, 2
    x_ref = np.array([0.2, -0.1, 0.05, 0.0])[:, None] * np.ones((n, N + 1))
    u_ref = np.array([0.1, -0.2])[:, None] * np.ones((m, N))
    Q, R = 100.0 * np.eye(n), 0.1 * np.eye(m)
    X0 = x_ref[:, 0][None, :] + 0.5 * mo.splitmix_normal(0x5EED0004, 21, batch, n)
    print(f"| relin step, 1024 x N 20, synthetic Fnn (tanh) | us per step over {steps} steps (host clock, one synchronise) | "
          "jacobian / design / step of the last step (ms, device events) |")
    print("|---|---|---|")
    for mode in MODES:
        Al, Bl = f.jacobian(x_ref[:, -1], u_ref[:, -1])
        if mode == "continuous":
            Al, Bl = zoh(Al, Bl, TS_RELIN)
        P = capi.dare(Al, Bl, Q, R)
        for warm in (0, 1):
            s = capi.Solver(n, m, N, batch, timing=True)
            if HAS_MODE:
                s.set_model_time(mode, TS_RELIN)
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
            r = s.get_results(want=("status",))
            s.close()
            print(f"| model time {mode}, {'warm' if warm else 'cold'} ({int((r['status'] != 0).sum())} unsolved) | {1e6 * np.median(t):.1f} "
                  f"(min {1e6 * min(t):.1f}, max {1e6 * max(t):.1f}) | {st['jacobian_ms']:.3f} / {st['design_ms']:.3f} / {st['step_ms']:.3f} |", flush=True)


for part in parts:
    {"c2d": c2d, "design": design, "relin": relin}[part]()
    print()
