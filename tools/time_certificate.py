"""Time the certificate of a step (almpc_certificate, k_cert) beside the step of the same handle, in one run: the headline batch
(quadrotor N = 30, 4096 instances, condensed handle) and the structured N = 50 batch (the batch of tools/time_sens_face.py).
    python tools/time_certificate.py [reps=50]
Per handle: the step, almpc_certificate with COST | RES, almpc_certificate with all four bits -- each a host clock around a call that
ends in a wait for the handle's stream (best and median after a warm-up call; the results stay on the device), and the bytes one
launch moves, computed from the shapes.  Kernel times of k_cert and of the step's kernels: run the script under
`rocprofv3 --kernel-trace --stats -- python tools/time_certificate.py` in a run of its own (tracing slows the host clocks)."""
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
b = 4096
X0 = np.concatenate([mo.quadrotor_x0_batch(b // 4 if a != 1.0 else b // 2, a, first_instance=k * b) for k, a in enumerate((0.3, 1.0, 3.0))])[:b]
COST_RES = capi.CERT["cost"] | capi.CERT["res"]
ALL = COST_RES | capi.CERT["grad"] | capi.CERT["costate"]


def clock(call):
    call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return f"{1e6 * min(ts):9.1f} us best, {1e6 * float(np.median(ts)):9.1f} us median"


def step(s):
    s.calculate(sync=False)
    s.synchronize()


def bytes_moved(n, m, N, want):
    """what one launch reads and writes: the trajectories of every instance, the shared operands once per wave at most (not counted),
    and the outputs asked for"""
    rd = b * ((N + 1) * n + 2 * N * m) * 8
    wr = b * 8 * (bool(want & 1) + bool(want & 2) + (N * m if want & 4 else 0) + ((N + 1) * n if want & 8 else 0))
    return rd, wr


for N, structured in ((30, False), (50, True)):
    p = mo.quadrotor(N)
    s = capi.Solver(p.n, p.m, N, b, structured=structured)
    s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max)
    s.set_reference(p.x_ref, p.u_ref); s.update_initialization(X0)
    s.calculate()
    st = s.get_results(want=("status",))["status"]
    print(f"N {N} {'structured' if structured else 'condensed'} handle, {b} instances: status {np.bincount(st, minlength=4).tolist()}", flush=True)
    print(f"    step                      {clock(lambda: step(s))}", flush=True)
    for name, want in (("certificate COST | RES ", COST_RES), ("certificate all four   ", ALL)):
        rd, wr = bytes_moved(p.n, p.m, N, want)
        print(f"    {name}   {clock(lambda: s._check(s.L.almpc_certificate(s.h, want)))};  reads {rd / 1e6:.1f} MB, writes {wr / 1e6:.1f} MB", flush=True)
    c = s.certificate()
    rel = c["res"] / np.maximum(1.0, np.abs(c["grad"]).max(axis=(1, 2)))
    print(f"    res / max(1, |g|_inf): median {np.median(rel):.2e}, max {rel.max():.2e}; res max {c['res'].max():.2e}; cost median {np.median(c['cost']):.4g}", flush=True)
    s.close()
