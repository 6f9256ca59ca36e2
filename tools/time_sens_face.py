"""Time the sensitivities on structured handles (k_sens_face, and k_sens_face_rate on a design with a rate weight) beside the
structured step, and at N = 30 beside k_sens on a condensed handle: quadrotor, 4096 instances, mixed amplitudes (the batch of
tools/time_structured.py).
python tools/time_sens_face.py [--rate S] [N ...]   (default 50 30)

--rate S: after the S = 0 design, the same problem with the input-rate weight S I on a structured handle, through
almpc_sensitivity_stagewise_rate / _rate_vjp (k_sens_face_rate) -- the old kernel on the S = 0 design of the same run is its yardstick.

Every figure is a host clock around a synchronous call (the calls settle the stream before they return); the Jacobian calls leave
their results on the device (no almpc_get_sensitivity in the window), the VJP calls upload g_u, g_x and bring g_x0 back, as the entry
point does.  Best and median of 20 calls after a warm-up call."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np, almpc_loader, mpc_oracle as mo
capi = almpc_loader.load_package()._capi
b = 4096
X0 = np.concatenate([mo.quadrotor_x0_batch(b // 4 if a != 1.0 else b // 2, a, first_instance=k * b) for k, a in enumerate((0.3, 1.0, 3.0))])[:b]
K0, ALL = capi.SENS["K0"], capi.SENS["K0"] | capi.SENS["dU"] | capi.SENS["dX"]
args = sys.argv[1:]
rate = 0.0
if "--rate" in args:
    i = args.index("--rate")
    rate = float(args[i + 1])
    del args[i:i + 2]


def clock(call, reps=20):
    call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return f"{1e3 * min(ts):8.3f} ms best, {1e3 * float(np.median(ts)):8.3f} ms median"


def step(s):
    s.calculate(sync=False)
    s.synchronize()


for N in [int(a) for a in args] or [50, 30]:
    p = mo.quadrotor(N)
    rng = np.random.default_rng(N)
    g_u, g_x = rng.normal(size=(b, p.m, N)), rng.normal(size=(b, p.n, N + 1))
    for structured, s_w in ((True, 0.0), (False, 0.0)) + (((True, rate),) if rate else ()):
        if not structured and p.m * N > 128:
            continue   # (no condensed handle exists)
        s = capi.Solver(p.n, p.m, N, b, structured=structured)
        s.design_shared(p.A, p.B, p.Q, p.R, s_w * np.eye(p.m) if s_w else p.S, None, p.u_min, p.u_max)
        s.set_reference(p.x_ref, p.u_ref); s.update_initialization(X0)
        s.calculate()
        if s_w:
            jac, vjp, read = s.L.almpc_sensitivity_stagewise_rate, s.sensitivity_stagewise_rate_vjp, s.sensitivity_stagewise_rate
            who = f"structured handle with S = {s_w:g} I, k_sens_face_rate"
        elif structured:
            jac, vjp, read, who = s.L.almpc_sensitivity_stagewise, s.sensitivity_stagewise_vjp, s.sensitivity_stagewise, "structured handle, k_sens_face"
        else:
            jac, vjp, read, who = s.L.almpc_sensitivity, s.sensitivity_vjp, s.sensitivity, "condensed handle, k_sens"
        st = s.get_results(want=("status",))["status"]
        print(f"N {N} {who}: status {np.bincount(st, minlength=4).tolist()}", flush=True)
        print(f"    step          {clock(lambda: step(s))}", flush=True)
        print(f"    K0            {clock(lambda: s._check(jac(s.h, K0, 0.0)))}", flush=True)
        print(f"    K0 | dU | dX  {clock(lambda: s._check(jac(s.h, ALL, 0.0)))}", flush=True)
        print(f"    VJP           {clock(lambda: vjp(g_u, g_x))}", flush=True)
        rows = read(("K0",))["rows"]
        print(f"    rows at a bound: mean {rows[rows >= 0].mean():.1f}, max {rows.max()}, unsolved {int((rows < 0).sum())}", flush=True)
        s.close()
