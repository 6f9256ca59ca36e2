"""Outputs of one library build (ALMPC_LIB) on small cases of the SQP loop and the re-linearised step (the black-box-model section of
csrc/almpc_api.hip), for a bit-for-bit comparison of two builds:
    python tools/dump_sqp_relin_cases.py OUT.npz   (once per build), then
    python tools/dump_sqp_relin_cases.py --compare A.npz B.npz [C.npz]
With C (a second dump of build A) a case A does not reproduce against C is reported and left out of the comparison with B."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
import numpy as np

KEYS = ("u", "x", "e_u", "e_x", "status", "iters")

if len(sys.argv) < 2 or (sys.argv[1] == "--compare") != (len(sys.argv) in (4, 5)) or (sys.argv[1] != "--compare" and len(sys.argv) != 2):
    sys.exit(__doc__)
if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files), "different cases"
    same = lambda p, q, k: p[k].dtype == q[k].dtype and np.array_equal(p[k], q[k], equal_nan=True)
    case = lambda k: k.rsplit("/", 1)[0]
    cases = sorted({case(k) for k in a.files})
    unstable = set()
    if len(sys.argv) == 5:
        c = np.load(sys.argv[4])
        assert sorted(a.files) == sorted(c.files), "different cases"
        unstable = {case(k) for k in a.files if not same(a, c, k)}
        print("%d of %d cases reproduce themselves" % (len(cases) - len(unstable), len(cases)), sorted(unstable))
    bad = sorted({case(k) for k in a.files if case(k) not in unstable and not same(a, b, k)})
    print("%d of %d cases equal, %d arrays compared" % (len(cases) - len(unstable) - len(bad), len(cases) - len(unstable),
                                                        sum(case(k) not in unstable for k in a.files)), bad)
    sys.exit(1 if bad or len(unstable) > 2 else 0)

import almpc_loader, mpc_oracle as mo, sqp_rows_ref as rr, densenet_ref as dn
capi = almpc_loader.load_package()._capi

out = {}


def keep(tag, s, **more):
    r = s.get_results(want=KEYS)
    for k in KEYS:
        out["%s/%s" % (tag, k)] = np.ascontiguousarray(r[k])
    for k, v in more.items():
        out["%s/%s" % (tag, k)] = np.ascontiguousarray(v)


def iterate(s, tag, iters, **more):
    try:
        st, de = s.sqp_fnn_iterate(iters)
    except capi.AlmpcError:   # an instance skipped an iteration: the histories are filled all the same
        st, de = s.sqp_last
    keep(tag, s, step_inf=st, defect_inf=de, skipped=s.sqp_fnn_skipped(), **more)


def solve(s, tag, iters, **more):
    o = s.sqp_fnn_solve(iters, 1e-6)
    keep(tag, s, solve_status=o["status"], solve_iters=o["iters"], kkt=o["kkt"], skipped=s.sqp_fnn_skipped(), **more)


n, m, b, N = 4, 2, 8, 10
f = mo.synthetic_fnn(act="tanh")
x_ref = np.tile(np.array([0.2, -0.1, 0.05, 0.0])[:, None], (1, N + 1))
u_ref = np.tile(np.array([0.1, -0.2])[:, None], (1, N))
Q, R, P, UMIN, UMAX = 100.0 * np.eye(n), 0.1 * np.eye(m), 150.0 * np.eye(n), -np.ones(m), np.ones(m)
X0 = x_ref[:, 0][None, :] + 0.6 * mo.splitmix_normal(0x5EED0005, 0, b, n)

# ---- SQP, input box: fixed steps, the merit rule to a tolerance, the exact Hessian
s = capi.Solver(n, m, N, b)
s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, UMIN, UMAX, act="tanh")
s.sqp_fnn_start(X0); iterate(s, "sqp box iterate 4", 4)
s.sqp_fnn_start(X0); solve(s, "sqp box solve", 12)
s.sqp_fnn_set_hessian("exact")
s.sqp_fnn_start(X0); solve(s, "sqp box exact solve", 12)
s.close()

# ---- SQP on the state-box fixture, row multipliers on, both Hessian modes
fb, kw, xlo, xhi, X0b = rr.state_box_fixture()
s = capi.Solver(n, m, kw["u_ref"].shape[1], len(X0b))
s.sqp_fnn_setup(fb.W_in, fb.W_h, fb.b_h, fb.W_out, kw["x_ref"], kw["u_ref"], kw["Q"], kw["R"], kw["S"], kw["P"], kw["u_min"], kw["u_max"],
                act="tanh", xmin=xlo, xmax=xhi)
s.sqp_fnn_set_row_multipliers(True)
for hessian in ("gauss_newton", "exact"):
    s.sqp_fnn_set_hessian(hessian)
    s.sqp_fnn_start(X0b); iterate(s, "sqp rows %s iterate 2" % hessian, 2, mu=s.sqp_fnn_state_multipliers())
    s.sqp_fnn_start(X0b); solve(s, "sqp rows %s solve" % hessian, 12, mu=s.sqp_fnn_state_multipliers())
s.close()

# ---- SQP with every QP stage-wise: on a condensed handle, on a structured one
for tag, structured in (("sqp set_structured", False), ("sqp structured handle", True)):
    s = capi.Solver(n, m, N, b, structured=structured)
    s.sqp_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, UMIN, UMAX, act="tanh", qp_solver="structured")
    s.sqp_fnn_start(X0); iterate(s, tag + " iterate 3", 3)
    s.close()

# ---- DenseNet
g = dn.synthetic_densenet(act="tanh")
s = capi.Solver(n, m, N, b)
s.sqp_densenet_setup(g.W_in, g.W_h, g.b_h, g.W_out, x_ref, u_ref, Q, R, None, P, UMIN, UMAX, act="tanh")
s.sqp_fnn_start(X0); iterate(s, "sqp densenet iterate 3", 3)
s.close()

# ---- the re-linearised step, condensed and structured: as set up, terminal weights from k_dare, a continuous-time network
for structured in (False, True):
    for variant in ("plain", "dare_device", "continuous"):
        s = capi.Solver(n, m, N, b, structured=structured)
        if variant == "dare_device":
            s.set_terminal_weight("dare_device")
        if variant == "continuous":
            s.set_model_time("continuous", 0.1)
        s.relin_fnn_setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, Q, R, None, P, UMIN, UMAX, act="tanh")
        tag = "relin %s %s" % ("structured" if structured else "condensed", variant)
        s.update_initialization(X0)
        s.relin_fnn_step(capi.default_opts()); keep(tag + " cold", s)
        for k in (1, 2):
            if variant == "continuous":   # (the plant of a continuous-time network is the caller's integrator)
                s.update_initialization(0.9 ** k * X0)
            else:
                s.relin_fnn_advance()
            s.relin_fnn_step(capi.default_opts(warm_start=1)); keep(tag + " warm %d" % k, s)
        s.close()
np.savez(sys.argv[1], **out)
print(os.path.basename(capi.LIB_PATH), len(out), "arrays ->", sys.argv[1])
