"""Outputs of one library build (ALMPC_LIB) on the small cases of tests/test_gpu_step_critical_path.py, for a bit-for-bit comparison of
two builds:  python tools/dump_critical_path_cases.py OUT.npz   (once per build), then
             python tools/dump_critical_path_cases.py --compare A.npz B.npz"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
import numpy as np

KEYS = ("u", "e_u", "x", "e_x", "status", "iters", "polish_iters")

if len(sys.argv) not in (2, 4) or (len(sys.argv) == 4) != (sys.argv[1] == "--compare"):
    sys.exit(__doc__)
if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files), "different cases"
    bad = [k for k in a.files if not (a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]))]
    print("%d arrays compared, %d differ" % (len(a.files), len(bad)), bad[:10])
    sys.exit(1 if bad else 0)

import almpc_loader, bench, mpc_oracle as mo, condensed_step_cases as cc
capi = almpc_loader.load_package()._capi


class t:   # the inputs of tests/test_gpu_step_critical_path.py, restated (a tool does not import the test suite)
    BATCH = cc.BATCH
    FINISH_AMPS, FINISH_K, FINISH_RHO = (1.0, 2.0, 3.0, 4.0, 6.0), (1, 2, 6), 45.0
    ADMM_CASES = tuple(cc.CASE_BY_ID[i] for i in ("3-2-6", "6-1-41", "12-4-30", "11-11-11", "56-2-1"))
    PROFILES = (("scalar", 0.1), ("stiffness", 30.0))
    ITERATE_OPTS = ((1, 1), (2, 1), (7, 1), (7, 2), (7, 7))
    LOOSE = dict(eps_abs=0.1, eps_rel=0.1, max_iter=12, check_every=1)

    @staticmethod
    def _admm_solver(capi, p, batch, rho, profile, refs=None):
        s = capi.Solver(p.n, p.m, p.N, batch, structured_fallback=False)
        s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=rho, rho_profile=profile)
        if refs is None:
            s.set_reference(p.x_ref, p.u_ref)
        else:
            s.set_reference(refs[0], refs[1], per_instance=True)
        return s

    @staticmethod
    def _run(s, o):
        s.calculate(o)
        return s.get_results()


out = {}


def keep(tag, r):
    for k in KEYS:
        out["%s/%s" % (tag, k)] = np.ascontiguousarray(r[k])


# the finish cases: every amplitude, K, with and without the warm state, on the three routes
p = mo.quadrotor()
for name, env, fusion in (("fused", {}, True), ("tile", {}, False), ("tile_l2", {"ALMPC_POLISH_NO_GLDS": "1"}, True)):
    os.environ.update(env)
    s = capi.Solver(p.n, p.m, p.N, t.BATCH, structured_fallback=False)
    for k in env:
        del os.environ[k]
    s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=t.FINISH_RHO, rho_profile="stiffness")
    s.set_reference(p.x_ref, p.u_ref)
    s.set_step_fusion(fusion)
    for amp in t.FINISH_AMPS:
        X0 = bench.make_x0(mo, 0, t.BATCH, amp)
        for K in t.FINISH_K:
            for kw in (True, False):
                s.update_initialization(X0)
                s.calculate(capi.default_opts(rho=t.FINISH_RHO, max_iter=K, check_every=K, keep_warm_state=kw))
                keep("finish %s amp %g K %d keep %d" % (name, amp, K, kw), s.get_results())
    s.close()

# the ADMM cases: iterates, the loose tolerance, a warm start; batch 37 and 1; shared and per-instance references
for case in t.ADMM_CASES:
    p, X0f = cc.problem(case), cc.x0(case)
    xr = np.ascontiguousarray(np.broadcast_to(p.x_ref[None], (t.BATCH,) + p.x_ref.shape))
    ur = np.ascontiguousarray(np.broadcast_to(p.u_ref[None], (t.BATCH,) + p.u_ref.shape))
    for profile, rho in t.PROFILES:
        for batch in (t.BATCH, 1):
            for refs in (None, (xr[:batch], ur[:batch])):
                s = t._admm_solver(capi, p, batch, rho, profile, refs=refs)
                X0 = X0f[:batch]
                s.update_initialization(X0)
                tag = "admm %s %s batch %d %s" % (case.id, profile, batch, "shared" if refs is None else "per-instance")
                for mi, ce in t.ITERATE_OPTS:
                    keep("%s it %d/%d" % (tag, mi, ce), t._run(s, capi.default_opts(rho=rho, polish=0, max_iter=mi, check_every=ce)))
                keep(tag + " loose", t._run(s, capi.default_opts(rho=rho, polish=0, **t.LOOSE)))
                keep(tag + " cold", t._run(s, capi.default_opts(rho=rho, polish=0, max_iter=7, check_every=2)))
                s.update_initialization(0.9 * X0)
                keep(tag + " warm", t._run(s, capi.default_opts(rho=rho, polish=0, warm_start=1, max_iter=7, check_every=2)))
                s.close()
np.savez(sys.argv[1], **out)
print(os.path.basename(capi.LIB_PATH), len(out), "arrays ->", sys.argv[1])
