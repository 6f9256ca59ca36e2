"""Hashes of what one library build (ALMPC_LIB) hands out of the structured-handle sensitivities (k_sens_face, k_sens_face_rate), for a
bit-for-bit comparison of two builds:
    python tools/ab_sens_face.py OUT.npz                       (the build under ALMPC_LIB, or the in-tree one)
    python tools/ab_sens_face.py OUT.npz --against OTHER.npz   (the same, then the comparison: exit status 1 on any difference)

Per case: a solve on a structured handle, the Jacobian call with K0 | dU | dX and with K0 alone, the VJP with g_x and without.  Kept
per case: the SHA-256 of u and status (both runs must have differentiated the same solution), of K0, dU, dX, rows, of the K0 of the
K0-only call, and of g_x0 and vrows with g_x and without.  The cases (tests/sens_face_cases.py, tests/sens_face_rate_cases.py) are
the smallest that reach every shared piece of the two kernels in both of their builds:
    k_sens_face       1-1-1, 2-2-9, 9-4-12 (generic build, m = 4), 11-5-8 (m > 4: the Cholesky in LDS), 32-16-5 (n n = 1024,
                      n m = 512: the edges of the register arrays), quad-30 (the <12, 4> build), inst-5-3-12 (a model per instance)
    k_sens_face_rate  1-1-5-S, 2-1-7-S and 4-1-7-S (odd n + m: the odd edge of the 2 x 2 blocks), 8-8-6-S (m > 4), 12-4-8-S (the
                      <12, 4> build), 32-16-4-S (m (n + m) = 768: 12 look-ahead registers), 30-7-6-S ((n + m)^2 > 1024), inst-5-3-12-S
    unsolved          quad-30 under ALMPC_STRUCTURED_PRIMAL with polish_max_iter = 8 (the batch of tests/test_gpu_sens_face.py's
                      test_unsolved_instances_get_minus_one_and_zeros): rows = -1 and zeros are in the comparison"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
import numpy as np

args = sys.argv[1:]
other = None
if "--against" in args:
    i = args.index("--against")
    if i + 1 >= len(args):
        sys.exit(__doc__)
    other = args[i + 1]
    del args[i:i + 2]
if len(args) != 1:
    sys.exit(__doc__)

import almpc_loader, sens_face_cases as fc0, sens_face_gpu as fg, sens_face_rate_cases as fc1
capi = almpc_loader.load_package()._capi

PLAIN = ("1-1-1", "2-2-9", "9-4-12", "11-5-8", "32-16-5", "quad-30", "inst-5-3-12")
RATE = ("1-1-5-S", "2-1-7-S", "4-1-7-S", "8-8-6-S", "12-4-8-S", "32-16-4-S", "30-7-6-S", "inst-5-3-12-S")
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
out = {}


def keep(tag, s, rate, loss):
    jac, vjp = (s.sensitivity_stagewise_rate, s.sensitivity_stagewise_rate_vjp) if rate else (s.sensitivity_stagewise, s.sensitivity_stagewise_vjp)
    r = s.get_results(want=("u", "status"))
    sens = jac()
    g_u, g_x = loss
    got = dict(u=r["u"], status=r["status"], K0=sens["K0"], dU=sens["dU"], dX=sens["dX"], rows=sens["rows"], K0_alone=jac(("K0",))["K0"])
    got["g_x0"], got["vrows"] = vjp(g_u, g_x)
    got["g_x0_null"], got["vrows_null"] = vjp(g_u, None)
    s.close()
    for k, v in got.items():
        out["%s/%s" % (tag, k)] = np.array(sha(v))
    st = np.asarray(r["status"])
    print("%-16s unsolved %d of %d, rows %d .. %d" % (tag, int((st != 0).sum()), st.size, sens["rows"].min(), sens["rows"].max()), flush=True)
    return int((st != 0).sum())


for name in PLAIN:
    keep(name, fg.solve(capi, name, cases=fc0, batched_S=False), False, fc0.loss(name))
for name in RATE:
    keep(name, fg.solve(capi, name, cases=fc1, batched_S=True), True, fc1.loss(name))
os.environ["ALMPC_STRUCTURED_PRIMAL"] = "1"   # (a handle reads its switches when it is made)
s = fg.solve(capi, "quad-30", capi.default_opts(polish_max_iter=8), cases=fc0, batched_S=False)
del os.environ["ALMPC_STRUCTURED_PRIMAL"]
if not keep("unsolved", s, False, fc0.loss("quad-30")):
    sys.exit("the capped batch left no instance unsolved: the failure epilogue is not in the comparison")
np.savez(args[0], **out)
print("%d hashes of %d cases -> %s" % (len(out), len(PLAIN) + len(RATE) + 1, args[0]))

if other:
    ref = np.load(other)
    bad = sorted(set(out) ^ set(ref.files)) + sorted(k for k in out if k in ref.files and str(ref[k]) != str(out[k]))
    for k in bad:
        print("DIFFERENT: case %s, array %s" % tuple(k.rsplit("/", 1)))
    print("%d of %d hashes equal to %s" % (len(out) - len(bad), len(out), other))
    sys.exit(1 if bad else 0)
