"""The active-set finish keeps, for every position of its working set, the element offset row * gs of that row in G (wrow_s in
polish_body, csrc/almpc_kernels.hip.h): the cases at which a wrong offset can survive the other suites.  Run on an MI355X:
pytest -m gpu.

Every case is one cold step of batch 37 at the benchmark's operating point (stiffness profile, rho = 45, K = 6 ADMM iterations, one
check), structured_fallback=False, shapes from tests/condensed_step_cases.py and tests/instance_step_cases.py.  Each is held to the
exact oracle at the suite's 1e-6 on u and 1e-4 on x (every third instance, the heavy cases every one), and every instance must come
back with status 0.

    4-1-113          k_step_fused<8,30>           nz odd: gs = 114 != nz, an offset scaled by the wrong stride shows
    12-4-30          k_step_fused<8,30>           amplitudes 1, 3 and 6: more than one chunk; the workgroup-shared second tier (> 32 rows)
    7-5-25-heavy     k_admm + k_polish<true>      working sets up to 58 rows: memory mode, slot_to_global
    16-1-128         k_admm + k_polish<false>     G in global memory, gs = nzs
    3-2-6            k_step_inst_wave<16>         the one-wave route
    4-2-32-heavy     k_admm_inst + k_polish_sgl   per-instance models, G_i in the wave's LDS (ALMPC_NO_INST_WAVE=1)
    3-29-4           k_step_fused<8,30>           m > 24: the stage-by-stage rollout in the tail (% m indexing)
    5-4-28           k_admm + k_polish<true>      the blocked rollout (lane -> stage, row)

What the cases make the finish do, from trace_finish below (the oracle's active-set restatement mo.polish_active_set with the
kernel's position order -- the last position moves into the hole of a removal -- and counters; it agrees with the oracle's own
counts on every instance) on the ADMM iterates of cc.admm at this operating point, per case over the 37 instances:
instances with a removal that fills a hole (rp != last) / with a purge pass (two or more wrong-sign rows dropped together, the
inverse rebuilt) / largest working set beyond 8, 32, 48 rows / undecided:

    4-1-113           0 /  0 /   7,  0,  0 / 0        (largest set 14)
    12-4-30 amp 1     0 /  0 /   0,  0,  0 / 0        (largest set 7)
    12-4-30 amp 3     1 /  0 /  18,  0,  0 / 0        (largest set 22)
    12-4-30 amp 6     2 /  1 /  34,  3,  1 / 0        (largest set 50)
    7-5-25-heavy     10 /  3 /  36, 11,  2 / 0        (largest set 58)
    16-1-128          0 /  0 /   3,  0,  0 / 0        (largest set 10)
    3-2-6             0 /  0 /   3,  0,  0 / 0        (largest set 10)
    4-2-32-heavy      0 /  0 /  32,  5,  2 / 0        (largest set 57)
    3-29-4            0 /  0 /   4,  0,  0 / 0        (largest set 23)
    5-4-28            2 /  1 /   2,  0,  0 / 0        (largest set 15)

(python tests/test_gpu_finish_offsets.py prints this table; it needs no GPU.)"""
import functools

import numpy as np
import pytest

import condensed_step_cases as cc
import instance_step_cases as ic
import mpc_oracle as mo

U_TOL = 1e-6
X_TOL = 1e-4
PROFILE, RHO, K = "stiffness", 45.0, 6
OPTS = dict(rho=RHO, max_iter=K, check_every=K)
QUAD_AMPS = (1.0, 3.0, 6.0)
SHARED = ("4-1-113", "7-5-25-heavy", "16-1-128", "3-2-6", "3-29-4", "5-4-28")
ROUTES = {"4-1-113": "fused", "12-4-30": "fused", "7-5-25-heavy": "tile", "16-1-128": "tile_l2", "3-2-6": "wave", "3-29-4": "fused",
          "5-4-28": "tile"}
INST = "4-2-32-heavy"


# ---------------------------------------------------------------------------- the finish on the CPU, with counters
def trace_finish(G, v0, lo, hi, z, y):
    """mo.polish_active_set in the kernel's position order: dict(w, n_add, n_remove, n_purged, n_active, holes, kmax, decided)"""
    nz = v0.size
    w = np.clip(z, lo, hi)
    W = [j for j in range(nz) if (y[j] < 0 and w[j] <= lo[j]) or (y[j] > 0 and w[j] >= hi[j])]
    side = {j: (-1 if y[j] < 0 else 1) for j in W}
    kmax = len(W)

    def face():
        b = np.array([hi[j] if side[j] > 0 else lo[j] for j in W])
        r = v0[W] - b
        K_ = G[np.ix_(W, W)]
        lam = np.linalg.solve(K_, r)
        lam = lam + np.linalg.solve(K_, r - K_ @ lam)
        viol = np.array([-lam[i] if side[W[i]] > 0 else lam[i] for i in range(len(W))])
        return b, lam, viol

    n_add = n_rem = n_purged = holes = 0
    if 0 < len(W) <= 32:
        _, lam, viol = face()
        bad = viol > 1e-12 * max(1.0, float(np.max(np.abs(lam))))
        if bad.sum() >= 2:
            n_purged = int(bad.sum())
            n_rem += n_purged
            W = [W[i] for i in range(len(W)) if not bad[i]]
            side = {j: side[j] for j in W}
    decided = False
    for _ in range(2 * nz + 50):
        t = v0.copy()
        if W:
            b, lam, viol = face()
            t = v0 - G[:, W] @ lam
            t[W] = b
        step = t - w
        free = np.ones(nz, dtype=bool)
        free[W] = False
        with np.errstate(divide="ignore", invalid="ignore"):
            r_hi = np.where(free & (t > hi), (hi - w) / step, np.inf)
            r_lo = np.where(free & (t < lo), (lo - w) / step, np.inf)
        rr = np.minimum(r_hi, r_lo)
        j = int(np.argmin(rr))
        if rr[j] < 1.0:
            w = w + max(rr[j], 0.0) * step
            up = r_hi[j] <= r_lo[j]
            w[j] = hi[j] if up else lo[j]
            W.append(j)
            side[j] = 1 if up else -1
            n_add += 1
            kmax = max(kmax, len(W))
            continue
        w = t
        if not W:
            decided = True
            break
        i = int(np.argmax(viol))
        if viol[i] <= 1e-12 * max(1.0, float(np.max(np.abs(lam)))):
            decided = True
            break
        del side[W[i]]
        if i != len(W) - 1:     # the kernel's remove_pos: the last position moves into the hole
            holes += 1
            W[i] = W[-1]
        W.pop()
        n_rem += 1
    return dict(w=np.clip(w, lo, hi), n_add=n_add, n_remove=n_rem, n_purged=n_purged, n_active=len(W), holes=holes, kmax=kmax,
                decided=decided)


def _trace_instance(p, des, x0_):
    fs = cc.fs_of(p, des, x0_)
    a = cc.admm(des, fs, max_iter=K, check_every=K)
    v0 = -des["G"] @ fs
    t = trace_finish(des["G"], v0, des["lo"], des["hi"], a["z"], a["y"])
    o = mo.polish_active_set(des["G"], v0, des["lo"], des["hi"], a["z"], a["y"])
    same = all(t[k] == o[k] for k in ("n_add", "n_remove", "n_purged", "n_active")) and float(np.abs(t["w"] - o["w"]).max()) <= 1e-9
    return t, same


def finish_counts():
    """{row of the table in the docstring: (holes, purges, > 8, > 32, > 48, undecided, kmax, agrees with the oracle)}"""
    out = {}
    rows = [(cid, None) for cid in SHARED[:1]] + [("12-4-30", a) for a in QUAD_AMPS] + [(cid, None) for cid in SHARED[1:3]]
    rows += [(SHARED[3], None), (INST, None)] + [(cid, None) for cid in SHARED[4:]]
    for cid, amp in rows:
        if cid == INST:
            c = ic.CASE_BY_ID[cid]
            X0, des = ic.x0(c), ic.designs(c, PROFILE, RHO)
            tr = [_trace_instance(ic.problem(c, i), des[i], X0[i]) for i in range(c.batch)]
        else:
            c = cc.CASE_BY_ID[cid]
            p, X0 = cc.problem(c), cc.x0(c, amp)
            des = mo.design_shared(p, rho=RHO, rho_profile=PROFILE)
            tr = [_trace_instance(p, des, X0[i]) for i in range(cc.BATCH)]
        t = [a for a, _ in tr]
        out[cid + ("" if amp is None else " amp %g" % amp)] = (
            sum(a["holes"] > 0 for a in t), sum(a["n_purged"] > 0 for a in t), sum(a["kmax"] > 8 for a in t), sum(a["kmax"] > 32 for a in t),
            sum(a["kmax"] > 48 for a in t), sum(not a["decided"] for a in t), max(a["kmax"] for a in t), all(s for _, s in tr))
    return out


# ---------------------------------------------------------------------------- the GPU runs
def _check(r, exact, who):
    assert np.all(r["status"] == 0), (who, np.nonzero(r["status"])[0].tolist())
    err_u = max(float(np.abs(r["u"][i] - e["u"]).max()) for i, e in exact.items())
    err_x = max(float(np.abs(r["x"][i] - e["x"]).max()) for i, e in exact.items())
    print("finish-offsets %s exact-u %.3e of %.1e exact-x %.3e of %.1e" % (who, err_u, U_TOL, err_x, X_TOL))
    assert err_u <= U_TOL and err_x <= X_TOL, (who, err_u, err_x)


@functools.lru_cache(maxsize=None)
def _quad_exact(amp):
    c = cc.CASE_BY_ID["12-4-30"]
    if amp == c.amp:
        return cc.reference(c)["exact"]
    return cc.exact_batch(cc.problem(c), cc.x0(c, amp), c.exact)


def _shared_step(capi, c, X0, monkeypatch, env=()):
    p = cc.problem(c)
    with monkeypatch.context() as mp:
        for k, v in dict(env).items():
            mp.setenv(k, v)
        s = capi.Solver(p.n, p.m, p.N, len(X0), structured_fallback=False)
    s.design_shared(p.A, p.B, p.Q, p.R, p.S, None, p.u_min, p.u_max, rho=RHO, rho_profile=PROFILE)
    s.set_reference(p.x_ref, p.u_ref)
    s.update_initialization(X0)
    s.calculate(capi.default_opts(**OPTS))
    r = s.get_results()
    s.close()
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("cid", SHARED)
def test_shared_model_finish_against_the_exact_oracle(capi, cid, monkeypatch):
    c = cc.CASE_BY_ID[cid]
    assert c.route == ROUTES[cid]
    ref = cc.reference(c)
    _check(_shared_step(capi, c, ref["X0"], monkeypatch), ref["exact"], "%s %s" % (cid, c.route))


@pytest.mark.gpu
@pytest.mark.parametrize("amp", QUAD_AMPS)
def test_quadrotor_finish_at_three_amplitudes(capi, amp, monkeypatch):
    c = cc.CASE_BY_ID["12-4-30"]
    assert c.route == ROUTES[c.id]
    _check(_shared_step(capi, c, cc.x0(c, amp), monkeypatch), _quad_exact(amp), "%s amp %g %s" % (c.id, amp, c.route))


@pytest.mark.gpu
def test_per_instance_finish_with_g_in_the_waves_lds(capi, monkeypatch):
    c = ic.CASE_BY_ID[INST]
    assert ic.step_kernels(*c.shape, c.batch, PROFILE, True, ic.NO_WAVE)[1] == ("polish", "sgl")
    with monkeypatch.context() as mp:
        for k, v in ic.NO_WAVE.items():
            mp.setenv(k, v)
        s = capi.Solver(c.n, c.m, c.N, c.batch, structured_fallback=False)
    A, B = ic.models(c)
    t = ic.template(c)
    s.design_batched(A, B, t.Q, t.R, t.S, t.P, t.u_min, t.u_max, rho=RHO, rho_profile=PROFILE)
    s.set_reference(t.x_ref, t.u_ref)
    s.update_initialization(ic.x0(c))
    s.calculate(capi.default_opts(**OPTS))
    r = s.get_results()
    s.close()
    _check(r, ic.reference(c)["exact"], "%s k_polish_sgl" % c.id)


if __name__ == "__main__":
    for name, v in finish_counts().items():
        print("    %-16s %2d / %2d /  %2d, %2d, %2d / %d        (largest set %d)%s" % (name, *v[:7], "" if v[7] else "   DIFFERS FROM THE ORACLE"))
