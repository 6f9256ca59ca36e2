"""tests/ltv_stage_ref.py::prepare -- the numpy restatement k_ltv_stage_prepare is held against on the device -- held against the
oracle's own forms of the same terms: stage_qp_from_ltv's ebar, qu, dU (the stage-wise QP) and the input part of mpc_oracle.ltv_qp's
gradient (the dense QP).  The rounding bound of a sum of m + 2 terms, 4 (m + 2) eps sum |terms|, is the one the device test uses."""
import numpy as np
import pytest

import ltv_stage_ref
import ltv_stagewise_cases as lc

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def so():
    import stagewise_oracle
    return stagewise_oracle


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_prepare_matches_both_oracle_forms(case, mo, so):
    d = lc.generate(case)
    n, m, N = case.n, case.m, case.N
    for i in range(case.batch):
        ref = ltv_stage_ref.prepare(d["xbar"][i], d["ubar"][i], d["x_ref"], d["u_ref"], d["R"], d["S"])
        bound = 4 * (m + 2) * EPS * ref["mag"] + 1e-300
        q = lc.stage_qp(so, d, i)
        assert np.array_equal(ref["ebar"], q.ebar)
        # stage-wise form: the cost carries 2 qu_k'v_k and (v_k - v_{k+1} + dU_k)'S(...): input k's linear term is qu_k + S dU_k - S dU_{k-1}
        lin = q.qu.copy()
        if q.useS:
            lin[:-1] += q.dU @ q.S
            lin[1:] -= q.dU @ q.S
        assert np.all(np.abs(0.5 * ref["qadd"] - lin) <= bound)
        # dense form: with Q = P = 0 the gradient of ltv_qp is its input part alone
        c = None if d["c_all"] is None else d["c_all"][i]
        q_in = mo.ltv_qp(d["A_all"][i], d["B_all"][i], c, d["xbar"][i], d["ubar"][i], d["x_ref"], d["u_ref"], 0.0 * d["Q"], d["R"], d["S"],
                         0.0 * d["P"], d["umin"], d["umax"])[1]
        assert np.all(np.abs(ref["qadd"] - q_in.reshape(N, m)) <= bound)
        xr = np.zeros((n, N + 1)) if d["x_ref"] is None else d["x_ref"]
        assert np.array_equal(ref["eqt"], xr[:, N])
        if case.eq:   # the stage-wise QP's target is in dx: x_ref_N - xbar_N
            assert np.array_equal(q.eqt, ref["eqt"] - d["xbar"][i][:, N])


def test_branch_rules():
    rng = np.random.default_rng(0)
    n, m, N = 3, 2, 5
    xbar, ubar = rng.standard_normal((n, N + 1)), rng.standard_normal((m, N))
    R, S = np.eye(m) + 0.1, 0.4 * np.eye(m)
    full = ltv_stage_ref.prepare(xbar, ubar, None, None, R, S)
    assert np.abs(full["qadd"]).min() > 0.0
    assert np.array_equal(full["ebar"], xbar[:, 1:].T)   # no reference: xbar itself
    R0 = R.copy(); R0[0, 0] = 0.0
    assert not ltv_stage_ref.prepare(xbar, ubar, None, None, R0, S)["qadd"].any()        # R[0,0] == 0 drops R and S
    S0 = S.copy(); S0[0, 0] = 0.0
    no_rate = ltv_stage_ref.prepare(xbar, ubar, None, None, R, S0)["qadd"]
    assert np.array_equal(no_rate, ltv_stage_ref.prepare(xbar, ubar, None, None, R, None)["qadd"])
    assert np.allclose(no_rate, 2.0 * (0.5 * (R + R.T) @ ubar).T)
    one = ltv_stage_ref.prepare(xbar[:, :2], ubar[:, :1], None, None, R, S)["qadd"]      # N = 1: no rate pair at all
    assert np.allclose(one, 2.0 * (0.5 * (R + R.T) @ ubar[:, :1]).T)
