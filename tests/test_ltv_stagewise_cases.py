"""The case table of tests/ltv_stagewise_cases.py, held on the CPU from the oracle alone: every case poses what its row says, and the
stage-wise oracle agrees with the dense exact solvers where the dense form exists (the two open-loop unstable cases are the ones
condensing loses: see the table's docstring)."""
import numpy as np
import pytest

import ltv_stagewise_cases as lc

DENSE_TOL = 1e-8


@pytest.fixture(scope="module")
def so():
    import stagewise_oracle
    return stagewise_oracle


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_case_poses_what_the_table_says(case, mo, so):
    d, res = lc.answers(case)
    b, N, m = case.batch, case.N, case.m
    status = [r["status"] for r in res]
    assert 3 <= b <= 8
    assert set(status) <= {0, 3}, status                      # solved or proven infeasible, nothing else
    infeasible = status.count(3)
    assert 3 * infeasible <= b, status                        # at most a third
    assert (infeasible > 0) == (not case.feasible), status    # the "tight" cases hold infeasible instances, the others none
    if not case.rows:
        assert infeasible == 0                                # an input box alone is always feasible
        assert sum(r["n_active_u"] for r in res) >= N * m / 4
    elif case.feasible:
        assert sum(r["n_active_x"] for r in res) >= 1         # a state row holds somewhere in the batch
    # the route of the step and the shape limits of the entry point
    nt = case.n + (case.m if (case.s != 0.0 and not case.r00_zero) else 0)
    if case.route == "sdual":
        assert nt <= 16 and case.m <= 8
    else:
        assert case.n <= 32 and case.m <= 16
    if not case.dense:
        return
    assert m * N <= 160
    for i in range(b):
        v = lc.dense_solve(mo, d, i)
        if res[i]["status"] == 3:
            assert v is None
            continue
        assert v is not None
        assert np.abs(v - res[i]["v"]).max() <= DENSE_TOL


def test_the_table_covers_the_builds_and_branches():
    names = {c.name for c in lc.CASES}
    assert len(names) == len(lc.CASES)
    by = lc.BY_NAME
    assert by["widest-11-5-8"].n + 0 <= 16 and by["widest-11-5-8"].m > 4        # the (16, 8) build: nt <= 16, m in 5..8
    assert by["smallest-2-1-2"].N == 2 and by["smallest-2-1-2"].s != 0.0 and by["smallest-2-1-2"].eq   # one rate pair
    assert by["r00-3-1-37"].r00_zero and by["r00-3-1-37"].route == "riccati"     # R[0,0] = 0 drops R and S: the Riccati route
    assert by["nullrefs-4-2-16"].null_refs
    assert any(c.m * c.N > 128 for c in lc.CASES)                                # beyond the condensed design's limit
    assert any(c.a > 1.0 and c.route == "riccati" for c in lc.CASES) and any(c.a > 1.0 and c.route == "sdual" for c in lc.CASES)
    d = lc.generate(by["nullrefs-4-2-16"])
    assert d["x_ref"] is None and d["u_ref"] is None and d["c_all"] is None
