"""CPU tests of the case table behind tests/test_gpu_stagewise_shapes.py (tests/stagewise_shape_cases.py): the table names every build of
k_sdual and k_riccati that csrc/almpc_api.hip instantiates -- a build added later without a case fails here --, every build sees every
feature at an exact-fit and at a padded shape, and every instance the GPU tests compare is well posed: the exact oracle
(mpc_oracle.solve_mpc_exact: KKT certificate, ValueError for an infeasible problem) and the restatement of the kernel's algorithm
(stagewise_oracle.solve_mpc_stagewise) give the same verdict and the same inputs, with the constraints of the case active."""
import os
import re

import numpy as np
import pytest

import stagewise_shape_cases as sc
from conftest import ROOT

API = os.path.join(ROOT, "automationlabsmodelpredictivecontrol.jl_amd", "csrc", "almpc_api.hip")


def _pairs(text):
    return tuple((int(a), int(b)) for a, b in re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*\}", text))


def test_the_table_names_the_builds_the_source_instantiates():
    with open(API) as f:
        src = f.read()
    lines = [ln for ln in src.splitlines() if re.search(r"\bSD_SHAPES\s*\[\s*\]\s*\[\s*2\s*\]\s*=", ln)]
    assert len(lines) == 1
    assert _pairs(lines[0]) == sc.SD_SHAPES
    launched = tuple((int(a), int(b)) for a, b in re.findall(r"\bRICCATI_LAUNCH\(\s*(\d+)\s*,\s*(\d+)\s*\)", src))
    assert launched[-1] == (0, 0) and launched.count((0, 0)) == 1          # the generic build, last
    assert launched[:-1] == sc.RICCATI_SHAPES
    # the selection rule and the horizon limit as the source states them
    assert "if (nt <= s[0] && m <= s[1])" in src
    assert "(N + 64 / (NT + MC)) / (64 / (NT + MC)) > 64" in src
    for b in sc.SD_SHAPES:
        G = sc.G_of(b)
        assert (sc.n_max(b) + G) // G == 64 and (sc.n_max(b) + 1 + G) // G == 65


def test_pick_build_takes_the_first_pair_that_covers():
    assert sc.pick_build(1, 1) == (2, 2) and sc.pick_build(3, 1) == (4, 2) and sc.pick_build(4, 3) == (8, 4)
    assert sc.pick_build(13, 5) == (16, 8) and sc.pick_build(17, 1) == (32, 16) and sc.pick_build(33, 2) == (48, 16)
    assert sc.pick_build(49, 1) is None and sc.pick_build(4, 17) is None
    assert [sc.G_of(b) for b in sc.SD_SHAPES] == [16, 10, 8, 5, 4, 3, 2, 1, 1]


def test_every_build_sees_every_feature_exact_fit_and_padded():
    ids = [c.id for c in sc.CASES]
    assert len(set(ids)) == len(ids)
    for b in sc.SD_SHAPES:
        cs = [c for c in sc.CASES if c.build == b]
        assert any(c.exact_fit for c in cs), b
        assert any(c.padded for c in cs), b
        assert {c.feat for c in cs} == set(sc.FEATURES), b
        # every build is reachable with S ((NT - 1, 1) = (n, m) with n + m = NT); a structured handle takes n <= 32, so (48, 16) only so
        assert any(c.S for c in cs), b
        if b == (48, 16):
            assert all(c.S for c in cs)
    for c in tuple(sc.CASES) + tuple(sc.EDGE_CASES):
        assert c.build is not None and c.n <= 32 and c.N <= sc.n_max(c.build), c.id
        assert c.batch == 37
        if c.has_eq:            # a single-input plant with the terminal equality is ill posed
            assert c.m >= 2 and c.m * c.N >= 2 * c.n, c.id
    assert {c.build for c in sc.EDGE_CASES} == {(16, 8), (32, 16)}
    assert all(c.N == sc.n_max(c.build) for c in sc.EDGE_CASES)
    # k_riccati: every specialised build, and shapes that only the generic one takes
    shapes = {(c.n, c.m) for c in sc.RICCATI_CASES}
    assert set(sc.RICCATI_SHAPES) <= shapes and len(shapes - set(sc.RICCATI_SHAPES)) >= 3
    assert all(c.feat == "ubox" and not c.S for c in sc.RICCATI_CASES)


@pytest.mark.parametrize("case", tuple(sc.CASES) + tuple(sc.EDGE_CASES), ids=lambda c: c.id)
def test_compared_instances_are_well_posed_with_their_constraints_active(case):
    ref = sc.reference(case)
    p, X0 = ref["p"], ref["X0"]
    n_ok = n_inf = act_u = n_act_x = last_u = last_x = 0
    for i in case.compared:
        e = ref["exact"][i] if i in ref["exact"] else sc.exact_or_none(p, X0[i])          # (RuntimeError: not certified -> the test fails)
        r = ref["restated"][i] if i in ref["restated"] else sc.restate(p, X0[i])
        if e is None:
            assert r["status"] == 3, (i, r["status"])
            n_inf += 1
            continue
        assert r["status"] == 0, (i, r["status"])
        assert np.abs(r["u"] - e["u"]).max() <= 1e-9, (i, np.abs(r["u"] - e["u"]).max())
        n_ok += 1
        act_u += sc.active_inputs(p, e["u"])
        n_act_x += sc.active_states(p, e["x"]) > 0
        last_u += sc.active_inputs(p, e["u"][:, -1:])
        last_x += sc.active_states(p, e["x"][:, -2:])
    assert n_ok >= 1
    if case in sc.CASES:
        if case.feat == "ubox":
            assert act_u >= 1 and n_inf == 0
        if case.feat == "xbox":
            assert n_act_x >= 1 and n_inf >= 1
    if case in sc.EDGE_CASES:      # the rows that use bit 63 of the working-set mask are active (eq: the terminal rows always are)
        if case.feat == "xbox":
            assert last_x >= 1
        else:
            assert last_u >= 1
