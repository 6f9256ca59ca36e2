"""Host-side mirror of the reference interface: argument handling and error behaviour (CPU only)."""
import os

import numpy as np
import pytest

from conftest import ROOT


def test_design_reference_broadcast(pkg):
    # src/main/main_mpc.jl:105-117: x = x_ref .* ones(n, N+1), u = u_ref .* ones(m, N)
    r = pkg._design_reference_mpc([0.65] * 4, [1.2, 1.3], 5)
    assert r.x.shape == (4, 6) and r.u.shape == (2, 5)
    assert np.all(r.x == 0.65) and np.all(r.u[0] == 1.2) and np.all(r.u[1] == 1.3)


def test_weights_defaults_and_kws_idiom(pkg):
    sys_ = pkg.ConstrainedLinearControlDiscreteSystem(np.eye(3), np.ones((3, 2)), pkg.Hyperrectangle([0] * 3, [1] * 3),
                                                      pkg.Hyperrectangle([0, 0], [1, 1]))
    w = pkg._create_weights_coefficients(sys_)
    assert np.array_equal(w.Q, 100 * np.eye(3)) and np.array_equal(w.R, 0.1 * np.eye(2)) and not w.S.any()
    w = pkg._create_weights_coefficients(sys_, kws=dict(mpc_Q=7.0, mpc_S=2.0))  # kws passed through, as the reference does
    assert w.Q[0, 0] == 7.0 and w.S[1, 1] == 2.0
    w = pkg._create_weights_coefficients(sys_, mpc_R=3.0)
    assert w.R[0, 0] == 3.0


def _sys(pkg):
    return pkg.ConstrainedLinearControlDiscreteSystem([[1, 1], [0, 1]], [[0.5], [1.0]], pkg.Hyperrectangle([-5, -5], [5, 5]),
                                                      pkg.Hyperrectangle([-1], [1]))


def test_proceed_controller_argument_errors(pkg):
    s = _sys(pkg)
    assert pkg.proceed_controller(s, "economic_model_predictive_control", 10, 1, [0, 0], [0]) is None  # removed in v0.1.4
    with pytest.raises(TypeError):
        pkg.proceed_controller(s, "model_predictive_control", 10, 1.5, [0, 0], [0])  # sample time must be Int
    with pytest.raises(KeyError):
        pkg.proceed_controller(s, "model_predictive_control", 10, 1, [0, 0], [0], mpc_solver="highs")
    with pytest.raises(KeyError):
        pkg.proceed_controller(s, "model_predictive_control", 10, 1, [0, 0], [0], mpc_programming_type="quadratic")
    for kw in (dict(mpc_solver="osqp"), dict(mpc_programming_type="non_linear"), dict(mpc_terminal_ingredient="contractive")):
        with pytest.raises(NotImplementedError):
            pkg.proceed_controller(s, "model_predictive_control", 10, 1, [0, 0], [0], **kw)


def test_design_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg._capi.AlmpcError):
        pkg.proceed_controller(_sys(pkg), "model_predictive_control", 10, 1, [0, 0], [0])


def test_system_validation(pkg):
    with pytest.raises(ValueError):
        pkg.Hyperrectangle([1.0], [0.0])
    with pytest.raises(ValueError):
        pkg.ConstrainedLinearControlDiscreteSystem(np.eye(2), np.ones((3, 1)), pkg.Hyperrectangle([0, 0], [1, 1]),
                                                   pkg.Hyperrectangle([0], [1]))


@pytest.mark.parametrize("batch,world", [(4096, 1), (32768, 8), (10, 3), (5, 8), (0, 2)])
def test_shard_range_partitions(pkg, batch, world):
    rs = [pkg.shard_range(batch, r, world) for r in range(world)]
    assert rs[0][0] == 0 and rs[-1][1] == batch
    assert all(rs[i][1] == rs[i + 1][0] for i in range(world - 1))
    sizes = [b - a for a, b in rs]
    assert max(sizes) - min(sizes) <= 1 and sorted(sizes, reverse=True) == sizes
    with pytest.raises(ValueError):
        pkg.shard_range(batch, world, world)


def test_aggregate_rate(pkg):
    assert pkg.sharding.aggregate_rate(4096, 10, 2.0, 8) == 8 * 4096 * 10 / 2.0


def test_workloads_module_matches_the_oracle_generators(pkg, mo):
    """bench.py takes its synthetic inputs from the product-side workloads module (it may not route inputs through oracle/);
    the oracle keeps its own copies for the tests: the two must produce identical arrays."""
    import importlib
    wl = importlib.import_module(pkg.__name__ + ".workloads")
    assert np.array_equal(wl.splitmix_normal(0x5EED0002, 5, 9, 12), mo.splitmix_normal(0x5EED0002, 5, 9, 12))
    assert np.array_equal(wl.quadrotor_x0_batch(7, 3.0, first_instance=11), mo.quadrotor_x0_batch(7, 3.0, first_instance=11))
    A, B = wl.quadrotor_model()
    Ao, Bo = mo.quadrotor_model()
    assert np.array_equal(A, Ao) and np.array_equal(B, Bo)
    q, qo = wl.quadrotor(30), mo.quadrotor(30)
    for k in ("Q", "R", "S", "u_min", "u_max", "x_ref", "u_ref"):
        assert np.array_equal(getattr(q, k), getattr(qo, k)), k
    W_in, W_h, b_h, W_out = wl.synthetic_fnn_weights()
    fo = mo.synthetic_fnn(act="tanh")
    A0, _ = mo.FnnModel(W_in, W_h, b_h, W_out, "tanh").jacobian(np.zeros(4), np.zeros(2))
    assert np.array_equal(W_in, fo.W_in) and np.array_equal(W_h[1], fo.W_h[1]) and np.array_equal(b_h[0], fo.b_h[0])
    assert np.array_equal(wl.scale_to_radius(W_out, A0), fo.W_out)
    # the reference's own test size: the product-side constants are the values the oracle decodes from the reference-held fixture
    import os
    from conftest import ROOT
    Af, Bf = mo.decode_linear_regressor_fixture(open(os.path.join(ROOT, "tests", "golden", "linear_regressor_train_result.jls"), "rb").read())
    qf, qfo = wl.qtp_fixture(), mo.qtp_linear_fixture_problem(Af, Bf)
    assert np.array_equal(qf.A, Af) and np.array_equal(qf.B, Bf)
    for k in ("Q", "R", "S", "u_min", "u_max", "x_ref", "u_ref"):
        assert np.array_equal(getattr(qf, k), getattr(qfo, k)), k


def test_bench_dump_outputs_cap_and_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: one float64 .npy per result array; a batch beyond the size cap is cut to a fixed, seeded sample of
    instances (the same rows of every array, indices in instance_index.npy) that fits the cap."""
    import bench
    rng = np.random.default_rng(3)
    b, n, m, N = 500, 3, 2, 4
    res = {"x": rng.standard_normal((b, n, N + 1)), "e_x": rng.standard_normal((b, n, N + 1)), "u": rng.standard_normal((b, m, N)),
           "e_u": rng.standard_normal((b, m, N)), "status": rng.integers(0, 3, b).astype(np.int32), "iters": np.zeros(b, np.int32)}
    bench.write_outputs(str(tmp_path / "all"), res)
    assert sorted(os.listdir(tmp_path / "all")) == ["e_u.npy", "e_x.npy", "status.npy", "u.npy", "x.npy"]
    for k in bench.DUMP_NAMES:
        a = np.load(tmp_path / "all" / (k + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, res[k])
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100_000)
    for d in ("s1", "s2"):
        bench.write_outputs(str(tmp_path / d), res)
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 100_000
    idx = np.load(tmp_path / "s1" / "instance_index.npy").astype(np.int64)
    assert 0 < len(idx) < b and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "s2" / "instance_index.npy"))
    for k in bench.DUMP_NAMES:
        assert np.array_equal(np.load(tmp_path / "s1" / (k + ".npy")), res[k][idx].astype(np.float64))


def _reference_stand_in(patch_text, golden):
    """The reference's files as far as the patch knows them: every preimage line of every hunk (context and removed lines) at its own
    line number, a comment line wherever the patch carries none, as many lines as the reference file has (tests/golden)."""
    import re
    out, cur, old = {}, None, 0
    for ln in patch_text.splitlines():
        if ln.startswith("diff --git"):
            path = ln.split(" b/")[1].strip()
            cur = [f"# reference line {k + 1}" for k in range(golden[path]["lines"])] if path in golden else None
            if cur is not None:
                out[path] = cur
        elif cur is None or ln.startswith(("index ", "--- ", "+++ ")):
            continue
        elif ln.startswith("@@"):
            old = int(re.match(r"@@ -(\d+)", ln).group(1)) - 1
        elif ln.startswith((" ", "-")):
            assert old < len(cur), "hunk beyond the end of the reference file"
            cur[old] = ln[1:]
            old += 1
    return {path: "\n".join(lines) + "\n" for path, lines in out.items()}


def test_reference_side_patch_applies_to_the_reference(tmp_path):
    """julia/reference_hip.patch (the reference-side edits of INTEGRATION.md as an actual diff: hip_solver_def tag, "hip" in
    _IMPLEMENTATION_SOLVER_LIST, the design branches of the linear-system AND the black-box method to
    _model_predictive_control_design_hip, batch-sized result arrays, the dispatch in update_initialization! / calculate!, and the
    shim itself as src/hip/AlmpcHIP.jl) was made against the reference's own files (its preimage blobs are the ones
    tests/golden/reference_files.json records), applies cleanly, and is what julia/make_reference_patch.py produces from the current
    shim.  The reference's files are stood in for by the preimage lines the patch itself carries."""
    import importlib.util
    import json
    import re
    import subprocess
    with open(os.path.join(ROOT, "tests", "golden", "reference_files.json")) as f:
        golden = json.load(f)["files"]
    files = ["src/types/types.jl", "src/sub/solver_selection.jl", "src/sub/design_mpc.jl", "src/main/computation_mpc.jl",
             "src/AutomationLabsModelPredictiveControl.jl"]
    assert sorted(golden) == sorted(files)
    patch = os.path.join(ROOT, "julia", "reference_hip.patch")
    patch_text = open(patch).read()
    touched = {ln.split(" b/")[1].strip() for ln in open(patch) if ln.startswith("diff --git")}
    assert touched == set(files) | {"src/hip/AlmpcHIP.jl"}
    # the preimage of every edited file is the reference's blob; the added shim is julia/AlmpcHIP.jl's blob
    index = dict(re.findall(r"^diff --git a/\S+ b/(\S+)\n(?:new file mode \d+\n)?index (\S+)", patch_text, re.M))
    assert sorted(index) == sorted(touched)
    for f in files:
        assert golden[f]["git_blob"].startswith(index[f].split("..")[0]), f
    shim_blob = subprocess.check_output(["git", "hash-object", os.path.join(ROOT, "julia", "AlmpcHIP.jl")], text=True).strip()
    assert index["src/hip/AlmpcHIP.jl"].startswith("0000000..") and shim_blob.startswith(index["src/hip/AlmpcHIP.jl"].split("..")[1])
    ref = tmp_path / "reference"
    for f, text in _reference_stand_in(patch_text, golden).items():
        os.makedirs(os.path.dirname(ref / f), exist_ok=True)
        with open(ref / f, "w") as fo:
            fo.write(text)
        assert len(text.splitlines()) == golden[f]["lines"], f
    work = tmp_path / "patched"
    for f in files:
        os.makedirs(os.path.dirname(work / f), exist_ok=True)
        with open(work / f, "w") as fo:
            fo.write(open(ref / f).read())
    r = subprocess.run(["git", "apply", "--check", "--verbose", patch], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    subprocess.check_call(["git", "apply", patch], cwd=work)
    sel = open(work / "src/sub/solver_selection.jl").read()
    assert "hip = hip_solver_def()," in sel
    design = open(work / "src/sub/design_mpc.jl").read()
    assert "AlmpcHIP.design_hip(" in design
    # both design methods branch to the GPU design: the linear-system one and the black-box one
    assert design.count("if mpc_solver isa hip_solver_def") == 2
    assert "AlmpcHIP.design_relin_fnn!(" in design and "AlmpcHIP.design_sqp_fnn!(" in design and "AlmpcHIP.fnn_linearize(" in design
    # results of a batched controller are allocated with the batch (a single-instance allocation would be overrun by the library)
    assert "_memory_allocation_initialization_results_hip(" in design and "(horizon + 1) * batch" in design
    # the shim travels with the patch, identical to julia/AlmpcHIP.jl
    shim = open(os.path.join(ROOT, "julia", "AlmpcHIP.jl")).read()
    assert open(work / "src/hip/AlmpcHIP.jl").read() == shim
    spec = importlib.util.spec_from_file_location("make_reference_patch", os.path.join(ROOT, "julia", "make_reference_patch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # (blob ids and the function names git puts after a hunk's line numbers come from lines the stand-in does not have)
    def hunks(text):
        return [re.sub(r"^(@@ [^@]* @@).*", r"\1", ln) for ln in text.splitlines() if not ln.startswith("index ")]
    assert hunks(mod.build(str(ref))) == hunks(patch_text), "julia/reference_hip.patch is stale: run python julia/make_reference_patch.py"
    # every ccall in the shim names a symbol the header declares
    import re
    hdr = open(os.path.join(ROOT, "include", "almpc.h")).read()
    for sym in set(re.findall(r"ccall\(\(:(almpc_[a-z_]+), libalmpc\)", shim)):
        assert re.search(r"\b" + sym + r"\s*\(", hdr), sym
    # the entry points that write through caller-supplied result pointers check the lengths first (a single-instance allocation with
    # mpc_batch > 1 must raise DimensionMismatch, not overrun the Julia heap)
    for fn in ("function calculate!(", "function read_results!(", "function results_wait!(", "function _model_predictive_control_computation(mod::HipModeler"):
        body = shim[shim.index(fn):]
        body = body[:body.index("\nend\n")]
        assert "check_result_sizes(mod, x, e_x, u, e_u)" in body, fn


def test_julia_shim_binds_every_entry_point_of_the_header():
    """julia/AlmpcHIP.jl is the binding a maintainer of the reference would add: every symbol include/almpc.h declares has a ccall
    there (the shim cannot be executed here -- no julia -- so at least its coverage of the ABI is checked)."""
    import re
    header = open(os.path.join(ROOT, "include", "almpc.h")).read()
    names = sorted(set(re.findall(r"\b(almpc_[a-z0-9_]+)\s*\(", header)))
    shim = open(os.path.join(ROOT, "julia", "AlmpcHIP.jl")).read()
    bound = set(re.findall(r"\(:(almpc_[a-z0-9_]+), libalmpc\)", shim))
    missing = [n for n in names if n not in bound]
    assert not missing, f"not bound in julia/AlmpcHIP.jl: {missing}"
    assert len(names) >= 45


def test_the_environment_is_read_in_one_place_and_the_switch_table_is_documented():
    """csrc/almpc_switches.h: read_switches() is the only code under csrc/ that calls getenv (a handle's switches are fixed by
    almpc_create; INTEGRATION.md, "Diagnostic switches"), and the table there lists exactly the names of the header's table."""
    import re
    csrc = os.path.join(ROOT, "automationlabsmodelpredictivecontrol.jl_amd", "csrc")
    hits = []
    for folder, _, files in os.walk(csrc):
        for name in files:
            for i, line in enumerate(open(os.path.join(folder, name), errors="replace"), 1):
                if "getenv" in line:
                    hits.append((os.path.relpath(os.path.join(folder, name), csrc), i))
    header = open(os.path.join(csrc, "almpc_switches.h")).read()
    reader = header[header.index("inline Switches read_switches()"):]
    reader = reader[:reader.index("\n}\n")]
    assert len(hits) == 1 and hits[0][0] == "almpc_switches.h" and reader.count("getenv") == 1, hits
    names = re.findall(r"^\s*X\((ALMPC_\w+), \w+, (?:ON_IF_1|ON_IF_SET|INTEGER), \"", header, re.M)
    assert len(names) == len(set(names)) == header.count(" X(ALMPC_") == 40
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    doc = doc[doc.index("## Diagnostic switches"):]
    doc = doc[:doc.index("\n## ", 5)]
    listed = re.findall(r"^\| `(ALMPC_\w+)` \|", doc, re.M)
    assert sorted(listed) == sorted(names)
