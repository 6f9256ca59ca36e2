"""AddressSanitizer + UndefinedBehaviorSanitizer walk of the host side of time-varying designs on the stage-wise solvers
(almpc_design_ltv_stagewise, almpc_ltv_stagewise_update, almpc_get_ltv_stagewise_prepared) in the host form and the device form, every
refusal included: tests/sanitize/ltv_stagewise_driver.cpp, a stand-alone program against the fake HIP runtime, built exactly as
tests/test_sanitizers_sens_ltv.py builds its driver.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_sanitizers import SAN, _run


@pytest.mark.timeout(900)
def test_ltv_stagewise_entry_points_under_asan_ubsan(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not (os.path.exists(hipcc) and os.path.exists(clang)):
        pytest.skip("no ROCm toolchain here")
    src = os.path.join(ROOT, "automationlabsmodelpredictivecontrol.jl_amd", "csrc", "almpc_api.hip")
    api_o = str(tmp_path / "api.o")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fPIC", "--cuda-host-only", "-DALMPC_UNITY", "-Wno-unused-function",
                           "-Wno-cuda-compat"] + SAN + ["-c", "-o", api_o, src], stderr=subprocess.DEVNULL)
    # hip-clang's module constructor registers a fat binary that a host-only compile does not have: give the symbol a body
    und = subprocess.check_output(["nm", "-u", api_o], text=True)
    fat = [w for w in und.split() if w.startswith("__hip_fatbin_")]
    assert len(fat) == 1, fat
    (tmp_path / "fatbin.cpp").write_text('extern "C" { char %s[64] = {0}; }\n' % fat[0])
    objs = [api_o]
    for name, extra in (("fake_hip_runtime", ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]), ("ltv_stagewise_driver", []), ("fatbin", [])):
        d = str(tmp_path) if name == "fatbin" else os.path.join(ROOT, "tests", "sanitize")
        o = str(tmp_path / (name + ".o"))
        subprocess.check_call([clang, "-std=c++17"] + SAN + extra + ["-c", os.path.join(d, name + ".cpp"), "-o", o])
        objs.append(o)
    exe = str(tmp_path / "ltv_stagewise_san")
    subprocess.check_call([clang] + SAN + ["-o", exe] + objs + ["-lpthread", "-ldl"])
    r = _run([exe])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert "ltv stagewise host logic ok" in r.stdout
    assert int(r.stdout.split("ok:")[1].split()[0]) > 100   # the prepare, solver and finish launches were reached
