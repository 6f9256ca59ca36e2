"""AddressSanitizer + UndefinedBehaviorSanitizer run of hm::c2d (csrc/almpc_host_math.h), the host restatement of k_c2d:
tests/sanitize/c2d_driver.cpp is a stand-alone program with its own main, compiled with the sanitizers and run as a program."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_sanitizers import SAN, _run


@pytest.mark.timeout(300)
def test_host_c2d_under_asan_ubsan(tmp_path):
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("no ROCm toolchain here")
    exe = str(tmp_path / "c2d_san")
    subprocess.check_call([clang, "-std=c++17"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "sanitize", "c2d_driver.cpp")])
    r = _run([exe])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert "c2d host math ok: 81" in r.stdout
