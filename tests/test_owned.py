"""CPU: the owners of the host layer's device resources (facedeform_amd/csrc/fd_owned.h) on their own, under the address and
undefined-behaviour sanitizers.  tests/tools/owned_check.cpp includes that header as shipped over a fake of the few runtime calls
it uses (tests/tools/owned_fake/hip/hip_runtime.h: malloc, counters, a log of the calls, a switch that makes the n-th allocation
or creation fail) and checks the grow rule, the lazily created event and that every resource is released exactly once.  The GPU
test of the same paths through the library is test_gpu_scratch_regrow.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "facedeform_amd", "csrc")
TOOLS = os.path.join(ROOT, "tests", "tools")


def test_owners_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    out = str(tmp_path / "owned_check")
    # as test_fit_host.py builds its program: the sanitizers' runtimes linked statically.  The fake's directory comes first, so
    # that <hip/hip_runtime.h> is the fake wherever a real one is installed.
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", os.path.join(TOOLS, "owned_fake"), "-I", CSRC,
                        os.path.join(TOOLS, "owned_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
