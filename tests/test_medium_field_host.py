"""A field of the medium and the copies derived from it (radiativetransfer_amd/csrc/ftte_medium.h) on the CPU:
tests/host/medium_field_check.cpp compiles the header against a stub of the HIP runtime (tests/host/stub) and runs under
AddressSanitizer and UndefinedBehaviorSanitizer with leak detection.  It drives the type through the call sequences the library
performs -- the setters, the one-pass device setter that carries layouts along, the sweeps that make layouts, brick-order and
cell-major copies, the lanes of ftte_diffuse_iteration, growing buffers, failed allocations, another grid -- and pins after each
step which copies are current."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_medium_field_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "medium")
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(HOST, "stub"), "-I" + CSRC, os.path.join(HOST, "medium_field_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "medium field under the sanitizers: ok" in run.stdout and "ERROR" not in run.stderr
