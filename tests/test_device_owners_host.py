"""The owners of device buffers, pinned buffers, events, streams and graphs (radiativetransfer_amd/csrc/ftte_device.h) on the
CPU: tests/host/device_owners_check.cpp compiles the header against a stub of the HIP runtime (tests/host/stub) and runs under
AddressSanitizer and UndefinedBehaviorSanitizer with leak detection.  It pins what is freed and when, that a moved-from owner is
empty, that reserve() keeps a buffer that is large enough and frees before it grows, that a failed allocation leaves neither a
pointer nor a capacity behind, and that the library's count of owned objects follows the stub's."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_device_owners_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "owners")
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(HOST, "stub"), "-I" + CSRC, os.path.join(HOST, "device_owners_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "device owners under the sanitizers: ok" in run.stdout and "ERROR" not in run.stderr
