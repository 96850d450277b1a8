"""The host side of the brick sweeps (radiativetransfer_amd/csrc/ftte_bricks.h) on the CPU: tests/host/brick_tables_check.cpp
compiles the header against a stub of the HIP runtime (tests/host/stub) and runs under AddressSanitizer and
UndefinedBehaviorSanitizer with leak detection.  It pins which plan a set of device tables holds (by the plan's id: another plan
in the same tables displaces the first, which copies again when it comes back; a failed allocation leaves nothing held and leaks
nothing), when a Sent buffer copies (identical bytes once, a changed byte again, a grown or reset buffer again), the launch record
of brick_launch against a field-by-field fill with literal numbers (a task range, a frequency range, the hybrid sweep's strides,
the fine block's caller), the order and count of a merge's accumulators, and that the lanes' frequency slices tile the groups."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_brick_tables_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "bricks")
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(HOST, "stub"), "-I" + CSRC, os.path.join(HOST, "brick_tables_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "brick tables under the sanitizers: ok" in run.stdout and "ERROR" not in run.stderr
