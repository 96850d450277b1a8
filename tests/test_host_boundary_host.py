"""The owner of the host-array boundary (radiativetransfer_amd/csrc/ftte_host.h: the two pinned staging blocks with their events,
the registered ranges, the two staging loops) on the CPU: tests/host/host_boundary_check.cpp compiles the header against a stub of
the HIP runtime (tests/host/stub) and runs under AddressSanitizer and UndefinedBehaviorSanitizer with leak detection.  The stub
runs the laziest legal schedule -- an asynchronous copy is carried out when the host waits for it -- so a staging block that is
rewritten before the transfer out of it, or read before the transfer into it, delivers wrong bytes every time.  With blocks of
4096 bytes and sizes of 1, 4095, 4096, 4097, 8192, 8193 and 5 * 4096 + 17 bytes it pins: exact bytes in both directions and nothing
beyond them; two sends on two streams with no wait in between (two lanes); a send whose stream is never waited for, followed by a
send or a fetch on another stream (a sweep that returned an error behind a lane's upload: the upload() of before this owner took
both blocks for free at its start and would have refilled block 0 under the first transfer); a fetch directly after a send; the
outstanding flags, cleared by whoever waited; the ranges (both ends, the gap between two, a contained pin, a failed pin, an unknown
base, learn twice and forget once, the destructor unpinning exactly its own); a failed block allocation."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_host_boundary_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "boundary")
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I" + os.path.join(HOST, "stub"), "-I" + CSRC, os.path.join(HOST, "host_boundary_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "host boundary under the sanitizers: ok" in run.stdout and "ERROR" not in run.stderr
