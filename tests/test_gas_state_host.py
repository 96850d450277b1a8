"""The species medium, the chemistry's buffers and the rate-table sets (radiativetransfer_amd/csrc/ftte_gas.h, TableSets of
ftte_point.h) on the CPU: tests/host/gas_state_check.cpp compiles the headers against a stub of the HIP runtime (tests/host/stub)
and runs under AddressSanitizer and UndefinedBehaviorSanitizer with leak detection.  It drives the types through the call sequences
the library performs -- ftte_set_medium with and without a density, traces that pack the medium, an update that commits new species,
another cell count, failed allocations, another grid, table sets that grow and shrink -- and pins after each step whether the gas is
ready, ready with a density, and whether the tracer's packed copy is current."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_gas_state_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "gas")
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(HOST, "stub"), "-I" + CSRC, os.path.join(HOST, "gas_state_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "gas state under the sanitizers: ok" in run.stdout and "ERROR" not in run.stderr
