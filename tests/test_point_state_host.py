"""The owners of the point-source path (radiativetransfer_amd/csrc/ftte_point.h), the tree on the device (ftte_device_tree.h) and
the tracer's host-only steps on the CPU: tests/host/point_state_check.cpp compiles ftte_point.cpp and the table mathematics it calls
against a stub of the HIP runtime (tests/host/stub), with stand-ins for the kernels, and runs under AddressSanitizer and
UndefinedBehaviorSanitizer with leak detection.  It drives the rate tables (current set, slots that grow and shrink, the memory
pre-check, a failed allocation, the output cross-sections' two rules), the accumulated rates, the device tree on a uniform and a
refined 2^3 grid, the check of a call's stars, the scratch, the ray counts, the escape record, and a trace that finds everything
prepared: that one allocates nothing and copies what it copied before."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_point_state_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "point")
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(HOST, "stub"), "-I" + CSRC, os.path.join(HOST, "point_state_check.cpp")]
    cmd += [os.path.join(CSRC, s) for s in ("ftte_point.cpp", "ftte_tables.cpp", "ftte_amr.cpp", "ftte_geometry.cpp")] + ["-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "point state under the sanitizers: ok" in run.stdout and "ERROR" not in run.stderr


def test_table_mathematics_compiles_without_hip(tmp_path):
    """ftte_tables.cpp is plain C++: it compiles with nothing but the stub's directory beside the sources, warnings as errors."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    cmd = [gxx, "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(HOST, "stub"), "-I" + CSRC, "-c", os.path.join(CSRC, "ftte_tables.cpp"),
           "-o", str(tmp_path / "tables.o")]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    for name in ("ftte_tables.cpp", "ftte_tables.h"):
        assert "#include <hip" not in open(os.path.join(CSRC, name)).read(), name
