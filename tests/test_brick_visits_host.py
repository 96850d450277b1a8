"""Two passes of an izone per visit, on the CPU (radiativetransfer_amd/csrc/ftte_planner.cpp: link_visits, seat_stage_lists;
csrc/ftte_bricks.h: BrickKey::duo, BrickOptions::visits): tests/host/brick_visits_check.cpp compiles the planner with g++ against a
stub of the HIP runtime (tests/host/stub) and runs under AddressSanitizer and UndefinedBehaviorSanitizer with leak detection.
Direction sets of 24, 48 and 192 directions and the benchmark's 96, grids of 64 and 128 cells a side, 8 frequency groups: every
(pass, brick) once, linked seats two passes of one izone on one brick in one stage, helpers that never store or accumulate,
exactly the first visitor of an accumulator's brick stores, upstream neighbours a stage earlier, merge points behind the last
writers, 36 -> 23 and 72 -> 46 visits, the LDS of a workgroup, and the digests of a key without the new member."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_brick_visits_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "brick_visits")
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I" + os.path.join(HOST, "stub"), "-I" + CSRC, os.path.join(HOST, "brick_visits_check.cpp"), os.path.join(CSRC, "ftte_planner.cpp"),
           os.path.join(CSRC, "ftte_amr.cpp"), os.path.join(CSRC, "ftte_geometry.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "brick visits under the sanitizers: ok" in run.stdout and "ERROR" not in run.stderr
