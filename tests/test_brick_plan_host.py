"""The uniform grid's planners (radiativetransfer_amd/csrc/ftte_planner.cpp: plan_bricks, plan_tiles) and the rules that resolve
the brick options (csrc/ftte_bricks.h: BrickOptions) on the CPU: tests/host/brick_plan_check.cpp compiles them with g++ against a
stub of the HIP runtime (tests/host/stub) and runs under AddressSanitizer and UndefinedBehaviorSanitizer with leak detection.
Direction sets of 24, 48 and 192 directions (groups of one, two and three), grids of 5, 64, 70, 128 and 130 cells a side, one to
eight frequency groups, every form of the sweep: every (group, brick) once and in the list of its stage and lane, the groups with
the most directions first, exactly the first visitor of an accumulator's brick stores, every dependency the right neighbour and
earlier in the list, merge points around the blocks' last writers, queues that hold whole dependency chains; the tile plan's items,
launches and accumulator slots; what the options resolve to; and the plans' FNV-1a-64 digests equal those of build_brick_plan and
build_plan before they were cut into steps."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_brick_and_tile_plans_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "brick_plan")
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I" + os.path.join(HOST, "stub"), "-I" + CSRC, os.path.join(HOST, "brick_plan_check.cpp"), os.path.join(CSRC, "ftte_planner.cpp"),
           os.path.join(CSRC, "ftte_amr.cpp"), os.path.join(CSRC, "ftte_geometry.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "brick and tile plans under the sanitizers: ok" in run.stdout and "ERROR" not in run.stderr
