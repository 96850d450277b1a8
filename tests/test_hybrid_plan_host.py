"""The hybrid sweep's planner (radiativetransfer_amd/csrc/ftte_planner.cpp) and the owners of the refined-grid sweeps
(csrc/ftte_forests.h, csrc/ftte_hybrid.h) on the CPU: tests/host/hybrid_plan_check.cpp compiles them with g++ against a stub of the
HIP runtime (tests/host/stub) and runs under AddressSanitizer and UndefinedBehaviorSanitizer with leak detection.  Four trees (a
one-level patch and a ragged two-level one, the smallest grids on which a brick leaves lanes outside a box; a fully refined cube
that gets bricks of its own; three patches on the diagonal in slot and in phase form), one direction per izone: the bricks cover
every base cell outside a group's boxes once and none inside, the forests' leaf list and activity bytes cover the rest, pieces
come after what they take rays from and around the forest passes as pass_at says, exactly the first visitor of an accumulator's
brick stores, the fine block's lists, what a failed scratch allocation leaves, what drop_grid releases, what the graph signature
covers; and the plans' FNV-1a-64 digests equal those of the planner before it was split into steps."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_hybrid_plan_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "hybrid_plan")
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I" + os.path.join(HOST, "stub"), "-I" + CSRC, os.path.join(HOST, "hybrid_plan_check.cpp"), os.path.join(CSRC, "ftte_planner.cpp"),
           os.path.join(CSRC, "ftte_amr.cpp"), os.path.join(CSRC, "ftte_geometry.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "hybrid plan under the sanitizers: ok" in run.stdout and "ERROR" not in run.stderr
