"""How a stage launch of the brick sweep deals its workgroups to (brick, frequency group) pairs (brick_deal,
radiativetransfer_amd/csrc/ftte_brick_rec.h: the function the kernels call), on the CPU: tests/host/brick_deal_check.cpp under
AddressSanitizer and UndefinedBehaviorSanitizer.  For 1..16 frequency groups, run lengths 0, 1, 4 and 16 and 1..1000 tasks: every
pair is swept exactly once; for a run length >= 1 the workgroups of one class `work % 8` (one XCD under round-robin placement)
sweep every group equally often to within the run length; run length 0 is group = work % nnu."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_brick_deal_is_a_bijection_and_levels_the_xcds(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "deal")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + CSRC, "-I" + os.path.join(HOST, "stub"), os.path.join(HOST, "brick_deal_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "brick deal: ok" in run.stdout and "ERROR" not in run.stderr
