"""The host side of the per-leaf updates (radiativetransfer_amd/csrc/ftte_leaf_pass.cpp: leaf_pass and the entry points of the
ionisation equilibrium, its advance, the start-up equilibrium, the thermal balance, the temperature step and the coupled step) on the
CPU, against a checked model of the device: tests/host/leaf_pass_check.cpp links that translation unit with g++ against a stub of the
HIP runtime (tests/host/stub) and host definitions of the seven launches it reaches -- serial loops over the cells' own statements,
reading and writing through the launch record as the kernels do -- and runs under AddressSanitizer and UndefinedBehaviorSanitizer with
leak detection: "device" memory is malloc there, so every pointer and offset the pass hands to the device is a checked access.  One
tree of 71 leaves; every family in every rate mode bit for bit against a loop of the program's own; refusals with one and with two bad
leaves, bad arguments in front of every allocation and copy, missing preconditions in their order, every allocation of a coupled call
failing in turn; two seeded faults that the comparisons must see."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_leaf_pass_against_the_device_model_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "leaf_pass")
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-pthread", "-I" + os.path.join(HOST, "stub"), "-I" + CSRC, os.path.join(HOST, "leaf_pass_check.cpp"),
           os.path.join(CSRC, "ftte_leaf_pass.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if build.returncode and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.strip().splitlines()[-1] == "leaf pass against the device model: ok" and "ERROR" not in run.stderr
    # each seeded fault left in: the program's own comparison ends it, no sanitizer does
    for k in (1, 2):
        seeded = subprocess.run([exe, "fault", str(k)], capture_output=True, text=True, timeout=600, env=env)
        assert seeded.returncode == 1 and "a seeded fault" in seeded.stderr and "ERROR" in seeded.stderr, (k, seeded.stdout[-2000:], seeded.stderr[-2000:])
        assert "Sanitizer" not in seeded.stderr and "runtime error" not in seeded.stderr and "went unseen" not in seeded.stdout, (k, seeded.stderr[-2000:])
