"""The host side of the sweeps of a refined cell array (radiativetransfer_amd/csrc/ftte_sweeps.cpp: forest_sweep, prepare_forests,
the batches, passes and fused levels; csrc/ftte_hybrid.cpp: hybrid_sweep, its buffers, pipelines and face blocks; with the planners,
the owners and the host-array copies they call) on the CPU, against a checked model of the device: tests/host/refined_sweep_check.cpp
links them with g++ against a stub of the HIP runtime (tests/host/stub) and host definitions of the launches they reach
(tests/host/device_model.cpp: serial loops with the kernels' own addressing for the forests and the medium copies, an oracle brick
for launch_brick that requires every face element a brick takes to hold, bit for bit, the value of an independent evaluation of
the whole tree), and runs under AddressSanitizer and UndefinedBehaviorSanitizer with leak detection: "device" memory is malloc
there, so every index the host hands to the device is a checked access.  Seven trees (the two corner patches of
test_refined_cells_on_the_domain_boundary scaled down to n = 64, a patch against one face and its mirror image, and the ragged,
diagonal -- by slot and by phase -- and fully refined trees of hybrid_plan_check.cpp), one direction per izone, one context per tree,
face block and scratch poisoned before every sweep: the device test's own order of calls, 1, 2 and 4 pipelines, batches shorter
than the direction list, every level its own launch and whole passes fused, little free memory and a failed scratch allocation;
two frequency groups, the first corner tree with one and three as well, and with both emission forms; J against the oracle
(one direction bit for bit, several to 64 eps) and the forests' tables property by property after every sweep; three seeded faults
(an export moved by one element, an upstream segment of a later depth, a brick task left out) that the comparisons must see.
The fully refined tree has twice the leaves of any other and ran twice as long: it goes through every sequence with one group and
through the first with two.  The twelve jobs run in processes of their own, as many at a time as there are processors, the three
runs with a seeded fault left in beside them: 1 min 55 s of wall time for the program on eight processors (12 min of processor
time), 2 min 47 s for this test with its build."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


def test_refined_sweeps_against_the_device_model_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "refined_sweep")
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
             "-I" + os.path.join(HOST, "stub"), "-I" + CSRC]
    sources = [os.path.join(HOST, "refined_sweep_check.cpp"), os.path.join(HOST, "device_model.cpp")]
    sources += [os.path.join(CSRC, name) for name in ("ftte_sweeps.cpp", "ftte_hybrid.cpp", "ftte_plan.cpp", "ftte_host_arrays.cpp", "ftte_planner.cpp",
                                                      "ftte_amr.cpp", "ftte_geometry.cpp")]
    # (nine translation units, the planner's the longest: compiled side by side, then linked)
    objects = [str(tmp_path / (os.path.basename(src)[:-4] + ".o")) for src in sources]
    compiles = [subprocess.Popen([gxx] + flags + ["-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for src, obj in zip(sources, objects)]
    stderr = ""
    failed = False
    for child in compiles:
        stderr += child.communicate(timeout=900)[1]
        failed = failed or child.returncode != 0
    if not failed:
        build = subprocess.run([gxx] + flags + objects + ["-o", exe], capture_output=True, text=True, timeout=900)
        stderr += build.stderr
        failed = build.returncode != 0
    if failed and ("asan" in stderr or "ubsan" in stderr) and "cannot find" in stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert not failed, stderr[-3000:]
    # each seeded fault left in, beside the sweeps: the program's own comparison ends it, no sanitizer does
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    seeded = [subprocess.Popen([exe, "fault", str(k)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for k in (1, 2, 3)]
    try:
        run = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
        last = run.stdout.strip().splitlines()[-1]
        assert last.startswith("refined sweeps against the device model: ok:") and "ERROR" not in run.stderr
        # every tree with every sequence, the first corner tree with one and three groups, the seeded faults, both emission forms
        for tree in ("corner 0", "corner n - 3", "face 0", "face n - 3", "ragged two levels n = 72", "diagonal slots", "diagonal phases"):
            for seq in "abcde":
                assert "[%s nnu 2 (%s)]" % (tree, seq) in last, (tree, seq)
        for seq in "abcde":  # (twice the leaves of any other tree: every sequence with one group, the first with two)
            assert "[refined 32^3 cube nnu 1 (%s)]" % seq in last, seq
        assert "[refined 32^3 cube nnu 2 (a)]" in last
        for nnu in (1, 3):
            for seq in "abcde":
                assert "[corner 0 nnu %d (%s)]" % (nnu, seq) in last
        for extra in ("seeded faults", "source", "eta"):
            assert "[corner 0 nnu 2 %s]" % extra in last
        for k in (1, 2, 3):
            assert "seeded fault %d" % k in run.stdout
        for k, child in zip((1, 2, 3), seeded):
            out, err = child.communicate(timeout=900)
            assert child.returncode == 1 and "a seeded fault" in err and "ERROR" in err, (k, out[-2000:], err[-2000:])
            assert "Sanitizer" not in err and "runtime error" not in err and "went unseen" not in out, (k, err[-2000:])
    finally:
        for child in seeded:
            if child.poll() is None:
                child.kill()
                child.communicate()
