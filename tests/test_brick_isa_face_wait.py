"""Where the whole-brick form of the brick sweep (brick_kernel<4, 0, 0, false, true>) waits for the rays from the brick below
(csrc/ftte_brick.hip, brick_step: row 0 takes that ray at the end of a shape step).  The load then has the step's arithmetic to
arrive, and what is left of `vmcnt(0)` in the layer loop stands at the end of a step, never in front of the LDS swap of the rays or
a register copy.  CPU only: it compiles, it runs nothing (tools/brick_isa.py prints the whole report)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not found")


@pytest.fixture(scope="module")
def rep():
    import brick_isa
    asm = brick_isa.compile_asm(os.path.join(ROOT, "radiativetransfer_amd", "csrc", "ftte_brick.hip"))
    return brick_isa.report(asm, brick_isa.find_kernel(asm, None))


def drains(rep):
    return [w for w in rep["loop_waits"] if "vmcnt(0)" in w["text"] or w["text"] == "s_waitcnt 0"]


def test_it_is_the_bench_instance_within_its_registers(rep):
    assert rep["kernel"] == "_ZN4ftte12brick_kernelILi4ELi0ELi0ELb0ELb1EEEvNS_11BrickLaunchE"
    assert rep["vgpr"] + rep["agpr"] <= 128 and rep["vgpr_spill"] == 0 and rep["scratch"] == 0, rep


def test_at_most_one_drain_per_v_shape_step(rep):
    """Three v-shapes, two layers in the loop: six steps that wait for a face, each once.  (Twelve: the bound with a second,
    branch-free copy of every step.)"""
    print("vmcnt(0) in the layer loop:", [(w["block"], w["before"]) for w in drains(rep)])
    assert rep["layer_loop"] is not None and rep["loop_instructions"] > 1000, rep["layer_loop"]
    assert len(drains(rep)) <= 12, [(w["block"], w["before"]) for w in drains(rep)]


def test_no_drain_holds_back_the_swap_of_the_rays_or_a_copy(rep):
    bad = [w for w in drains(rep) if w["before"].startswith(("ds_write", "v_mov_b64"))]
    assert not bad, bad
