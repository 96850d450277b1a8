"""The gfx950 code of the benchmarked brick sweep (brick_kernel<4, 0, 0, false, true>), as the compiler makes it: its register
budget, and no drain of the memory queue at the places of the layer loop where the whole-brick form removed them
(tools/brick_isa.py prints the whole report).  CPU only: it compiles, it runs nothing."""
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


def test_bench_instance_keeps_four_waves_per_simd(rep):
    assert rep["kernel"] == "_ZN4ftte12brick_kernelILi4ELi0ELi0ELb0ELb1EEEvNS_11BrickLaunchE"
    assert rep["vgpr"] + rep["agpr"] <= 128, rep
    assert rep["scratch"] == 0 and rep["vgpr_spill"] == 0, rep
    assert rep["lds_static"] == 0, rep


def test_layer_loop_does_not_drain_at_its_header_or_its_copies(rep):
    """No wait on vmcnt at the loop header (the prologue's loads are retired before it), and no vmcnt(0) in front of a
    register copy or an LDS write of the rays (the opacity hand-over and the direction swap of the parent's loop)."""
    assert rep["layer_loop"] is not None and rep["loop_instructions"] > 1000, rep["layer_loop"]
    header = [w["text"] for w in rep["loop_waits"] if w["header"] and "vmcnt" in w["text"]]
    assert not header, header
    drains = [w for w in rep["loop_waits"] if "vmcnt(0)" in w["text"]]
    bad = [w for w in drains if w["before"].startswith(("ds_write", "v_mov_b64"))]
    assert not bad, bad


def test_layer_loop_drains_no_more_than_the_v_face_loads_need(rep):
    """The drains left in the loop wait for a brick's rays from below, the youngest load when a shape step needs it: at most
    eleven per layer (the loop holds two layers)."""
    drains = [w for w in rep["loop_waits"] if "vmcnt(0)" in w["text"]]
    assert len(drains) <= 22, [(w["block"], w["before"]) for w in drains]
