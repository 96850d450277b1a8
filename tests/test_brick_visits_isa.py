"""The gfx950 code of the two-wavefront brick sweep (brick_duo_kernel, csrc/ftte_brick.hip), as the compiler makes it: the
register budget of four wavefronts per SIMD, and a layer loop whose waits on the memory queue are those of the single-wavefront
form -- none at the loop header, no drain in front of a barrier, an LDS write or a register copy, and no more drains than that
form is held to (tools/brick_isa.py --kernel prints the whole report).  Waits and registers only.  CPU only: it compiles, it runs
nothing."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not found")

DUO = "_ZN4ftte16brick_duo_kernelENS_11BrickLaunchEi"


@pytest.fixture(scope="module")
def built():
    import brick_isa
    asm = brick_isa.compile_asm(os.path.join(ROOT, "radiativetransfer_amd", "csrc", "ftte_brick.hip"))
    return asm, brick_isa.report(asm, brick_isa.find_kernel(asm, DUO))


def test_four_waves_per_simd_and_nothing_spilled(built):
    rep = built[1]
    assert rep["kernel"] == DUO
    assert rep["vgpr"] + rep["agpr"] <= 128, rep
    assert rep["scratch"] == 0 and rep["vgpr_spill"] == 0, rep
    assert rep["lds_static"] == 0, rep


def test_layer_loop_does_not_wait_at_its_header(built):
    rep = built[1]
    assert rep["layer_loop"] is not None and rep["loop_instructions"] > 1000, rep["layer_loop"]
    header = [w["text"] for w in rep["loop_waits"] if w["header"] and "vmcnt" in w["text"]]
    assert not header, header


def test_no_drain_in_front_of_a_barrier_an_lds_write_or_a_copy(built):
    """The instruction a vmcnt(0) of the layer loop holds back -- scalar instructions and the markers of an inline asm skipped, the
    barrier itself not -- is no s_barrier, ds_write or v_mov_b64; and the loop does hold the barriers."""
    asm, rep = built
    start = asm.index("\n" + DUO + ":")
    body = asm[start:asm.index(".Lfunc_end", start)].split("\n")
    drains = [w for w in rep["loop_waits"] if "vmcnt(0)" in w["text"] or w["text"] == "s_waitcnt 0"]
    bad = []
    for w in drains:
        for line in body[w["line"] + 1:]:
            ins = line.strip()
            if not ins or ins.startswith(";") or re.match(r"^\.?\w+:", ins):
                continue
            if ins.startswith("s_") and not ins.startswith("s_barrier"):
                continue
            if ins.startswith(("s_barrier", "ds_write", "v_mov_b64")):
                bad.append((w["block"], ins))
            break
    assert not bad, bad
    assert sum(1 for line in body if line.strip().startswith("s_barrier")) == 4  # two per layer, two layers in the loop


def test_layer_loop_drains_no_more_than_the_single_wavefront_form_may(built):
    rep = built[1]
    assert rep["loop_vmcnt0"] <= 12, [(w["block"], w["before"]) for w in rep["loop_waits"] if "vmcnt(0)" in w["text"]]
