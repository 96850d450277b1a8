"""Where the brick sweep's layer loop waits: the gfx950 code of one brick_kernel instance, from the compiler.

    python tools/brick_isa.py [--source FILE] [--kernel NAME] [--json]
    python tools/brick_isa.py [--source FILE] --compare OTHER.s

--compare: is the device code of FILE (a .hip unit, or assembly kept as .s; several units' assembly may stand in one file) the
same, kernel by kernel, as that of OTHER.s?  Exit status 1 if anything differs.

Compiles csrc/ftte_brick.hip (or FILE) with the library's FLAGS (radiativetransfer_amd/build.py) to gfx950 assembly, finds the
instance `bench.py` runs (launch_brick: brick_kernel<4, 0, 0, false, true>, or brick_kernel<4, 0, 0, false> in a tree that
has no whole-brick form) and prints its VGPRs, SGPR and VGPR spills, scratch and LDS, and every s_waitcnt inside its layer
loop.  The layer loop is the outermost loop of the instance with the most instructions; blocks belong to a loop by the
compiler's own loop comments (`Loop Header`, `in Loop: Header=`, `Parent Loop`).

vmcnt counts loads and stores together, in issue order: a `vmcnt(0)` inside the loop retires everything the wavefront still
has outstanding, the next layer's opacities and the J stores included.  tests/test_brick_isa.py keeps it out of the loop.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from radiativetransfer_amd import build  # noqa: E402  (FLAGS and hipcc only: nothing is built)

# the instance bench.py runs, and its name before the whole-brick form existed
BENCH = ["_ZN4ftte12brick_kernelILi4ELi0ELi0ELb0ELb1EEEvNS_11BrickLaunchE", "_ZN4ftte12brick_kernelILi4ELi0ELi0ELb0EEEvNS_11BrickLaunchE"]
PAIR = "_ZN4ftte17brick_pair_kernelILi4ELi0EEEvNS_11BrickLaunchEi"


def compile_asm(source: str) -> str:
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "brick.s")
        cmd = [build.hipcc(), *build.FLAGS, "-x", "hip", "--cuda-device-only", "-S", source, "-o", out]
        subprocess.run(cmd, check=True, capture_output=True, text=True)
        return open(out).read()


def compare(asm: str, other: str) -> list[str]:
    """What differs between two assemblies, kernel by kernel: the names, each body from its label to its .Lfunc_end without comment,
    debug and .loc lines and without the function number in local labels (.LBB12_3 -> .LBB_3), and each metadata record.  Either
    side may be several units' assembly one after the other.  Text only: no instruction is looked for."""
    def kernels(text):
        out = {}
        for name in re.findall(r"\.symbol:\s+(\S+)\.kd", text):
            start = text.index("\n" + name + ":")
            body = text[start:text.index(".Lfunc_end", start)].split("\n")
            body = [re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", ln.split(";")[0].rstrip()) for ln in body
                    if not re.match(r"^\s*(;|\.loc\s|\.file\s|\.Ltmp|\.cfi_|$)", ln)]
            out[name] = ("\n".join(body), metadata(text, name))
        return out
    a, b = kernels(asm), kernels(other)
    diffs = [f"only here: {n}" for n in sorted(set(a) - set(b))] + [f"only there: {n}" for n in sorted(set(b) - set(a))]
    for n in sorted(set(a) & set(b)):
        if a[n][0] != b[n][0]:
            diffs.append(f"body differs: {n}")
        if a[n][1] != b[n][1]:
            diffs.append(f"metadata differs: {n}: {a[n][1]} / {b[n][1]}")
    print(f"{len(a)} kernels here, {len(b)} there, {len(set(a) & set(b))} in both: {len(diffs)} differ")
    return diffs


def metadata(asm: str, name: str) -> dict:
    """The code object's record of the kernel (.amdgpu_metadata)."""
    m = re.search(r"\.name:\s+" + re.escape(name) + r"\n(.*?)(?:\n  - |\n\.end_amdgpu_metadata)", asm, re.S)
    start = asm.rfind("\n  - ", 0, m.start()) if m else -1
    if not m or start < 0:
        raise KeyError(name)
    rec = asm[start:m.end()]
    num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", rec).group(1))  # noqa: E731
    return {"vgpr": num("vgpr_count"), "agpr": num("agpr_count"), "sgpr": num("sgpr_count"), "sgpr_spill": num("sgpr_spill_count"),
            "vgpr_spill": num("vgpr_spill_count"), "scratch": num("private_segment_fixed_size"), "lds_static": num("group_segment_fixed_size")}


def blocks(body: list[str], depth: dict):
    """(label, loops the block is in, first line, instructions) per basic block; depth: loop header -> its depth."""
    out, cur = [], None
    for k, line in enumerate(body):
        lab = re.match(r"^(\.LBB\w+|; %bb\.\d+):(.*)$", line)
        if lab:
            cur = [re.sub(r"^\.L", "", lab.group(1)).replace("; %bb.", "bb."), set(), k, []]
            out.append(cur)
            comment = lab.group(2)
            j = k + 1
            while j < len(body) and re.match(r"^\s+;", body[j]):  # continuation lines of the block comment
                comment += body[j]
                j += 1
            cur[1].update(re.findall(r"(?:Header=|Parent Loop )(BB\w+)", comment))
            head = re.search(r"Loop Header: Depth=(\d+)", comment)
            if head:
                cur[1].add(cur[0])
                depth[cur[0]] = int(head.group(1))
            continue
        if cur is not None and re.match(r"^\s+[a-z_][\w.]*", line) and not re.match(r"^\s+\.", line):
            cur[3].append((k, line.strip()))
    return out


def report(asm: str, name: str) -> dict:
    start = asm.index("\n" + name + ":")
    end = asm.index(".Lfunc_end", start)
    body = asm[start:end].split("\n")
    depth = {}
    bl = blocks(body, depth)
    # the outermost loops and their size in instructions
    size = {h: sum(len(b[3]) for b in bl if h in b[1]) for h, d in depth.items() if d == 1}
    loop = max(size, key=lambda h: size[h]) if size else None
    waits = []
    for b in bl:
        for k, ins in b[3]:
            if ins.startswith("s_waitcnt"):
                nxt = next((x for _, x in b[3] if _ > k and not x.startswith(("s_", ";"))), "")  # the vector instruction it holds back
                waits.append({"line": k, "block": b[0], "in_loop": loop in b[1], "header": b[0] == loop, "text": ins.split(";")[0].strip(),
                              "before": nxt.split()[0] if nxt else ""})
    in_loop = [w for w in waits if w["in_loop"]]
    drains = [w for w in in_loop if re.search(r"vmcnt\(0\)", w["text"]) or w["text"] == "s_waitcnt 0"]
    return {"kernel": name, **metadata(asm, name), "layer_loop": loop, "loop_instructions": size.get(loop, 0),
            "instructions": sum(len(b[3]) for b in bl), "loop_waits": in_loop, "loop_vmcnt0": len(drains),
            "waits_outside_loop": [w["text"] for w in waits if not w["in_loop"] and "vmcnt" in w["text"]]}


def find_kernel(asm: str, wanted: str | None) -> str:
    names = re.findall(r"^(_Z\w+):", asm, re.M)
    for cand in ([wanted] if wanted else BENCH):
        if cand in names:
            return cand
    raise SystemExit(f"kernel {wanted or BENCH[0]} not in the assembly; instances: {names}")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--source", default=os.path.join(build.CSRC, "ftte_brick.hip"))
    ap.add_argument("--kernel", default=None, help=f"mangled name (default: the bench instance; the pair kernel: {PAIR})")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--compare", metavar="OTHER.s", default=None, help="compare every kernel's text and metadata with this assembly")
    a = ap.parse_args()
    asm = open(a.source).read() if a.source.endswith(".s") else compile_asm(os.path.abspath(a.source))
    if a.compare:
        diffs = compare(asm, open(a.compare).read())
        print("\n".join(diffs), end="\n" if diffs else "")
        return 1 if diffs else 0
    rec = report(asm, find_kernel(asm, a.kernel))
    if a.json:
        print(json.dumps(rec, indent=1))
        return 0
    print(f"kernel            {rec['kernel']}")
    print(f"VGPRs             {rec['vgpr']} (AGPRs {rec['agpr']}); SGPRs {rec['sgpr']}, {rec['sgpr_spill']} spilled to VGPR lanes; "
          f"VGPR spills {rec['vgpr_spill']}; scratch {rec['scratch']} B; static LDS {rec['lds_static']} B")
    print(f"instructions      {rec['instructions']}, of which {rec['loop_instructions']} in the layer loop (header {rec['layer_loop']})")
    print(f"waits in the layer loop: {len(rec['loop_waits'])}, vmcnt(0): {rec['loop_vmcnt0']}")
    for w in rec["loop_waits"]:
        print(f"  {w['line']:6d}  {w['block']:12s} {w['text']:28s} before {w['before']}")
    print(f"vmcnt waits outside the loop: {', '.join(rec['waits_outside_loop']) or 'none'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
