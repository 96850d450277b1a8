#!/usr/bin/env python3
"""The star catalogue's launches on one GPU: 10^6 uniformly random stars on the 256^3 uniform grid and on BASELINE's 128^3 grid
with its refined 32^3 patch (2 326 528 leaves), device time per launch from the events the library records around them
(ftte_counter "catalogue_ns_locate" / "_count" / "_scan" / "_emit"), the whole call on the host clock, and beside them the only
route the parent commit has: a host loop over ftte_locate_cell for the same stars (their call sequences computed beforehand, which
that route also needs and is not charged for).

usage: bench_catalogue.py [--stars N] [--reps R] [--loop-stars M]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import radiativetransfer_amd as rt  # noqa: E402
from radiativetransfer_amd import synthetic  # noqa: E402


def flag(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def run(title, st, n, level, xyz, reps, loop_stars):
    st.set_grid(n, level, 3.0e22)
    nc = len(level)
    phases = ("locate", "count", "scan", "emit")
    for _ in range(3):                                                    # warm-up: code objects, buffers, the tree on the device
        cat = st.star_catalogue(xyz)
    times, calls = {p: [] for p in phases}, []
    for _ in range(reps):
        t0 = time.perf_counter()
        cat = st.star_catalogue(xyz)
        calls.append((time.perf_counter() - t0) * 1e3)
        for p in phases:
            times[p].append(st.counter("catalogue_ns_" + p) * 1e-6)
    ns, nsrc = len(xyz), len(cat["cell"])
    print(f"{title}: {nc} leaves, {ns} stars, {nsrc} sources, {cat['outside']} outside")
    for p in phases:
        a = np.array(times[p])
        print(f"  {p:7s} {np.median(a):9.4f} ms  (min {a.min():.4f}, max {a.max():.4f}, {reps} repetitions)")
    dev = sum(np.median(times[p]) for p in phases)
    a = np.array(calls)
    print(f"  device, four launches {dev:.4f} ms = {dev * 1e6 / ns:.2f} ns per star; whole call with both copies "
          f"{np.median(a):.2f} ms (min {a.min():.2f}, max {a.max():.2f})")
    locate = np.median(times["locate"])
    print(f"  locate: {32 * ns / locate * 1e-6:.2f} GB/s of star data (24 B in, 8 B out); count + emit read {8 * nc * 1e-6:.1f} MB of counts")
    # what bounds the locate: the same stars with weight 0 take the same loads and issue no atomic
    zero = np.zeros(ns, np.int32)
    bare = []
    for _ in range(3 + reps):
        st.star_catalogue(xyz, weight=zero)
        bare.append(st.counter("catalogue_ns_locate") * 1e-6)
    a = np.array(bare[3:])
    print(f"  locate with every weight 0 (no atomics) {np.median(a):.4f} ms (min {a.min():.4f}, max {a.max():.4f}): "
          f"the two atomics per star cost {locate - np.median(a):.4f} ms = {2 * ns / max(locate - np.median(a), 1e-9) * 1e3:.3e} atomics/s")
    cat = st.star_catalogue(xyz)
    # the parent commit's route: one ftte_locate_cell per star on the host
    m = min(loop_stars, ns)
    seqs = [st.cell_position(int(c)) for c in cat["star_cell"][:m] if c >= 0]
    t0 = time.perf_counter()
    cells = [st.locate_cell(s) for s in seqs]
    dt = time.perf_counter() - t0
    assert cells == [int(c) for c in cat["star_cell"][:m] if c >= 0]
    print(f"  host loop over ftte_locate_cell: {dt / len(seqs) * 1e9:.0f} ns per star ({len(seqs)} stars, through the Python binding)")


def main():
    ns, reps, loop_stars = flag("--stars", 1000000), flag("--reps", 20), flag("--loop-stars", 100000)
    rng = np.random.default_rng(746)
    xyz = rng.uniform(0, 1, (ns, 3))
    with rt.StellarTransfer(device=0) as st:
        run("256^3 uniform", st, 256, np.zeros(256 ** 3, np.int32), xyz, reps, loop_stars)
        n = 128
        q = n // 4
        blocks = [(n // 2 - q // 2 + a, n // 2 - q // 2 + b, n // 2 - q // 2 + c) for a in range(q) for b in range(q) for c in range(q)]
        run("128^3 + refined 32^3 patch", st, n, synthetic.refine_levels(n, blocks, depth=1), xyz, reps, loop_stars)


if __name__ == "__main__":
    main()
