#!/usr/bin/env python3
"""The brick plan's merge points for bench.py's workload (256^3, 8 frequency groups, 96 directions): after which stage each merge
point runs and how many merge blocks (32^3 cells) are final by then -- the measured counterpart of a geometric estimate.  One sweep on
the GPU builds the plan.  Prints one JSON line.  usage: merge_points.py [n] [ndir]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import radiativetransfer_amd as rt  # noqa: E402
from radiativetransfer_amd import synthetic  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
ndir = int(sys.argv[2]) if len(sys.argv) > 2 else 96
nnu = 8
nside = 1
while 12 * nside * nside < ndir:
    nside *= 2
ang = np.array([rt.pix2ang_nest(nside, i) for i in range(ndir)])
kappa, uvb, box = synthetic.uniform_workload(n, nnu)
with rt.DiffuseTransfer(device=0) as eng:
    eng.set_uniform_grid(n, box)
    eng.set_opacity(kappa)
    eng.transport(ang[:, 0].copy(), ang[:, 1].copy(), np.full(ndir, 1.0 / ndir), uvb)
    stages, blocks = eng.counter("brick_stages"), eng.counter("merge_blocks")
    points = [{"after_stage": eng.counter(f"merge_stage_{k}"), "final_blocks": eng.counter(f"merge_final_{k}"),
               "final_fraction": round(eng.counter(f"merge_final_{k}") / blocks, 4)} for k in range(eng.counter("merge_points"))]
print(json.dumps({"n": n, "ndir": ndir, "stages": stages, "merge_blocks": blocks, "points": points}))
