#!/usr/bin/env python3
"""The analysis modes at size: on a 256^3 uniform grid and on the 128^3 + refined 32^3 grid of BASELINE configs[3], a 1024^2 slice,
1024^2 projections (mass-weighted, zoom 1: the whole depth) for an izone whose depth axis is the contiguous storage axis (1), one
whose first map axis is (2) and one whose second map axis is (3), the clumping census and the gas PDF -- and, for comparison, what a
host pays today before it can draw anything: ftte_get_medium + ftte_get_density.  Each call is timed with HIP events on the
default stream around it (the library's stream is a blocking one, so the events bracket all of its work, the copy of the map to
the host included), median of `reps` after a warm-up.  Prints one JSON line per grid; --out FILE writes the list as JSON.
The kernels alone: run it under `rocprofv3 --kernel-trace --stats` with --reps 1.
usage: bench_analysis.py [--reps R] [--map M] [--out FILE] [--grid uniform|refined]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import radiativetransfer_amd as rt  # noqa: E402
from radiativetransfer_amd import synthetic  # noqa: E402


def option(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, nmap, out_path, only = option("--reps", 5), option("--map", 1024), option("--out", ""), option("--grid", "")
COPY_TBS = 4.4   # measured copy bandwidth of one MI355X, TB/s (DESIGN.md section 3d')
MSUN, PC = float(np.float32(1.98892e33)), float(np.float32(3.08568025e18))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn):
    return float(np.median([timed(fn) for _ in range(reps + 1)][1:])) if reps > 1 else timed(fn)


def grids():
    if only in ("", "uniform"):
        yield "uniform256", 256, np.zeros(256 ** 3, dtype=np.int32)
    if only in ("", "refined"):
        n, q = 128, 32
        blocks = [(n // 2 - q // 2 + a, n // 2 - q // 2 + b, n // 2 - q // 2 + c) for a in range(q) for b in range(q) for c in range(q)]
        yield "refined128", n, synthetic.refine_levels(n, blocks, depth=1)


results = []
for name, n, level in grids():
    nc = level.size
    rho = MSUN / PC ** 3 * 1e-3 * synthetic.lognormal_density(nc, seed=7, sigma_ln=1.5)
    HI = synthetic.lognormal_density(nc, seed=8, sigma_ln=2.0)
    abun2 = 0.02 * synthetic.lognormal_density(nc, seed=9, sigma_ln=0.5)
    with rt.StellarTransfer() as st:
        st.set_grid(n, level, 25.6e3 * PC)
        st.set_medium(HI, HI, HI, rho, abun2, 0)
        shape, centre = (nmap, nmap), (0.5, 0.5, 0.5)
        r = {"grid": name, "n": n, "leaves": int(nc), "map": nmap, "reps": reps}
        r["slice_ms"] = median_ms(lambda: st.slice_map(2, shape, 0.506896972656250))
        for izone, what in ((1, "depth_contiguous"), (2, "first_axis_contiguous"), (3, "second_axis_contiguous")):
            r[f"project_{what}_izone{izone}_ms"] = median_ms(lambda: st.project_map(izone, shape, centre, 1.0))
        r["project_path_integral_izone1_ms"] = median_ms(lambda: st.project_map(1, shape, centre, 1.0, 1))
        r["clumping_ms"] = median_ms(st.clumping)
        r["gas_pdf_ms"] = median_ms(st.gas_pdf)
        r["download_medium_and_density_ms"] = median_ms(lambda: (st.medium(), st.density()))
        r["census_floor_ms_9B_per_leaf"] = 9.0 * nc / (COPY_TBS * 1e12) * 1e3
        r["projection_floor_ms_16B_per_leaf"] = 16.0 * nc / (COPY_TBS * 1e12) * 1e3
        r["map_to_host_bytes"] = 4 * nmap * nmap
    print(json.dumps(r), flush=True)
    results.append(r)
if out_path:
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
