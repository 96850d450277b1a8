#!/usr/bin/env python3
"""The temperature step at 256^3: ftte_advance_temperature on the medium of tools/bench_advance.py (a log-normal density, the uniform
background behind the self-shielding test: half of the cells lit, half shielded), temperatures log-uniform over 1e3 .. 1e5 K,
dt = 1e12 s, one substep; timed with HIP events on the default stream around the call (the library's stream is a blocking one, so
the events bracket all of its work: the kernel, the two copies of the new temperature and its logarithm, the counters' way back),
`reps` calls after a warm-up, all quoted.  Both layouts of the cooling table are timed in one process: the caller's [13][nratec]
(the default) and node-major [nratec][16] (FTTE_THERMAL_TABLE=nodes, read by ftte_set_cooling_coefficients).  Also the
thermal-equilibrium pass.  Prints one JSON line.  usage: bench_thermal.py [n] [reps] [dt_s]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import radiativetransfer_amd as rt  # noqa: E402
from radiativetransfer_amd import synthetic  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dt = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0e12
nc = n ** 3
g = np.load(os.path.join(ROOT, "tests", "golden", "chem_uvb_refined.npz"))   # the reference's rate-coefficient tables
box = 2.5e23
rng = np.random.default_rng(11)
rho = 3.0e-26 * synthetic.lognormal_density(nc, seed=7, sigma_ln=1.5)
mp, mn, psi = (float(np.float32(x)) for x in (1.6726231e-24, 1.67492728e-24, 0.76))
nh, nhe = psi * rho / mp, (1 - psi) * rho / (2 * (mp + mn))
HI, HeI, HeII = nh * 10 ** rng.uniform(-5, 0, nc), nhe * rng.uniform(0, 0.7, nc), nhe * rng.uniform(0, 0.3, nc)
tgas = 10 ** rng.uniform(3.0, 5.0, nc)
_, ug = rt.uniform_table(1.8, 1.5)
mix = 1.0e-22 * ug[0] + 3.0e-22 * ug[1]
uniform_gamma = np.array([mix[0], mix[2], mix[1]])   # the gammas of HI, HeII, HeI
mfp = 1.0 / (np.minimum(HI, nh) * float(np.float32(6.3e-18)) + HeI * float(np.float32(7.42e-18)) + HeII * float(np.float32(1.58e-18)))
threshold = float(np.median(mfp))   # half of the cells lit, half self-shielded
cool, compa = rt.cooling_coefficient_tables(recombination_type=1)

st = rt.StellarTransfer()
st.set_uniform_grid(n, box)
st.set_rate_coefficients(float(g["logtem0"]), float(g["logtem9"]), float(g["dlogtem"]), g["k"])
st.set_medium(HI, HeI, HeII, rho, None, 0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


result = {"n": n, "cells": nc, "reps": reps, "dt_s": dt, "lit_share": float((mfp >= threshold).mean())}
for layout in ("rows", "nodes"):
    os.environ["FTTE_THERMAL_TABLE"] = layout
    st.set_cooling_coefficients(cool, compa, 9.0)
    ms, eq_ms, steps = [], [], 0
    for r in range(reps + 1):
        st.set_temperature(tgas)
        t, change = timed(lambda: st.advance_temperature(dt, False, None, None, uniform_gamma, threshold))
        steps = st.rate_equation_steps()
        if r:   # (the first round warms up)
            ms.append(t)
    for r in range(reps + 1):
        # (through the library itself, without the three host arrays StellarTransfer.thermal_equilibrium asks for)
        t, _ = timed(lambda: st._ok(st._lib.ftte_thermal_equilibrium(st._ctx, 0, None, None, uniform_gamma.ctypes.data_as(C.POINTER(C.c_double)),
                                                                     threshold, 0, None, None, None)))
        if r:
            eq_ms.append(t)
    per_cell = steps / float(nc)
    result[layout] = {"advance_call_ms": [min(ms), max(ms)], "advance_call_ms_all": ms, "steps_per_cell": per_cell,
                      "us_per_step_of_all_cells": [1e3 * min(ms) / per_cell, 1e3 * max(ms) / per_cell], "largest_change": change,
                      "equilibrium_call_ms": [min(eq_ms), max(eq_ms)]}
print(json.dumps(result))
st.close()
