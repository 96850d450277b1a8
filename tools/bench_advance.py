#!/usr/bin/env python3
"""The time-dependent ionisation step at 256^3: ftte_advance_rate_equations with the uniform background behind the self-shielding
test (half of the cells lit, half shielded), a log-normal density, substeps 1 and 4, timed with HIP events on the default stream
around the call (the library's stream is a blocking one, so the events bracket all of its work: the kernel, the three copies of
the new species into the medium and the counters' way back), median of `reps` after a warm-up; the mean bisection steps per cell
and substep.  The medium and dt are those of tools/bench_initial_equilibrium.py, whose two-pass kernel is the figure to hold this
one against.  Prints one JSON line.  usage: bench_advance.py [n] [reps] [dt_s]"""
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
dt = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0e13
nc = n ** 3
g = np.load(os.path.join(ROOT, "tests", "golden", "chem_uvb_refined.npz"))   # the reference's rate-coefficient tables
box = 2.5e23
rng = np.random.default_rng(11)
rho = 3.0e-26 * synthetic.lognormal_density(nc, seed=7, sigma_ln=1.5)
mp, mn, psi = (float(np.float32(x)) for x in (1.6726231e-24, 1.67492728e-24, 0.76))
nh, nhe = psi * rho / mp, (1 - psi) * rho / (2 * (mp + mn))
HI, HeI, HeII = nh * 10 ** rng.uniform(-5, 0, nc), nhe * rng.uniform(0, 0.7, nc), nhe * rng.uniform(0, 0.3, nc)
tgas = 10 ** rng.uniform(2.0, 6.5, nc)
uniform = np.array([3.0e-14, 1.0e-16, 2.0e-14])
mfp = 1.0 / (np.minimum(HI, nh) * float(np.float32(6.3e-18)) + HeI * float(np.float32(7.42e-18)) + HeII * float(np.float32(1.58e-18)))
threshold = float(np.median(mfp))   # half of the cells lit, half self-shielded

st = rt.StellarTransfer()
st.set_uniform_grid(n, box)
st.set_rate_coefficients(float(g["logtem0"]), float(g["logtem9"]), float(g["dlogtem"]), g["k"])
st.set_temperature(tgas)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


result = {"n": n, "cells": nc, "reps": reps, "dt_s": dt, "lit_share": float((mfp >= threshold).mean())}
for substeps in (1, 4):
    ms, steps = [], 0
    for r in range(reps + 1):
        st.set_medium(HI, HeI, HeII, rho, None, 0)
        t, change = timed(lambda: st.advance_rate_equations(dt, False, None, None, uniform, threshold, substeps=substeps))
        steps = st.rate_equation_steps()
        if r:   # (the first round warms up)
            ms.append(t)
    neutral, total = st.hydrogen_mass()
    result[f"substeps_{substeps}"] = {"call_ms": float(np.median(ms)), "call_ms_all": ms, "steps_per_cell_per_substep": steps / (float(substeps) * nc),
                                      "largest_change": change, "neutral_fraction": neutral / total}
print(json.dumps(result))
st.close()
