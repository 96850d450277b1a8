#!/usr/bin/env python3
"""The start-up expansion of HII regions at 256^3 (equiSources.f90:1035-1069): ftte_expand_hii_regions on a uniform grid with a
log-normal density (median nH = 1 cm^-3, sigma_ln = 1.5, box 25.6 kpc: cells of 100 pc under radii of 32 pc to some kpc) and 1024
stars at random leaves, parameters from the host leaves' densities.  Timed with HIP events on the default stream around the call
(the library's stream is a blocking one, so the events bracket all of its work), median of `reps` after a warm-up, without and
with rhoCoef coming back to the host.  Prints one JSON line: ms, exact star-leaf tests, their share of nsrc x ncell, leaves changed,
and the floor of 64 B per leaf (four fields read and written) at the copy bandwidth DESIGN.md quotes.
usage: bench_expansion.py [n] [nstars] [reps]"""
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
nstars = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
COPY_TBS = 4.4   # measured copy bandwidth of one MI355X, TB/s (DESIGN.md section 3d')
nc = n ** 3
box = 25.6e3 * float(np.float32(3.08568025e18))
rng = np.random.default_rng(1035)
mp, mn, psi = (float(np.float32(x)) for x in (1.6726231e-24, 1.67492728e-24, 0.76))
rho = (mp / psi) * synthetic.lognormal_density(nc, seed=7, sigma_ln=1.5)
nh, nhe = psi * rho / mp, (1 - psi) * rho / (2 * (mp + mn))
HI, HeI, HeII = nh * 10 ** rng.uniform(-5, 0, nc), nhe * rng.uniform(0, 0.7, nc), nhe * rng.uniform(0, 0.3, nc)
stars = rng.integers(0, nc, nstars)

st = rt.StellarTransfer()
st.set_uniform_grid(n, box)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


call_ms, with_coef_ms = [], []
for r in range(reps + 1):
    st.set_medium(HI, HeI, HeII, rho, None, 0)
    t, (_, changed) = timed(lambda: st.expand_hii_regions(stars, want_rho_coef=False))
    tests = st.counter("expansion_exact_tests")
    st.set_medium(HI, HeI, HeII, rho, None, 0)
    t2, (coef, changed2) = timed(lambda: st.expand_hii_regions(stars))
    assert changed2 == changed and int((coef < 1).sum()) == changed
    if r:   # (the first round warms up)
        call_ms.append(t)
        with_coef_ms.append(t2)
print(json.dumps({"n": n, "cells": nc, "stars": nstars, "reps": reps, "call_ms": float(np.median(call_ms)), "call_ms_all": call_ms,
                  "call_with_rho_coef_ms": float(np.median(with_coef_ms)), "exact_tests": tests,
                  "exact_tests_per_pair": tests / (float(nstars) * nc), "leaves_changed": changed,
                  "floor_ms_64B_per_leaf": 64.0 * nc / (COPY_TBS * 1e12) * 1e3}))
st.close()
