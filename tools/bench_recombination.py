#!/usr/bin/env python3
"""The diffuse recombination source at 256^3: ftte_recombination_source_device (40 bytes read and 24 written per leaf) beside
ftte_compute_opacities on the same medium (24 read, 24 written: the existing stream of the same class, the yardstick), a log-normal
density, temperatures over the table, the medium of tools/bench_advance.py.  Each call is timed with HIP events on the default stream
around it (the library's stream is a blocking one, so the events bracket all of its work: the kernel, the counters' way out and
back); the calls alternate -- the opacities, the pass with no emission in force (evolve's way), the pass with one in force --
`reps` times after a warm-up of each, and the medians are reported with the bytes per second the algorithm's own traffic comes to.  A call's time, not a kernel's: it holds a host synchronise.  Prints one JSON line.
usage: bench_recombination.py [n] [reps]"""
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
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
nc = n ** 3
box = 2.5e23
rng = np.random.default_rng(11)
rho = 3.0e-26 * synthetic.lognormal_density(nc, seed=7, sigma_ln=1.5)
mp, mn, psi = (float(np.float32(x)) for x in (1.6726231e-24, 1.67492728e-24, 0.76))
nh, nhe = psi * rho / mp, (1 - psi) * rho / (2 * (mp + mn))
HI, HeI, HeII = nh * 10 ** rng.uniform(-5, 0, nc), nhe * rng.uniform(0, 0.7, nc), nhe * rng.uniform(0, 0.3, nc)
tgas = 10 ** rng.uniform(2.0, 6.5, nc)
k, logtem0, logtem9, dlogtem = rt.rate_coefficient_tables(recombination_type=1)
beta, ksi, _ = rt.uvb_beta_table([1.8, 1.5, 1.2])
share = np.array([[0.7, 0.2, 0.1], [0.0, 0.6, 0.3], [0.1, 0.1, 0.8]])

st = rt.StellarTransfer()
st.set_uniform_grid(n, box)
st.set_rate_coefficients(logtem0, logtem9, dlogtem, k)
st.set_ground_recombination(rt.ground_recombination_tables())
st.set_medium(HI, HeI, HeII, rho, None, 0)
st.set_temperature(tgas)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


# recombination_source: no emission in force before the call, as in evolve's steps (the kernel writes the emission field itself);
# recombination_source_in_force: the call before it has left one in force (the kernel writes beside the field, one device copy brings S
# in: 48 B per leaf more)
calls = {"compute_opacities": (lambda: st.compute_opacities_from_medium(beta), 48), "recombination_source": (lambda: st.recombination_source_device(ksi, share), 64),
         "recombination_source_in_force": (lambda: st.recombination_source_device(ksi, share), 112)}
ms = {name: [] for name in calls}
lost = None
for r in range(reps + 1):
    for name, (fn, _) in calls.items():
        if name == "recombination_source":
            st.set_source_function(None)   # (a host-side switch, outside the timed call)
        t, out = timed(fn)
        if r:   # (the first round warms up)
            ms[name].append(t)
        if name == "recombination_source":
            lost = out
result = {"n": n, "cells": nc, "reps": reps, "lost_pairs": lost}
for name, (_, bytes_per_leaf) in calls.items():
    med = float(np.median(ms[name]))
    result[name] = {"call_ms": med, "call_ms_min": float(np.min(ms[name])), "call_ms_max": float(np.max(ms[name])), "bytes_per_leaf": bytes_per_leaf,
                    "bytes_per_s": bytes_per_leaf * nc / (med * 1e-3)}
result["ratio"] = result["recombination_source"]["call_ms"] / result["compute_opacities"]["call_ms"]
print(json.dumps(result))
st.close()
