#!/usr/bin/env python3
"""The coupled step at 256^3: ftte_advance_thermochemistry on two media, timed with HIP events on the default stream around the call
(the library's stream is a blocking one, so the events bracket all of its work: the kernel, the copies of the new species, temperature,
logarithm and subcycle map, the counters' way back), `reps` calls after a warm-up, all quoted.

  (a) the medium of tools/bench_thermal.py (a log-normal density, the uniform background behind the self-shielding test: half of the
      cells lit, half shielded; T log-uniform over 1e3 .. 1e5 K), dt = 1e12 s, max_subcycles = 1: one chemistry and one temperature
      step per leaf, which is what the pair ftte_advance_rate_equations, ftte_advance_temperature does in two calls -- timed here too,
      on the same medium, alternating with the coupled call;
  (b) a front medium: the same, with a shell of neutral 100 K leaves around the box centre, about 2 % of the leaves, lit through
      the transfer's J at Gamma24 ~ 1e-12 /s (J = (3.8, 1.5, 0.5) 1e-22 in the three groups everywhere; the rest of the grid keeps its
      state), dt = 1e13 s, eta = 0.1, max_subcycles = 256: the time, the mean and the largest subcycle count, and the lane efficiency
      sum(n) / (64 sum over aligned groups of 64 consecutive leaves of max n) computed here from ftte_get_subcycles.  Twice: in the
      medium as it stands, whose every leaf starts far from balance with this J, and in the same medium brought into balance with it
      first, where only the shell has far to go.

Prints one JSON line.  usage: bench_thermochem.py [n] [reps]"""
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
nc = n ** 3
g = np.load(os.path.join(ROOT, "tests", "golden", "chem_uvb_refined.npz"))   # the reference's rate-coefficient tables, and ksi
box = 2.5e23
rng = np.random.default_rng(11)
rho = 3.0e-26 * synthetic.lognormal_density(nc, seed=7, sigma_ln=1.5)
mp, mn, psi = (float(np.float32(x)) for x in (1.6726231e-24, 1.67492728e-24, 0.76))
nh, nhe = psi * rho / mp, (1 - psi) * rho / (2 * (mp + mn))
HI, HeI, HeII = nh * 10 ** rng.uniform(-5, 0, nc), nhe * rng.uniform(0, 0.7, nc), nhe * rng.uniform(0, 0.3, nc)
tgas = 10 ** rng.uniform(3.0, 5.0, nc)
uniform = np.array([3.0e-14, 1.0e-16, 2.0e-14])      # tools/bench_advance.py's
_, ug = rt.uniform_table(1.8, 1.5)
mix = 1.0e-22 * ug[0] + 3.0e-22 * ug[1]
uniform_gamma = np.array([mix[0], mix[2], mix[1]])   # the gammas of HI, HeII, HeI: tools/bench_thermal.py's
mfp = 1.0 / (np.minimum(HI, nh) * float(np.float32(6.3e-18)) + HeI * float(np.float32(7.42e-18)) + HeII * float(np.float32(1.58e-18)))
threshold = float(np.median(mfp))   # half of the cells lit, half self-shielded
cool, compa = rt.cooling_coefficient_tables(recombination_type=1)
_, _, gamma = rt.uvb_beta_table([1.8, 1.5, 1.2])

st = rt.StellarTransfer()
st.set_uniform_grid(n, box)
st.set_rate_coefficients(float(g["logtem0"]), float(g["logtem9"]), float(g["dlogtem"]), g["k"])
st.set_cooling_coefficients(cool, compa, 9.0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def span(ms):
    return [min(ms), max(ms)]


result = {"n": n, "cells": nc, "reps": reps, "lit_share": float((mfp >= threshold).mean())}

# (a) one subcycle against the pair, alternating
dt = 1.0e12
coupled, chemistry, thermal, steps = [], [], [], {}
for r in range(reps + 1):
    st.set_medium(HI, HeI, HeII, rho, None, 0)
    st.set_temperature(tgas)
    t, out = timed(lambda: st.advance_thermochemistry(dt, False, None, None, None, uniform, uniform_gamma, threshold, max_subcycles=1))
    steps["coupled"] = st.rate_equation_steps()
    st.set_medium(HI, HeI, HeII, rho, None, 0)
    st.set_temperature(tgas)
    t1, _ = timed(lambda: st.advance_rate_equations(dt, False, None, None, uniform, threshold))
    steps["chemistry"] = st.rate_equation_steps()
    t2, _ = timed(lambda: st.advance_temperature(dt, False, None, None, uniform_gamma, threshold))
    steps["thermal"] = st.rate_equation_steps()
    if r:   # (the first round warms up)
        coupled.append(t); chemistry.append(t1); thermal.append(t2)
pair = [a + b for a, b in zip(chemistry, thermal)]
result["one_subcycle"] = {"dt_s": dt, "coupled_call_ms": span(coupled), "coupled_call_ms_all": coupled, "pair_ms": span(pair), "pair_ms_all": pair,
                          "chemistry_call_ms": span(chemistry), "thermal_call_ms": span(thermal),
                          "steps_per_cell": {k: v / float(nc) for k, v in steps.items()}, "subcycles": out}

# (b) the front medium
dt, eta, cap = 1.0e13, 0.1, 256
idx = np.arange(nc)
x, y, z = idx // (n * n), (idx // n) % n, idx % n
r2 = (x - n / 2 + 0.5) ** 2 + (y - n / 2 + 0.5) ** 2 + (z - n / 2 + 0.5) ** 2
r0 = 0.3 * n
shell = (r2 >= r0 ** 2) & (r2 < (r0 + 0.02 * nc / (4 * np.pi * r0 ** 2)) ** 2)      # ~2 % of the leaves
del idx, x, y, z, r2
J = np.array([3.8e-22, 1.5e-22, 0.5e-22])[:, None] * np.ones((1, nc))
pad = (-nc) % 64


def front(state):
    """the shell put into `state` (HI, HeI, HeII, tgas), the call timed, the subcycle map read"""
    fHI, fHeI, fHeII, ftgas = (a.copy() for a in state)
    fHI[shell], fHeI[shell], fHeII[shell], ftgas[shell] = nh[shell], nhe[shell], 0.0, 100.0
    ms, one = [], []
    for r in range(reps + 1):
        st.set_medium(fHI, fHeI, fHeII, rho, None, 0)
        st.set_temperature(ftgas)
        t, out = timed(lambda: st.advance_thermochemistry(dt, True, J, g["ksi"], gamma, eta=eta, max_subcycles=cap))
        if r:
            ms.append(t)
    sub, steps = st.subcycles().astype(np.int64), st.rate_equation_steps()
    groups = np.concatenate([sub, np.zeros(pad, np.int64)]).reshape(-1, 64)
    # the same medium in one subcycle per leaf: what (mean subcycles) x (one subcycle) is made of, J's upload included in both
    for r in range(reps + 1):
        st.set_medium(fHI, fHeI, fHeII, rho, None, 0)
        st.set_temperature(ftgas)
        t, _ = timed(lambda: st.advance_thermochemistry(dt, True, J, g["ksi"], gamma, eta=eta, max_subcycles=1))
        if r:
            one.append(t)
    return {"dt_s": dt, "eta": eta, "max_subcycles": cap, "shell_share": float(shell.mean()), "call_ms": span(ms), "call_ms_all": ms,
            "one_subcycle_call_ms": span(one), "subcycles": out, "mean_subcycles": float(sub.mean()),
            "mean_subcycles_in_the_shell": float(sub[shell].mean()), "mean_subcycles_outside": float(sub[~shell].mean()),
            "share_of_leaves_with_one_subcycle": float((sub == 1).mean()), "largest_subcycles": int(sub.max()),
            "lane_efficiency": float(sub.sum() / (64.0 * groups.max(axis=1).sum())), "steps_per_cell": steps / float(nc)}


# the shell in bench_thermal.py's medium as it stands: every leaf starts far from balance with this J
result["front"] = front((HI, HeI, HeII, tgas))
# and in the same medium brought into balance with this J first (three coupled calls of 1e16 s): only the shell has far to go
st.set_medium(HI, HeI, HeII, rho, None, 0)
st.set_temperature(tgas)
for _ in range(3):
    st.advance_thermochemistry(1.0e16, True, J, g["ksi"], gamma, eta=0.5, max_subcycles=64)
result["front_in_a_grid_in_balance"] = front((*st.medium(), st.temperature()))
print(json.dumps(result))
st.close()
