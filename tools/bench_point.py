#!/usr/bin/env python3
"""Throughput of the point-source tracer with many stars: 256^3 cells, log-normal hydrogen and helium, S stars at random
cells; without dust and with the dust approximation `completeSublimation`.  Prints ms per trace, stars/s, cell crossings/s.
usage: bench_point.py [n] [stars] [--populations N] [--root DIR] [--label TEXT]

--populations N: N stars, each with a population of its own (a distinct coefMetal), without dust, three ways:
  per-star  stellar_beta_table then point_sources(1 star) for every star, what the Fortran drop-in does with ftteStarBatch = 1
  batched   one stellar_beta_tables and one point_sources_populations (table time and trace time apart)
  shared    the N stars through point_sources with one table set (what the figures without --populations measure)
A build without population slots runs per-star and shared only.  --root DIR takes the package from another source tree (a build
of another commit), --label TEXT starts every line."""
import os, sys, time
import numpy as np
args = sys.argv[1:]


def option(name, default=None):
    if name in args:
        i = args.index(name)
        value = args[i + 1]
        del args[i:i + 2]
        return value
    return default


ROOT = os.path.abspath(option("--root", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
LABEL = option("--label", "")
POPULATIONS = int(option("--populations", 0))
sys.path.insert(0, ROOT)
import radiativetransfer_amd as rt
from radiativetransfer_amd import synthetic

n = int(args[0]) if len(args) > 0 else 256
S = POPULATIONS if POPULATIONS else int(args[1]) if len(args) > 1 else 512
nc = n ** 3
box = 3.0e22
st = rt.StellarTransfer()
st.set_uniform_grid(n, box)
st.stellar_beta_table(*synthetic.stellar_population(), 3, 0.4, 2, 0.3)
rho = synthetic.lognormal_density(nc, seed=3, sigma_ln=1.0)
HI = rho * 2.0 / (6.3e-18 * box)          # hydrogen optical depth 2 across the box at mean density
HeI, HeII = 0.08 * HI, 0.01 * HI
rng = np.random.default_rng(5)
src = rng.choice(nc, S, replace=False)
ndot = rng.uniform(1, 3, S)
if POPULATIONS:
    pop = synthetic.stellar_population()
    cm = (np.arange(S) + 0.5) / S                       # coefMetal is continuous: no two stars alike
    st.set_medium(HI, HeI, HeII, rho * 1e-24, np.full(nc, 0.02), 0)
    # the per-star table call through the C ABI with the library's arrays converted once, as a Fortran host holds them: the
    # Python method's copies of the spectra (1.8 MB per call) are not part of what is measured
    import ctypes as C
    dp = C.POINTER(C.c_double)
    a_f, wl, sl_f = np.asfortranarray(pop[0].reshape(7, 5)), np.ascontiguousarray(pop[1]), np.asfortranarray(pop[2])

    def table_of(coef_metal):
        total = C.c_double()
        st._ok(st._lib.ftte_stellar_beta_table(st._ctx, a_f.ctypes.data_as(dp), wl.size, wl.ctypes.data_as(dp), sl_f.shape[1], sl_f.shape[0],
                                               sl_f.ctypes.data_as(dp), 3, 0.4, 2, float(coef_metal), C.byref(total)))

    say = lambda what, text: print(f"{LABEL} {what:9s}: {S} stars in {n}^3: {text}", flush=True)
    for rep in range(3):
        st.set_zero_rates()
        t0 = time.perf_counter()
        for s in range(S):
            table_of(cm[s])
            st.point_sources(src[s:s + 1], ndot[s:s + 1])
        dt = time.perf_counter() - t0
        per_star = st.rates()
        say("per-star", f"{dt * 1e3:9.2f} ms = {dt / S * 1e3:7.3f} ms per star")
        if hasattr(st, "stellar_beta_tables"):
            st.set_zero_rates()
            t0 = time.perf_counter()
            st.stellar_beta_tables(*pop, np.full(S, 3), np.full(S, 0.4), np.full(S, 2), cm)
            t1 = time.perf_counter()
            st.point_sources_populations(src, ndot, np.arange(S))
            t2 = time.perf_counter()
            k = st.rates()
            say("batched", f"{(t2 - t0) * 1e3:9.2f} ms = {(t2 - t0) / S * 1e3:7.3f} ms per star (tables {(t1 - t0) * 1e3:8.2f} ms, trace "
                           f"{(t2 - t1) * 1e3:8.2f} ms, {st.ray_steps() / (t2 - t1):.3e} cell crossings/s); largest deviation from per-star "
                           f"{np.max(np.abs(k - per_star) / np.abs(per_star).max(axis=1, keepdims=True)):.1e} of the largest rate")
        st.stellar_beta_table(*pop, 3, 0.4, 2, 0.3)
        st.set_zero_rates()
        t0 = time.perf_counter(); st.point_sources(src, ndot); dt = time.perf_counter() - t0
        say("shared", f"{dt * 1e3:9.2f} ms = {dt / S * 1e3:7.3f} ms per star, {st.ray_steps() / dt:.3e} cell crossings/s")
    sys.exit(0)
for dust, label in ((0, "no dust"), (1, "dust ~ HI")):
    st.set_medium(HI, HeI, HeII, rho * 1e-24, np.full(nc, 0.02), dust)
    for rep in range(3):
        st.set_zero_rates()
        t0 = time.perf_counter(); st.point_sources(src, ndot); dt = time.perf_counter() - t0
    steps = st.ray_steps()
    k = st.rates()
    print(f"{label:10s}: {S} stars in {n}^3: {dt * 1e3:8.2f} ms = {S / dt:9.1f} stars/s, {steps / dt:.3e} cell crossings/s "
          f"({steps / S:.0f} per star); absorbed HI fraction {k[0].sum() / (st.rate_tables()[0, 0, 0, 0, 0] * ndot.sum()):.4f}", flush=True)
