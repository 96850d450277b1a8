#!/usr/bin/env python3
"""The ray spectra at size, on the medium of bench_spectra.py (an N^3 uniform grid, log-normal HI and temperature, a random
velocity field plus a Hubble flow), HI Lyman alpha, 1024 pixels, tau and the summaries kept on the device:
  (a) the N^2 axis-aligned rays that coincide with izone 1's pixel columns, next to ftte_sightline_spectra over the same columns in
      the same process (the yardstick), and whether the two gave the same bits;
  (b) 65 536 rays of random direction through random points of the box, from where they enter it to where they leave;
  (c) the rays of (b) continued periodically from their origins to a fixed length of 4 boxes (--boxes), with the time per segment
      beside (b)'s from the same process.
Each call is timed with HIP events on the default stream around it (the library's stream is a blocking one), median of `reps`
after a warm-up; the offsets-only call of ray_segments (the count launch, the read-back of the counts and the host's prefix sum)
by the wall clock.  Prints one JSON line; --out FILE writes it.  The kernels alone, and the share of the two walk launches: run it
under `rocprofv3 --kernel-trace --stats` with reps 1.
usage: bench_ray_spectra.py N reps [--nvel V] [--rays R] [--boxes B] [--out FILE]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import radiativetransfer_amd as rt  # noqa: E402
from radiativetransfer_amd import synthetic  # noqa: E402


def option(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


n, reps = int(sys.argv[1]), int(sys.argv[2])
nvel, nrandom, out_path, boxes = option("--nvel", 1024), option("--rays", 65536), option("--out", ""), option("--boxes", 4.0)
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


def wall_ms(fn):
    def once():
        t = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t)
    return float(np.median([once() for _ in range(reps + 1)][1:])) if reps > 1 else once()


nc = n ** 3
box = 25.6e3 * PC
rho = MSUN / PC ** 3 * 1e-3 * synthetic.lognormal_density(nc, seed=7, sigma_ln=1.5)
HI = 1e-9 * synthetic.lognormal_density(nc, seed=8, sigma_ln=2.0)
tgas = 1e4 * synthetic.lognormal_density(nc, seed=9, sigma_ln=0.5)
rng = np.random.default_rng(10)
vel = [rng.normal(0.0, 3.0e6, nc) for _ in range(3)]
hubble = 2.0e7 / box
v0, dv = -1.0e7, 4.0e7 / nvel
dev = torch.device("cuda", 0)

# (a) izone 1: map pixel (i, j) is storage column (i, j), the depth storage k; ray r = i + n j as the sightlines lie in memory
jj, ii = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
axis_o = np.stack([ii + 0.5, jj + 0.5, np.zeros(n * n)], axis=1)
axis_d = np.tile([0.0, 0.0, 1.0], (n * n, 1))
# (b) random directions through random points, from outside the box
rr = np.random.default_rng(11)
rand_d = rr.normal(size=(nrandom, 3))
rand_d /= np.sqrt((rand_d * rand_d).sum(axis=1, keepdims=True))
rand_o = rr.uniform(0.0, n, (nrandom, 3)) - 2.0 * n * rand_d

r = {"grid": f"uniform{n}", "n": n, "leaves": nc, "nvel": nvel, "reps": reps, "axis_rays": n * n, "random_rays": nrandom}
with rt.StellarTransfer() as st:
    st.set_grid(n, np.zeros(nc, dtype=np.int32), box)
    st.set_medium(HI, HI, HI, rho, None, 0)
    st.set_temperature(tgas)
    st.set_velocity(*vel)
    tau = torch.empty((n * n, nvel), dtype=torch.float64, device=dev)
    summary = torch.empty((n * n, 3), dtype=torch.float64, device=dev)
    tau_r = torch.empty((nrandom, nvel), dtype=torch.float64, device=dev)
    summary_r = torch.empty((nrandom, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    r["sightline_spectra_ms"] = median_ms(lambda: st.sightline_spectra(1, (n, n), nvel, v0, dv, rt.LYMAN_ALPHA, hubble=hubble, tau_device_ptr=tau.data_ptr(),
                                                                       summary_device_ptr=summary.data_ptr()))
    want_tau, want_summary = tau.clone(), summary.clone()
    r["axis_ray_spectra_ms"] = median_ms(lambda: st.ray_spectra(axis_o, axis_d, nvel, v0, dv, rt.LYMAN_ALPHA, hubble=hubble, tau_device_ptr=tau.data_ptr(),
                                                                summary_device_ptr=summary.data_ptr()))
    r["axis_rays_equal_the_sightlines_bit_for_bit"] = bool(torch.equal(tau.view(torch.int64), want_tau.view(torch.int64)) and
                                                           torch.equal(summary.view(torch.int64), want_summary.view(torch.int64)))
    r["axis_ratio_rays_over_sightlines"] = r["axis_ray_spectra_ms"] / r["sightline_spectra_ms"]
    dp, offsets = C.POINTER(C.c_double), np.zeros(n * n + 1, dtype=np.int64)
    r["axis_offsets_only_wall_ms"] = wall_ms(lambda: st._ok(st._lib.ftte_ray_segments(st._ctx, n * n, axis_o.ctypes.data_as(dp), axis_d.ctypes.data_as(dp), None,
                                                                                      offsets.ctypes.data_as(C.POINTER(C.c_int64)), 0, None, None, None)))
    r["random_ray_spectra_ms"] = median_ms(lambda: st.ray_spectra(rand_o, rand_d, nvel, v0, dv, rt.LYMAN_ALPHA, hubble=hubble, tau_device_ptr=tau_r.data_ptr(),
                                                                  summary_device_ptr=summary_r.data_ptr()))
    seg = st.ray_segments(rand_o, rand_d)
    counts = np.diff(seg["offset"])
    r["random_segments"], r["random_most_segments"], r["random_rays_that_hit"] = int(counts.sum()), int(counts.max()), int((counts > 0).sum())
    r["axis_pairs"], r["random_pairs"] = n * n * n * nvel, int(counts.sum()) * nvel
    s = summary_r.cpu().numpy()
    r["random_mean_W_cm_s"], r["random_mean_dv90_cm_s"] = float(s[:, 1].mean()), float(s[:, 2].mean())
    # (c) the same rays, periodic: the counts from the offsets-only call (the lists themselves would be gigabytes)
    length = np.full(nrandom, boxes * n)
    r["periodic_boxes"] = boxes
    r["periodic_ray_spectra_ms"] = median_ms(lambda: st.ray_spectra(rand_o, rand_d, nvel, v0, dv, rt.LYMAN_ALPHA, length, hubble=hubble, periodic=True,
                                                                    tau_device_ptr=tau_r.data_ptr(), summary_device_ptr=summary_r.data_ptr()))
    offsets = np.zeros(nrandom + 1, dtype=np.int64)
    st._ok(st._lib.ftte_ray_segments_periodic(st._ctx, nrandom, rand_o.ctypes.data_as(dp), rand_d.ctypes.data_as(dp), length.ctypes.data_as(dp),
                                              offsets.ctypes.data_as(C.POINTER(C.c_int64)), 0, None, None, None))
    counts = np.diff(offsets)
    r["periodic_segments"], r["periodic_most_segments"], r["periodic_pairs"] = int(counts.sum()), int(counts.max()), int(counts.sum()) * nvel
    r["random_ns_per_segment"] = 1e6 * r["random_ray_spectra_ms"] / r["random_segments"]
    r["periodic_ns_per_segment"] = 1e6 * r["periodic_ray_spectra_ms"] / r["periodic_segments"]
    s = summary_r.cpu().numpy()
    r["periodic_mean_W_cm_s"], r["periodic_mean_dv90_cm_s"] = float(s[:, 1].mean()), float(s[:, 2].mean())
print(json.dumps(r), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump([r], f, indent=1)
        f.write("\n")
