#!/usr/bin/env python3
"""The sightline spectra at size: an N^3 uniform grid with a synthetic log-normal medium (HI, temperature around 1e4 K, a random
velocity field of a few 1e6 cm/s plus a Hubble flow across the box), N^2 sightlines along izone 1 x 1024 pixels, HI Lyman alpha
and the same line with damping = 0; tau and the summaries stay on the device (the _device variant into torch tensors: what is
timed is the two kernels, not 8 N^2 1024 bytes over PCIe).  For comparison, what a host paid before it could start its own sum:
the medium, the density, the temperature, and the velocities it would have to bring itself.  Each call is timed with HIP events
on the default stream around it (the library's stream is a blocking one), median of `reps` after a warm-up.  Prints one JSON
line; --out FILE writes it.  The kernels alone: run it under `rocprofv3 --kernel-trace --stats` with reps 1.
usage: bench_spectra.py N reps [--nvel V] [--out FILE]"""
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


n, reps = int(sys.argv[1]), int(sys.argv[2])
nvel, out_path = option("--nvel", 1024), option("--out", "")
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


nc = n ** 3
box = 25.6e3 * PC
rho = MSUN / PC ** 3 * 1e-3 * synthetic.lognormal_density(nc, seed=7, sigma_ln=1.5)
HI = 1e-9 * synthetic.lognormal_density(nc, seed=8, sigma_ln=2.0)
tgas = 1e4 * synthetic.lognormal_density(nc, seed=9, sigma_ln=0.5)
rng = np.random.default_rng(10)
vel = [rng.normal(0.0, 3.0e6, nc) for _ in range(3)]
hubble = 2.0e7 / box                       # 200 km/s across the box
v0, dv = -1.0e7, 4.0e7 / nvel              # the flow plus the scatter, a margin on both sides
doppler = (rt.LYMAN_ALPHA[0], 0.0, rt.LYMAN_ALPHA[2], 0.0)
dev = torch.device("cuda", 0)
r = {"grid": f"uniform{n}", "n": n, "leaves": nc, "sightlines": n * n, "nvel": nvel, "reps": reps}
with rt.StellarTransfer() as st:
    st.set_grid(n, np.zeros(nc, dtype=np.int32), box)
    st.set_medium(HI, HI, HI, rho, None, 0)
    st.set_temperature(tgas)
    st.set_velocity(*vel)
    tau = torch.empty((n, n, nvel), dtype=torch.float64, device=dev)
    summary = torch.empty((n, n, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for name, line in (("lyman_alpha", rt.LYMAN_ALPHA), ("doppler", doppler)):
        r[f"spectra_{name}_ms"] = median_ms(lambda: st.sightline_spectra(1, (n, n), nvel, v0, dv, line, hubble=hubble, tau_device_ptr=tau.data_ptr(),
                                                                         summary_device_ptr=summary.data_ptr()))
        s = summary.cpu().numpy()
        r[f"{name}_mean_W_cm_s"], r[f"{name}_mean_dv90_cm_s"], r[f"{name}_max_tau"] = float(s[:, :, 1].mean()), float(s[:, :, 2].mean()), float(tau.max().item())
    r["summaries_only_lyman_alpha_ms"] = median_ms(lambda: st.sightline_spectra(1, (n, n), nvel, v0, dv, rt.LYMAN_ALPHA, hubble=hubble,
                                                                                 summary_device_ptr=summary.data_ptr()))
    r["download_medium_density_temperature_ms"] = median_ms(lambda: (st.medium(), st.density(), st.temperature()))
    r["pairs"] = n * n * n * nvel          # (pixel, segment) pairs a call evaluates: n segments per sightline
    r["velocity_bytes_the_host_would_bring"] = 3 * 8 * nc
print(json.dumps(r), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump([r], f, indent=1)
        f.write("\n")
