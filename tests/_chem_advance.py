"""The time-dependent ionisation step (chem_advance_cell of radiativetransfer_amd/csrc/ftte_chem_math.h) for the tests, twice:

  * advance(), equilibrium(): the header itself, compiled by g++ from tests/host/chem_advance_check.cpp into a small shared
    library (no sanitizers) and looped over the cells -- the host evaluation the GPU tests compare with bit for bit;
  * advance_numpy(): an independent restatement in numpy, vectorised over the cells, written from the scheme and not from the
    header: its own constants, interpolation, clip, rates, step and bisection.

Both take the argument list of _oracle.solve_rate_equations with (dt, substeps) appended."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from _hostlib import HostLib, dp as _dp, f64 as _f64

# The equilibrium limit (test_chem_advance_host.py (a), (b); test_chem_advance_gpu.py): the worst difference measured when the step
# was written, in units of the element's density; a test's bound is 16 times that and never above CEILING
WORST_A = 2.96e-15      # a step of 1e40 s, twice, against the reference's HI_out, HeI_out, HeII_out of initial_refined.npz (worst: HeII)
WORST_B = 1.05e-14      # once, against chem_bisect + chem_close at the same rates over chem_uvb_refined.npz (worst: HeII, no point rates)
CEILING = 1e-12


def _declare(L):
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
    head = [C.c_longlong, C.c_int, ip, C.c_double, dp, dp, dp, dp, dp, dp, C.c_int, dp, dp, dp, C.c_double, C.c_int, C.c_double, C.c_double,
            C.c_double, dp]
    L.ca_advance.argtypes = head + [C.c_double, C.c_int, dp, dp, dp, lp, dp]
    L.ca_equilibrium.argtypes = head + [dp, dp, dp]
    L.ca_advance.restype = L.ca_equilibrium.restype = C.c_longlong


lib = HostLib("chem_advance", "chem_advance_check.cpp", ("ftte_chem_math.h", "ftte_math.h"), "the chemistry step", _declare)


def _head(n, level, box, rho, tgas, HI, HeI, HeII, krate, run_uvb, J, ksi, uniform, threshold, logtem0, logtem9, dlogtem, k):
    keep = [np.ascontiguousarray(level, dtype=np.int32)] + [_f64(a) for a in (rho, tgas, HI, HeI, HeII)]
    nc = keep[1].size
    opt = [None if a is None else _f64(a) for a in (krate, J, ksi, uniform)]
    if opt[0] is not None:
        assert opt[0].shape == (3, nc)
    if run_uvb:
        assert opt[1].shape == (3, nc) and opt[2].size == 9
    else:
        assert opt[3].size == 3
    k = _f64(k)
    assert k.ndim == 2 and k.shape[0] == 6
    keep += opt + [k]
    args = [nc, int(n), keep[0].ctypes.data_as(C.POINTER(C.c_int32)), float(box), *[_dp(a) for a in keep[1:6]], _dp(opt[0]), int(bool(run_uvb)),
            _dp(opt[1]), _dp(opt[2]), _dp(opt[3]), float(threshold), k.shape[1], float(logtem0), float(logtem9), float(dlogtem), _dp(k)]
    return nc, args, keep


def advance(n, level, box, rho, tgas, HI, HeI, HeII, krate, run_uvb, J, ksi, uniform, threshold, logtem0, logtem9, dlogtem, k, dt, substeps=1):
    """-> HI, HeI, HeII, status (0, or 1 + the first failing cell), steps[ncell], change[ncell]"""
    nc, args, keep = _head(n, level, box, rho, tgas, HI, HeI, HeII, krate, run_uvb, J, ksi, uniform, threshold, logtem0, logtem9, dlogtem, k)
    out = [np.empty(nc) for _ in range(3)]
    steps, change = np.zeros(nc, dtype=np.int64), np.empty(nc)
    status = lib().ca_advance(*args, float(dt), int(substeps), *[_dp(a) for a in out], steps.ctypes.data_as(C.POINTER(C.c_longlong)), _dp(change))
    return out[0], out[1], out[2], int(status), steps, change


def equilibrium(n, level, box, rho, tgas, HI, HeI, HeII, krate, run_uvb, J, ksi, uniform, threshold, logtem0, logtem9, dlogtem, k):
    """the stationary state of the same equations at the same rates, by the header's own bisection -> HI, HeI, HeII, status"""
    nc, args, keep = _head(n, level, box, rho, tgas, HI, HeI, HeII, krate, run_uvb, J, ksi, uniform, threshold, logtem0, logtem9, dlogtem, k)
    out = [np.empty(nc) for _ in range(3)]
    status = lib().ca_equilibrium(*args, *[_dp(a) for a in out])
    return out[0], out[1], out[2], int(status)


# ---- the restatement ------------------------------------------------------------------------------------------------------

f32 = np.float32
PI = float(f32(3.141592654))
MP, MN = float(f32(1.6726231e-24)), float(f32(1.67492728e-24))
PSI = float(f32(0.76))
MH, MHE = MP, 2.0 * (MP + MN)
SIGMA = (float(f32(6.3e-18)), float(f32(7.42e-18)), float(f32(1.58e-18)))
DE_FLOOR = float(f32(1.0e-30))
MAX_STEPS = 4096
SLACK = 2.0 ** -48


def clip(rho, HI, HeI, HeII):
    """the incoming state within the elements' budgets"""
    nh, nhe = PSI * rho / MH, (1.0 - PSI) * rho / MHE
    return (nh, nhe, *within(nh, nhe, HI, HeI, HeII))


def within(nh, nhe, HI, HeI, HeII):
    a = np.fmax(np.fmin(HI, nh), 0.0)
    b = np.fmax(np.fmin(HeI, nhe), 0.0)
    d = np.fmax(np.fmin(HeII, nhe - b), 0.0)
    return a, b, d


def rates(n, level, box, nc, a, b, d, shield, krate, run_uvb, J, ksi, uniform, threshold):
    """photo-ionisation rates per absorber, Gamma24 (HI), Gamma25 (HeII), Gamma26 (HeI): the point sources' over the absorbers a, b, d
    of the clipped state; the background where the mean free path of `shield` (the incoming HI no more than nh, HeI and HeII as they
    come) is at least the threshold"""
    with np.errstate(all="ignore"):
        g = [np.zeros(nc) for _ in range(3)]
        if krate is not None:
            size = box / (f32(2) ** np.asarray(level).astype(f32) * f32(n)).astype(np.float64)
            vol = size * size * size
            for r, absorber in enumerate((a, d, b)):
                g[r] = np.maximum(np.where(absorber > 0.0, krate[r] / (vol * absorber), 0.0), 0.0)
        if run_uvb:
            ksi = np.asarray(ksi, dtype=np.float64).reshape(9)
            t1, t2, t3 = 4.0 * PI * J[0], 4.0 * PI * J[1], 4.0 * PI * J[2]
            g[0] = g[0] + t1 * ksi[0] + t2 * ksi[3] + t3 * ksi[6]
            g[1] = g[1] + t3 * ksi[7]
            g[2] = g[2] + t2 * ksi[5] + t3 * ksi[8]
        else:
            lit = 1.0 / (shield[0] * SIGMA[0] + shield[1] * SIGMA[1] + shield[2] * SIGMA[2]) >= threshold
            for r in range(3):
                g[r] = np.where(lit, g[r] + 4.0 * PI * uniform[r], g[r])
    return g


def coefficients(tgas, logtem0, logtem9, dlogtem, k):
    # (math.log is the C library's, as the library's host side takes it; numpy's own may differ in the last bit)
    lt = np.minimum(np.maximum(np.array([math.log(t) for t in tgas]), logtem0), logtem9)
    nr = k.shape[1]
    ix = np.clip(((lt - logtem0) / dlogtem).astype(np.int64) + 1, 1, nr - 1)
    t1, t2 = logtem0 + (ix - 1).astype(np.float64) * dlogtem, logtem0 + ix.astype(np.float64) * dlogtem
    return [k[r][ix - 1] + (lt - t1) * (k[r][ix] - k[r][ix - 1]) / (t2 - t1) for r in range(6)]


def step(h, de, nh, nhe, K, G, a, b, d):
    """one backward-Euler step of length h at electron density de"""
    k1, k2, k3, k4, k5, k6 = K
    g24, g25, g26 = G
    ion, rec = k1 * de + g24, k2 * de
    a1 = (a + h * rec * nh) / (1.0 + h * (ion + rec))
    hX, hY, hW, hZ = h * (k3 * de + g26), h * (k4 * de), h * (k5 * de + g25), h * (k6 * de)
    det = 1.0 + (hX + hY + hW + hZ) + (hX * hW + hX * hZ + hY * hZ)
    b1 = (b * (1.0 + (hY + hW + hZ)) + hY * (d + hZ * nhe)) / det
    d1 = (d + hZ * (nhe - b) + hX * (d + b) + hX * hZ * nhe) / det
    return a1, b1, d1


def advance_numpy(n, level, box, rho, tgas, HI, HeI, HeII, krate, run_uvb, J, ksi, uniform, threshold, logtem0, logtem9, dlogtem, k, dt, substeps=1):
    """-> HI, HeI, HeII, ok[ncell], steps[ncell]"""
    rho, tgas, HI, HeI, HeII, k = (np.asarray(x, dtype=np.float64) for x in (rho, tgas, HI, HeI, HeII, k))
    nc = rho.size
    with np.errstate(all="ignore"):
        nh, nhe, a, b, d = clip(rho, HI, HeI, HeII)
        G = rates(n, level, box, nc, a, b, d, (np.fmin(HI, nh), HeI, HeII), krate, run_uvb, J, ksi, uniform, threshold)
        K = coefficients(tgas, logtem0, logtem9, dlogtem, k)
        h = dt / float(substeps)
        steps = np.zeros(nc, dtype=np.int64)
        ok = np.ones(nc, dtype=bool)
        for sub in range(substeps):
            if sub:      # a substep takes its state as a call does
                a, b, d = within(nh, nhe, a, b, d)
            lo, hi = np.full(nc, DE_FLOOR), nh + 2.0 * nhe
            moves = np.zeros(nc, dtype=np.int64)
            live = ok.copy()
            new = (a.copy(), b.copy(), d.copy())
            while live.any():
                mid = 0.5 * (lo + hi)
                s = step(h, mid, nh, nhe, K, G, a, b, d)
                for dst, src in zip(new, s):
                    dst[live] = src[live]
                live &= ~((mid == lo) | (mid == hi) | (moves >= MAX_STEPS))
                res = mid - ((nh - s[0]) + s[2] + 2.0 * (nhe - s[1] - s[2]))
                up = live & (res > 0.0)
                down = live & ~(res > 0.0)
                hi = np.where(up, mid, hi)
                lo = np.where(down, mid, lo)
                moves += live
            a, b, d = (np.where(ok, x, y) for x, y in zip(new, (a, b, d)))
            steps += np.where(ok, moves, 0)
            ok &= moves < MAX_STEPS
        fH, fHe = a / nh, (b + d) / nhe
        ok &= (fH >= -SLACK) & (fH <= 1.0 + SLACK) & (fHe >= -SLACK) & (fHe <= 1.0 + SLACK) & (b >= -SLACK * nhe) & (d >= -SLACK * nhe)
    return a, b, d, ok, steps
