"""The diffuse recombination source (radiativetransfer_amd/csrc/ftte_recombination_math.h) for the tests, twice:

  * source(): the header itself, compiled by g++ from tests/host/recombination_check.cpp into a small shared library (no
    sanitizers) and looped over the cells -- the host evaluation the GPU tests compare with bit for bit;
  * source_numpy(): an independent restatement in numpy, vectorised over the cells, written from the feature's statement and not
    from the header: its own constants, clip, interpolation (as a weighted mean of the two nodes) and sums.

The reference has nothing to compare with: its emissivity is hard-wired to zero."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from _hostlib import CSRC, ROOT, SANITIZE, HostLib, dp as _dp, f64 as _f64  # noqa: F401

EPS = np.finfo(float).eps
IDENTITY = np.eye(3)
SPLIT = np.array([[0.7, 0.2, 0.1], [0.0, 0.6, 0.3], [0.1, 0.1, 0.8]])      # rows (ions) over groups; every row sum <= 1
H_ONLY = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])


def _declare(L):
    dp = C.POINTER(C.c_double)
    L.rc_source.argtypes = [C.c_longlong, dp, dp, dp, dp, dp, C.c_int, C.c_double, C.c_double, C.c_double, dp, dp, dp, dp, dp, C.POINTER(C.c_longlong)]
    L.rc_source.restype = C.c_longlong


lib = HostLib("recombination", "recombination_check.cpp", ("ftte_recombination_math.h", "ftte_chem_math.h", "ftte_math.h"),
              "the recombination source", _declare)
SOURCE = lib.source


def libm_log(x):
    """the C library's log, which ftte_set_temperature stores per leaf (numpy's own may differ in the last bit)"""
    return np.array([math.log(v) for v in np.asarray(x, dtype=np.float64).ravel()])


def source(rho, logtem, HI, HeI, HeII, grid, g, ksi, share):
    """-> S[3][ncell], E[3][ncell], lost, status (0, or 1 + the first failing cell)"""
    f = [_f64(a) for a in (rho, logtem, HI, HeI, HeII)]
    g, ksi, share = _f64(g), _f64(ksi).reshape(3, 3), _f64(share).reshape(3, 3)
    assert g.ndim == 2 and g.shape[0] == 3
    nc = f[0].size
    S, E, lost = np.empty((3, nc)), np.empty((3, nc)), C.c_longlong()
    status = lib().rc_source(nc, *[_dp(a) for a in f], g.shape[1], *[float(v) for v in grid], _dp(g), _dp(ksi), _dp(share), _dp(S), _dp(E), C.byref(lost))
    return S, E, int(lost.value), int(status)


# ---- the restatement ------------------------------------------------------------------------------------------------------

f32 = np.float32
PI = float(f32(3.141592654))
MP, MN = float(f32(1.6726231e-24)), float(f32(1.67492728e-24))
PSI = float(f32(0.76))
MH, MHE = MP, 2.0 * (MP + MN)


def capture(HI, HeI, HeII, ksi):
    """D[3][ncell]: the absorbers' photon capture per unit 4 pi J from species already within their budgets"""
    k = np.asarray(ksi, dtype=np.float64).reshape(3, 3)
    return np.stack([HI * k[0, 0], HI * k[1, 0] + HeI * k[1, 2], HI * k[2, 0] + HeII * k[2, 1] + HeI * k[2, 2]])


def clipped(rho, HI, HeI, HeII):
    """-> nh, nhe and the species within their elements' budgets"""
    rho = np.asarray(rho, dtype=np.float64)
    nh, nhe = PSI * rho / MH, (1.0 - PSI) * rho / MHE
    hi = np.maximum(np.minimum(HI, nh), 0.0)
    hei = np.maximum(np.minimum(HeI, nhe), 0.0)
    heii = np.maximum(np.minimum(HeII, nhe - hei), 0.0)
    return nh, nhe, hi, hei, heii


def source_numpy(rho, logtem, HI, HeI, HeII, grid, g, ksi, share):
    """-> S, E, D, lost, and S_scale: S with each coefficient replaced by the larger of its two table nodes (what the comparison's
    bound is made of: the header's a + w (b - a) and the weighted mean here both lie within a few eps of max(a, b) of the exact value,
    not of the value itself where b << a and w -> 1)"""
    logtem0, logtem9, dlogtem = grid
    g, share = np.asarray(g, dtype=np.float64), np.asarray(share, dtype=np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        nh, nhe, hi, hei, heii = clipped(rho, HI, HeI, HeII)
        hii, heiii = nh - hi, nhe - hei - heii
        de = 2.0 * heiii + heii + hii                                   # (the other order)
        lt = np.minimum(np.maximum(np.asarray(logtem, dtype=np.float64), logtem0), logtem9)
        nr = g.shape[1]
        ix = np.clip(((lt - logtem0) / dlogtem).astype(np.int64) + 1, 1, nr - 1)
        t1, t2 = logtem0 + (ix - 1).astype(np.float64) * dlogtem, logtem0 + ix.astype(np.float64) * dlogtem
        w = (lt - t1) / (t2 - t1)
        ions = (hii, heii, heiii)
        R = [(g[r][ix - 1] * (1.0 - w) + g[r][ix] * w) * (ions[r] * de) for r in range(3)]
        Rmax = [np.maximum(g[r][ix - 1], g[r][ix]) * (ions[r] * de) for r in range(3)]
        E = np.stack([share[2, j] * R[2] + share[1, j] * R[1] + share[0, j] * R[0] for j in range(3)])
        Emax = np.stack([share[2, j] * Rmax[2] + share[1, j] * Rmax[1] + share[0, j] * Rmax[0] for j in range(3)])
        D = capture(hi, hei, heii, ksi)
        S = np.where(D == 0.0, 0.0, E / (D * PI * 4.0))
        scale = np.where(D == 0.0, 0.0, Emax / (D * PI * 4.0))
    return S, E, D, int(np.count_nonzero((E > 0) & (D == 0))), scale


# ---- the inputs the CPU and the GPU tests share ----------------------------------------------------------------------------

_tables = None


def tables():
    """on the goldens' temperature grid (5000 nodes, 1 .. 1e8 K): g[3][5000] of ground_recombination_tables, the case-A and case-B rate
    coefficients, the grid, and ksi of the reference's slopes.  Host code of libftte.so."""
    global _tables
    if _tables is None:
        import radiativetransfer_amd as rt
        ka, a, b, c = rt.rate_coefficient_tables(recombination_type=1)
        kb = rt.rate_coefficient_tables(recombination_type=2)[0]
        beta, ksi, _ = rt.uvb_beta_table([1.8, 1.5, 1.2])
        _tables = dict(g=rt.ground_recombination_tables(), ka=ka, kb=kb, grid=(a, b, c), ksi=ksi, beta=beta)
    return _tables


def medium(golden, name):
    """rho, tgas, HI, HeI, HeII and the grid arguments (n, level, box) of one of the three media of the tests"""
    if name == "wide":
        import _thermal
        n, level, box, rho, tgas, HI, HeI, HeII = _thermal.wide_medium(None)["head"]
    else:
        g = golden(name)
        n, level, box, rho, tgas, HI, HeI, HeII = int(g["n"]), g["level"], float(g["box"]), g["rho"], g["tgas"], g["HI"], g["HeI"], g["HeII"]
    return dict(n=n, level=level, box=box, rho=rho, tgas=tgas, HI=HI, HeI=HeI, HeII=HeII)


MEDIA = ["chem_uvb_refined", "initial_refined", "wide"]
