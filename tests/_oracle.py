"""ctypes view of oracle/libftte_oracle.so -- test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
LIB = os.path.join(ORACLE_DIR, "libftte_oracle.so")

ARITH_REFERENCE, ARITH_DEVICE, ARITH_EXACT = 0, 1, 2
ORDER_SERIAL, ORDER_CLASSED = 0, 1


class Pattern(C.Structure):
    _fields_ = [(n, C.c_double) for n in
                ("xy_x0", "xy_y0", "xy_len", "xz_x0", "xz_z0", "xz_len", "yz_y0", "yz_z0", "yz_len")] + \
               [(n, C.c_int32) for n in ("xz_active", "yz_active", "xy_top", "xz_top", "yz_top", "pad_")]


def build():
    src = [os.path.join(ORACLE_DIR, f) for f in ("ftte_oracle.c", "ftte_oracle_point.c", "ftte_oracle.h")]
    src += [os.path.join(ROOT, "radiativetransfer_amd", "csrc", f) for f in ("ftte_math.h", "ftte_chem_math.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in src):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "-B", "libftte_oracle.so"], stdout=subprocess.DEVNULL)


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        L.fo_pi.restype = L.fo_half_pi.restype = L.fo_two_pi.restype = C.c_double
        L.fo_rotate_indices.argtypes = [C.c_int] * 7 + [ip, ip, ip]
        L.fo_pix2ang_nest.argtypes = [C.c_int, C.c_int64, dp, dp]
        L.fo_fold_direction.argtypes = [C.c_double, C.c_double, dp, dp, ip]
        L.fo_set_pattern.argtypes = [C.POINTER(Pattern), C.c_double, C.c_double]
        L.fo_layer_patterns.argtypes = [C.c_int, C.c_double, C.c_double, C.POINTER(Pattern)]
        L.fo_diffuse_sweep_uniform.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.c_double, C.c_int, dp, dp, dp, dp, dp,
                                               C.c_int, C.c_int, dp]
        L.fo_diffuse_sweep_tree.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_int32), C.c_int, dp, dp, dp, C.c_double,
                                            C.c_int, dp, dp, dp, dp, dp, C.c_int, C.c_int, dp]
        L.fo_compute_opacities.argtypes = [C.c_int64, C.c_int, dp, dp, dp, dp, dp]
        L.fo_compute_opacities.restype = None
        L.fo_device_attenuation.argtypes = [C.c_int64, dp, dp, dp]
        L.fo_device_attenuation.restype = None
        L.fo_device_cell_mean.argtypes = [C.c_int64, dp, C.c_int, C.c_double, dp]
        L.fo_device_cell_mean.restype = None
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def rotate_indices(i, j, k, nx, ny, nz, izone):
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    rc = lib().fo_rotate_indices(i, j, k, nx, ny, nz, izone, C.byref(a), C.byref(b), C.byref(c))
    if rc:
        raise ValueError("bad izone")
    return a.value, b.value, c.value


def pix2ang_nest(nside, ipix):
    p, t = C.c_double(), C.c_double()
    rc = lib().fo_pix2ang_nest(nside, ipix, C.byref(p), C.byref(t))
    if rc:
        raise ValueError(f"fo_pix2ang_nest -> {rc}")
    return p.value, t.value


def healpix_directions(level, count=None):
    """Rotated NESTED pixel centres of angular level `level` (12*4^(level-1) pixels),
    equal weights 1/count (equiSources.f90:1385-1391)."""
    nside = 2 ** (level - 1)
    npix = 12 * nside * nside
    count = npix if count is None else count
    ang = np.array([pix2ang_nest(nside, i) for i in range(count)])
    return ang[:, 0].copy(), ang[:, 1].copy(), np.full(count, 1.0 / count)


def fold_direction(phi, theta):
    p, t, z = C.c_double(), C.c_double(), C.c_int()
    rc = lib().fo_fold_direction(phi, theta, C.byref(p), C.byref(t), C.byref(z))
    if rc:
        raise ValueError(f"fo_fold_direction -> {rc}")
    return p.value, t.value, z.value


def layer_patterns(n, phi, theta):
    arr = (Pattern * n)()
    rc = lib().fo_layer_patterns(n, phi, theta, arr)
    if rc:
        raise ValueError(f"fo_layer_patterns -> {rc}")
    return arr


def sweep_uniform(n, kappa, box, phi, theta, w, uvb, eta=None, src=None, arith=ARITH_REFERENCE, order=ORDER_SERIAL,
                  with_noise=False):
    kappa = _f64(kappa)
    nnu = kappa.shape[0]
    assert kappa.shape == (nnu, n ** 3)
    phi, theta, w, uvb = map(_f64, (phi, theta, w, uvb))
    J = np.empty_like(kappa)
    eta = _f64(eta) if eta is not None else None
    src = _f64(src) if src is not None else None
    eta_p = _dp(eta) if eta is not None else None
    src_p = _dp(src) if src is not None else None
    noise = np.empty_like(kappa) if with_noise else None
    rc = lib().fo_diffuse_sweep_uniform(n, nnu, _dp(kappa), eta_p, src_p, box, len(phi), _dp(phi), _dp(theta), _dp(w),
                                        _dp(uvb), _dp(J), arith, order, _dp(noise) if with_noise else None)
    if rc:
        raise ValueError(f"fo_diffuse_sweep_uniform -> {rc}")
    return (J, noise) if with_noise else J


def oracle_threads():
    """Threads sweep_uniform_parallel may use: the CPUs this process may run on, at most 16."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def sweep_uniform_parallel(n, kappa, box, phi, theta, w, uvb, arith=ARITH_REFERENCE, threads=None):
    """sweep_uniform spread over threads (the library has no mutable globals; ctypes lets go of the GIL during the call).
    Split by frequency group first -- groups never meet, so that alone gives the bits of one call; with fewer groups than
    threads each group's directions are also cut into blocks of consecutive directions, swept apart and added in block order
    -- one call's J to the rounding of that sum (SUM_RTOL)."""
    from concurrent.futures import ThreadPoolExecutor
    lib()                                   # built and loaded once, before the threads
    kappa = _f64(kappa)
    nnu = kappa.shape[0]
    phi, theta, w, uvb = map(_f64, (phi, theta, w, uvb))
    threads = oracle_threads() if threads is None else max(1, min(int(threads), oracle_threads()))
    nblk = max(1, min(len(phi), threads // nnu if nnu < threads else 1))
    cuts = [len(phi) * b // nblk for b in range(nblk + 1)]
    jobs = [(g, cuts[b], cuts[b + 1]) for g in range(nnu) for b in range(nblk)]

    def one(job):
        g, lo, hi = job
        return sweep_uniform(n, kappa[g:g + 1], box, phi[lo:hi], theta[lo:hi], w[lo:hi], uvb[g:g + 1], arith=arith)[0]

    with ThreadPoolExecutor(max_workers=min(threads, len(jobs))) as pool:
        parts = list(pool.map(one, jobs))
    J = np.empty_like(kappa)
    for g in range(nnu):
        J[g] = parts[g * nblk]
        for b in range(1, nblk):
            J[g] += parts[g * nblk + b]
    return J


def sweep_tree(n, level, kappa, box, phi, theta, w, uvb, eta=None, src=None, arith=ARITH_REFERENCE, order=ORDER_SERIAL,
               with_noise=False):
    kappa = _f64(kappa)
    level = np.ascontiguousarray(level, dtype=np.int32)
    nnu, ncell = kappa.shape
    assert ncell == len(level)
    phi, theta, w, uvb = map(_f64, (phi, theta, w, uvb))
    J = np.empty_like(kappa)
    noise = np.empty_like(kappa) if with_noise else None
    eta = _f64(eta) if eta is not None else None
    src = _f64(src) if src is not None else None
    rc = lib().fo_diffuse_sweep_tree(n, ncell, level.ctypes.data_as(C.POINTER(C.c_int32)), nnu, _dp(kappa),
                                     _dp(eta) if eta is not None else None, _dp(src) if src is not None else None, box,
                                     len(phi), _dp(phi), _dp(theta), _dp(w), _dp(uvb), _dp(J), arith, order,
                                     _dp(noise) if with_noise else None)
    if rc:
        raise ValueError(f"fo_diffuse_sweep_tree -> {rc}")
    return (J, noise) if with_noise else J


def compute_opacities(HI, HeI, HeII, beta):
    HI, HeI, HeII, beta = map(_f64, (HI, HeI, HeII, beta))
    nnu = beta.shape[1]
    kappa = np.empty((nnu, len(HI)))
    lib().fo_compute_opacities(len(HI), nnu, _dp(HI), _dp(HeI), _dp(HeII), _dp(beta), _dp(kappa))
    return kappa


def device_attenuation(tau):
    tau = _f64(tau)
    e, g = np.empty_like(tau), np.empty_like(tau)
    lib().fo_device_attenuation(tau.size, _dp(tau), _dp(e), _dp(g))
    return e, g


def device_segment_source(Iin, tau, src):
    """ftte_segment_source element-wise (a source function S, the exact path mean): returns (Iout, mean)."""
    I = np.array(Iin, dtype=np.float64, copy=True)
    tau, src = (_f64(np.broadcast_to(a, I.shape)) for a in (tau, src))
    mean = np.empty_like(I)
    dp = C.POINTER(C.c_double)
    lib().fo_device_segment_source.argtypes = [C.c_int64, dp, dp, dp, dp]
    lib().fo_device_segment_source.restype = None
    lib().fo_device_segment_source(I.size, _dp(I), _dp(tau), _dp(src), _dp(mean))
    return I, mean


def device_segment_emit(Iin, tau, eta, src):
    """ftte_segment_emit element-wise: returns (Iout, mean)."""
    I = np.array(Iin, dtype=np.float64, copy=True)
    tau, eta, src = (_f64(np.broadcast_to(a, I.shape)) for a in (tau, eta, src))
    mean = np.empty_like(I)
    dp = C.POINTER(C.c_double)
    lib().fo_device_segment_emit.argtypes = [C.c_int64, dp, dp, dp, dp, dp]
    lib().fo_device_segment_emit.restype = None
    lib().fo_device_segment_emit(I.size, _dp(I), _dp(tau), _dp(eta), _dp(src), _dp(mean))
    return I, mean


def device_log(x):
    x = _f64(x)
    out = np.empty_like(x)
    lib().fo_device_log.argtypes = [C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib().fo_device_log.restype = None
    lib().fo_device_log(x.size, _dp(x), _dp(out))
    return out


def device_cell_mean(acc, nseg, w):
    acc = _f64(acc)
    out = np.empty_like(acc)
    lib().fo_device_cell_mean(acc.size, _dp(acc), nseg, w, _dp(out))
    return out


# ---- point sources ------------------------------------------------------------------------------------------------------
NT = 11 ** 4


def stellar_beta_table(a_smc, wavelength, spec, iSpectrum, coefSpectrum, iMetal, coefMetal, with_sigma=False):
    a_smc, wavelength, spec = _f64(a_smc), _f64(wavelength), _f64(spec)
    tables = np.empty((6, NT))
    total = C.c_double()
    sig = np.empty((4, 300)) if with_sigma else None
    L = lib()
    L.fo_stellar_beta_table.restype = None
    L.fo_stellar_beta_table.argtypes = [C.POINTER(C.c_double)] * 3 + [C.c_int, C.c_double, C.c_int, C.c_double,
                                                                       C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                                       C.POINTER(C.c_double)]
    L.fo_stellar_beta_table(_dp(a_smc), _dp(wavelength), _dp(spec), iSpectrum, coefSpectrum, iMetal, coefMetal, _dp(tables),
                            C.byref(total), _dp(sig) if with_sigma else None)
    return (tables, total.value, sig) if with_sigma else (tables, total.value)


def get_rates(tables, dust, reaction, tau):
    L = lib()
    L.fo_get_rates.restype = None
    L.fo_get_rates.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int] + [C.c_double] * 4 + [C.POINTER(C.c_double)] * 2
    nr, hr = C.c_double(), C.c_double()
    tables = _f64(tables)
    L.fo_get_rates(_dp(tables), dust, reaction, *[float(t) for t in tau], C.byref(nr), C.byref(hr))
    return nr.value, hr.value


def rmax_table():
    out = np.empty(30)
    lib().fo_rmax.restype = None
    lib().fo_rmax.argtypes = [C.POINTER(C.c_double)]
    lib().fo_rmax(_dp(out))
    return out


def point_sources_escape(n, level, HI, HeI, HeII, rho, abun2, box, dust, src_leaf, src_ndot, tables, out_sigma=None, pix=None):
    """point_sources plus the per-star escape bookkeeping: returns rates, highestPixelLevel, dict(remaining [nsrc][7], boundary
    [nsrc][7], dust [nsrc], spectrum [nsrc][300], fraction [nsrc][7])."""
    level = np.ascontiguousarray(level, dtype=np.int32)
    HI, HeI, HeII, rho, abun2, tables, src_ndot = map(_f64, (HI, HeI, HeII, rho, abun2, tables, src_ndot))
    src_leaf = np.ascontiguousarray(src_leaf, dtype=np.int64)
    nsrc = len(src_leaf)
    rates = np.empty((6, len(level)))
    esc, frac = np.zeros((nsrc, 315)), np.zeros((nsrc, 7))
    hp = C.c_int()
    L = lib()
    dp = C.POINTER(C.c_double)
    L.fo_point_sources_escape.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_int32), dp, dp, dp, dp, dp, C.c_double, C.c_int, C.c_int,
                                          C.POINTER(C.c_int64), dp, dp, dp, C.POINTER(C.c_int), dp, C.c_int, dp, dp, dp]
    pix_levels = 0
    if pix is not None:
        pix_levels = len(pix)
        pix = _f64(np.concatenate([np.asarray(p).reshape(-1, 2) for p in pix]))
    sig = _f64(out_sigma) if out_sigma is not None else None
    rc = L.fo_point_sources_escape(n, len(level), level.ctypes.data_as(C.POINTER(C.c_int32)), _dp(HI), _dp(HeI), _dp(HeII), _dp(rho),
                                   _dp(abun2), box, dust, nsrc, src_leaf.ctypes.data_as(C.POINTER(C.c_int64)), _dp(src_ndot),
                                   _dp(tables), _dp(rates), C.byref(hp), _dp(pix) if pix is not None else None, pix_levels,
                                   _dp(sig) if sig is not None else None, _dp(esc), _dp(frac))
    if rc:
        raise ValueError(f"fo_point_sources_escape -> {rc}")
    return rates, hp.value, dict(remaining=esc[:, :7].copy(), boundary=esc[:, 7:14].copy(), dust=esc[:, 14].copy(),
                                 spectrum=esc[:, 15:].copy(), fraction=frac)


def point_sources(n, level, HI, HeI, HeII, rho, abun2, box, dust, src_leaf, src_ndot, tables, pix=None):
    level = np.ascontiguousarray(level, dtype=np.int32)
    HI, HeI, HeII, rho, abun2, tables, src_ndot = map(_f64, (HI, HeI, HeII, rho, abun2, tables, src_ndot))
    src_leaf = np.ascontiguousarray(src_leaf, dtype=np.int64)
    rates = np.empty((6, len(level)))
    hp = C.c_int()
    L = lib()
    dp = C.POINTER(C.c_double)
    L.fo_point_sources.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_int32), dp, dp, dp, dp, dp, C.c_double, C.c_int, C.c_int,
                                   C.POINTER(C.c_int64), dp, dp, dp, C.POINTER(C.c_int), dp, C.c_int]
    pix_levels = 0
    if pix is not None:
        pix_levels = len(pix)
        pix = _f64(np.concatenate([np.asarray(p).reshape(-1, 2) for p in pix]))
    rc = L.fo_point_sources(n, len(level), level.ctypes.data_as(C.POINTER(C.c_int32)), _dp(HI), _dp(HeI), _dp(HeII), _dp(rho),
                            _dp(abun2), box, dust, len(src_leaf), src_leaf.ctypes.data_as(C.POINTER(C.c_int64)), _dp(src_ndot),
                            _dp(tables), _dp(rates), C.byref(hp), _dp(pix) if pix is not None else None, pix_levels)
    if rc:
        raise ValueError(f"fo_point_sources -> {rc}")
    return rates, hp.value


def _rate_equation_call(name, restype, tail, n, level, box, rho, tgas, HI, HeI, HeII, krate, run_uvb, J, ksi, uniform, threshold, logtem0,
                        logtem9, dlogtem, k):
    """fo_solve_rate_equations' argument list in front of `tail` (ctypes type, value), for it and for the fo_device_ pair"""
    level = np.ascontiguousarray(level, dtype=np.int32)
    rho, tgas, k = _f64(rho), _f64(tgas), _f64(k)
    krate = None if krate is None else _f64(krate)
    J = None if J is None else _f64(J)
    ksi = _f64(ksi if ksi is not None else np.zeros(9))
    uniform = _f64(uniform if uniform is not None else np.zeros(3))
    dp = C.POINTER(C.c_double)
    fn = getattr(lib(), name)
    fn.restype = restype
    fn.argtypes = [C.c_int, C.c_long, C.POINTER(C.c_int32), C.c_double, dp, dp, dp, dp, dp, dp, C.c_int, dp, dp, dp, C.c_double, C.c_int,
                   C.c_double, C.c_double, C.c_double, dp, tail[0]]
    return fn(n, len(level), level.ctypes.data_as(C.POINTER(C.c_int32)), box, _dp(rho), _dp(tgas), _dp(HI), _dp(HeI), _dp(HeII),
              _dp(krate) if krate is not None else None, int(run_uvb), _dp(J) if J is not None else None, _dp(ksi), _dp(uniform),
              float(threshold), k.shape[1], float(logtem0), float(logtem9), float(dlogtem), _dp(k), tail[1])


def solve_rate_equations(n, level, box, rho, tgas, HI, HeI, HeII, krate, run_uvb, J, ksi, uniform, threshold, logtem0, logtem9,
                         dlogtem, k, name="fo_solve_rate_equations"):
    """fo_solve_rate_equations: returns (HI, HeI, HeII, status, bisection steps); status 0 or 1 + first stopping cell."""
    HI, HeI, HeII = (np.array(a, dtype=np.float64, copy=True) for a in (HI, HeI, HeII))
    its = C.c_long()
    st = _rate_equation_call(name, C.c_long, (C.POINTER(C.c_long), C.byref(its)), n, level, box, rho, tgas, HI, HeI, HeII, krate, run_uvb,
                             J, ksi, uniform, threshold, logtem0, logtem9, dlogtem, k)
    return HI, HeI, HeII, int(st), its.value


def device_solve_rate_equations(*args):
    """fo_device_solve_rate_equations, csrc/ftte_chem_math.h on the host: arguments and return as solve_rate_equations; the cells
    at which the reference stops keep their species, the steps are those of the cells that pass (what the kernel counts)."""
    return solve_rate_equations(*args, name="fo_device_solve_rate_equations")


def device_chem_tame(n, level, box, rho, tgas, HI, HeI, HeII, *rest):
    """fo_device_chem_tame: per cell, whether the kernel takes its residuals through the trimmed division; arguments as
    solve_rate_equations."""
    tame = np.empty(len(level), np.int32)
    _rate_equation_call("fo_device_chem_tame", None, (C.POINTER(C.c_int32), tame.ctypes.data_as(C.POINTER(C.c_int32))), n, level, box, rho,
                        tgas, _f64(HI), _f64(HeI), _f64(HeII), *rest)
    return tame.astype(bool)


def device_initial_equilibrium(rho, tgas, HI, HeI, HeII, uniform, threshold, logtem0, logtem9, dlogtem, k, passes=2):
    """fo_device_initial_equilibrium: (HI, HeI, HeII, status, bisection steps of all passes); arguments as
    _initial_equilibrium.initial_equilibrium."""
    rho, tgas, k, uniform = _f64(rho), _f64(tgas), _f64(k), _f64(uniform)
    HI, HeI, HeII = (np.array(a, dtype=np.float64, copy=True) for a in (HI, HeI, HeII))
    dp = C.POINTER(C.c_double)
    fn = lib().fo_device_initial_equilibrium
    fn.restype = C.c_long
    fn.argtypes = [C.c_long, dp, dp, dp, dp, dp, dp, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, dp, C.POINTER(C.c_long)]
    its = C.c_long()
    st = fn(rho.size, _dp(rho), _dp(tgas), _dp(HI), _dp(HeI), _dp(HeII), _dp(uniform), float(threshold), int(passes), k.shape[1],
            float(logtem0), float(logtem9), float(dlogtem), _dp(k), C.byref(its))
    return HI, HeI, HeII, int(st), its.value


def uvb_beta_table(alpha, nfreq=400, freqdel=float(np.float32(0.02))):
    """fo_uvb_beta_table: (beta, ksi, gamma), each [group][3] in the reference's field order (24, 25, 26 / HI, HeI, HeII)."""
    alpha = _f64(alpha)
    out = [np.empty((3, 3)) for _ in range(3)]
    dp = C.POINTER(C.c_double)
    lib().fo_uvb_beta_table.restype = None
    lib().fo_uvb_beta_table.argtypes = [C.c_int, C.c_double, dp, dp, dp, dp]
    lib().fo_uvb_beta_table(nfreq, freqdel, _dp(alpha), *[_dp(a) for a in out])
    return out


def assign_uvb_radiation(HI, HeI, HeII, rho, uvb, threshold):
    HI, HeI, HeII, rho, uvb = map(_f64, (HI, HeI, HeII, rho, uvb))
    J = np.empty((uvb.size, HI.size))
    dp = C.POINTER(C.c_double)
    lib().fo_assign_uvb_radiation.restype = None
    lib().fo_assign_uvb_radiation.argtypes = [C.c_long, C.c_int, dp, dp, dp, dp, dp, C.c_double, dp]
    lib().fo_assign_uvb_radiation(HI.size, uvb.size, _dp(HI), _dp(HeI), _dp(HeII), _dp(rho), _dp(uvb), float(threshold), _dp(J))
    return J


def uniform_table(alpha_quasar, alpha_stellar, nfreq=400, freqdel=float(np.float32(0.02))):
    """fo_uniform_table: (ksi[2][3], gamma[2][3]) for the quasar and stellar components."""
    ksi, gamma = np.empty((2, 3)), np.empty((2, 3))
    dp = C.POINTER(C.c_double)
    lib().fo_uniform_table.restype = None
    lib().fo_uniform_table.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, dp, dp]
    lib().fo_uniform_table(nfreq, freqdel, float(alpha_quasar), float(alpha_stellar), _dp(ksi), _dp(gamma))
    return ksi, gamma


def coll_rates(T, recombination_type):
    k = np.empty(6)
    lib().fo_coll_rates.restype = None
    lib().fo_coll_rates.argtypes = [C.c_double, C.c_int, C.POINTER(C.c_double)]
    lib().fo_coll_rates(float(T), int(recombination_type), _dp(k))
    return k


def rate_coefficient_tables(nratec, temstart, temend, recombination_type):
    k = np.empty((6, nratec))
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    dp = C.POINTER(C.c_double)
    lib().fo_rate_coefficient_tables.restype = None
    lib().fo_rate_coefficient_tables.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, dp, dp, dp, dp]
    lib().fo_rate_coefficient_tables(nratec, float(temstart), float(temend), int(recombination_type), _dp(k), C.byref(a), C.byref(b), C.byref(c))
    return k, a.value, b.value, c.value
