"""Host-side mirror of the reference's diffuse-transfer interface, on top of the C ABI.

The reference has no API object: its driver (equiSources.f90:1372-1808) calls
`computeOpacities`, then per direction `pix2ang_nest`, the folding block, `setPattern`,
`localizeCellFindNeighbours` and `transport`.  The names below follow that vocabulary.
Everything that touches cells runs in libftte.so on the GPU; there is no Python or CPU
implementation of the sweep in this package.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import FtteError, Pattern

__all__ = ["DiffuseTransfer", "StellarTransfer", "rmax", "dust_cross_section", "uvb_beta_table", "uniform_table", "coll_rates", "rate_coefficient_tables", "cooling_coefficient_tables", "FtteError", "Pattern", "pix2ang_nest", "healpix_directions", "fold_direction",
           "rotate_indices", "set_pattern", "layer_patterns", "compute_cell_intensity", "expansion_parameters", "map_axis", "slice_axis", "map_depth", "star_populations", "LYMAN_ALPHA"]


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# A ready `line` of sightline_spectra for HI Lyman alpha at b_turb = 0: sigma_line = (pi e^2 / m_e c) f lambda0 [cm^2 cm/s] with f = 0.4164 and
# lambda0 = 1215.67 A, damping = Gamma lambda0 / 4 pi [cm/s] with Gamma = 6.265e8 / s, the hydrogen atom's mass [g], b_turb [cm/s]
LYMAN_ALPHA = (1.3435e-7, 606.08, 1.6735e-24, 0.0)


def _check(code: int, what: str):
    if code:
        raise FtteError(code, what)


# ---- host geometry: the reference's callable surface ----------------------------------------------------

def rotate_indices(i: int, j: int, k: int, nx: int, ny: int, nz: int, izone: int) -> Tuple[int, int, int]:
    """rotateIndices (rotateIndicesModule.f90:7): sweep indices -> storage indices, 1-based."""
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    _check(_lib.load().ftte_rotate_indices(i, j, k, nx, ny, nz, izone, C.byref(a), C.byref(b), C.byref(c)),
           f"izone {izone} outside 1..24")
    return a.value, b.value, c.value


def _axis(fn, n: int, nmap: int, centre: float, zoom: float):
    base, frac = np.empty(max(nmap, 1), dtype=np.int32), np.empty(max(nmap, 1))
    _check(fn(int(n), int(nmap), float(centre), float(zoom), base.ctypes.data_as(C.POINTER(C.c_int32)), _dp(frac)),
           f"bad map axis: n {n}, nmap {nmap}, centre {centre}, zoom {zoom}")
    return base, frac


def map_axis(n: int, nmap: int, centre: float = 0.5, zoom: float = 1.0):
    """(i0[nmap] 1-based, xnew[nmap]) of the projection's pixel loops (equiSources.f90:703-709); host, no context."""
    return _axis(_lib.load().ftte_map_axis, n, nmap, centre, zoom)


def slice_axis(n: int, nmap: int, centre: float = 0.5, zoom: float = 1.0):
    """(i0[nmap] 1-based, xnew[nmap]) of the reader's pixel loops (readCellArray.f90:126-132) inside a window; host, no context."""
    return _axis(_lib.load().ftte_slice_axis, n, nmap, centre, zoom)


def map_depth(n: int, centre: float = 0.5, zoom: float = 1.0) -> Tuple[int, int]:
    """(kstart, kend) of the projection (equiSources.f90:687-700), 1-based and inclusive; host, no context."""
    a, b = C.c_int32(), C.c_int32()
    _check(_lib.load().ftte_map_depth(int(n), float(centre), float(zoom), C.byref(a), C.byref(b)), f"bad map depth: n {n}, centre {centre}, zoom {zoom}")
    return a.value, b.value


def pix2ang_nest(nside: int, ipix: int) -> Tuple[float, float]:
    """pix2ang_nest + rotateAngles (equiSources.f90:2118, 2297): rotated centre of a NESTED pixel."""
    p, t = C.c_double(), C.c_double()
    _check(_lib.load().ftte_pix2ang_nest(nside, ipix, C.byref(p), C.byref(t)), "nside/ipix out of range")
    return p.value, t.value


def healpix_directions(angular_level: int, count: Optional[int] = None):
    """(phi, theta, weight) of the first `count` pixels of angular level L (12*4^(L-1) pixels),
    equal weights 1/count: the direction loop header of equiSources.f90:1385-1391."""
    nside = 2 ** (angular_level - 1)
    npix = 12 * nside * nside
    count = npix if count is None else count
    if not 0 < count <= npix:
        raise ValueError("count out of range")
    ang = np.array([pix2ang_nest(nside, i) for i in range(count)])
    return ang[:, 0].copy(), ang[:, 1].copy(), np.full(count, 1.0 / count)


def fold_direction(phi: float, theta: float) -> Tuple[float, float, int]:
    """The folding block equiSources.f90:1395-1454: canonical (phi, theta) and izone."""
    p, t, z = C.c_double(), C.c_double(), C.c_int()
    _check(_lib.load().ftte_fold_direction(phi, theta, C.byref(p), C.byref(t), C.byref(z)),
           f"direction ({phi}, {theta}) cannot be folded")
    return p.value, t.value, z.value


def set_pattern(x0: float, y0: float, phi: float, theta: float) -> Pattern:
    """setPattern (transportRoutinesModule.f90:7) for a ray entering the unit cell at (x0, y0)."""
    p = Pattern()
    p.xy_x0, p.xy_y0 = x0, y0
    _check(_lib.load().ftte_set_pattern(C.byref(p), phi, theta), "ray pattern left the unit cell")
    return p


def layer_patterns(n: int, phi: float, theta: float):
    """Patterns of layers 1..n of a folded direction (equiSources.f90:1495-1534)."""
    arr = (Pattern * n)()
    _check(_lib.load().ftte_layer_patterns(n, phi, theta, arr), "ray pattern left the unit cell")
    return arr


def compute_cell_intensity(jmean: float, i_in: float, i_out: float) -> float:
    """computeCellIntensity (transportRoutinesModule.f90:1036): returns the updated Jmean."""
    j = C.c_double(jmean)
    _lib.load().ftte_compute_cell_intensity(C.byref(j), i_in, i_out)
    return j.value


# ---- the sweep ---------------------------------------------------------------------------------------------

class DiffuseTransfer:
    """One GPU's diffuse-transfer engine: the `if (runUVBTransfer)` block of the reference driver.

        rt = DiffuseTransfer(device=0)
        rt.set_grid(n, level, box_cm)            # the cell array (definitionsModule.f90:323-326)
        rt.compute_opacities(HI, HeI, HeII, beta)  # or rt.set_opacity(kappa)
        J = rt.transport(phi, theta, weight, uvb)  # J[nnu][ncell], cell-array order
    """

    def __init__(self, device: Optional[int] = None, devices: Optional[Sequence[int]] = None):
        """device: one HIP ordinal (default: the current device); devices: several ordinals -> ONE context that splits the sweep
        over them (frequency groups first, then directions) and takes host arrays only (include/ftte.h: ftte_create)."""
        self._lib = _lib.load()
        self._ctx = C.c_void_p()
        if devices is not None and len(devices) > 1:
            ids = (C.c_int * len(devices))(*devices)
            code = self._lib.ftte_create(C.byref(self._ctx), len(devices), ids)
        else:
            if devices is not None:
                device = devices[0]
            ids = (C.c_int * 1)(device) if device is not None else None
            code = self._lib.ftte_create(C.byref(self._ctx), 1, ids)
        if code:
            raise FtteError(code, self._lib.ftte_last_error(None).decode())
        self.n = 0
        self.ncell = 0
        self.nnu = 0

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.ftte_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ok(self, code: int):
        if code:
            raise FtteError(code, self._lib.ftte_last_error(self._ctx).decode())

    # -- inputs
    def set_grid(self, n, level: Sequence[int], box_cm: float):
        """n: base grid size (int, or (nx, ny, nz)); level: depth-first leaf levels; box_cm: physicalBoxSize."""
        nx, ny, nz = (n, n, n) if np.isscalar(n) else n
        level = np.ascontiguousarray(level, dtype=np.int32)
        self._ok(self._lib.ftte_set_grid(self._ctx, nx, ny, nz, level.size, level.ctypes.data_as(C.POINTER(C.c_int32)),
                                         float(box_cm)))
        self.n, self.ncell = int(nx), int(level.size)

    def set_uniform_grid(self, n: int, box_cm: float):
        self.set_grid(n, np.zeros(n ** 3, np.int32), box_cm)

    def set_opacity(self, kappa):
        """kappa[nnu][ncell] (numpy, host)."""
        kappa = _f64(kappa)
        if kappa.ndim != 2 or (self.ncell and kappa.shape[1] != self.ncell):
            raise ValueError("kappa must have shape [nnu][ncell]")
        self._ok(self._lib.ftte_set_opacity(self._ctx, kappa.shape[0], _dp(kappa)))
        self.nnu = kappa.shape[0]

    def set_opacity_device(self, nnu: int, device_ptr: int):
        """kappa[nnu][ncell] already in device memory (e.g. torch.Tensor.data_ptr())."""
        self._ok(self._lib.ftte_set_opacity_device(self._ctx, nnu, C.c_void_p(device_ptr)))
        self.nnu = nnu

    def compute_opacities(self, HI, HeI, HeII, beta):
        """computeOpacities (equiSources.f90:4956): beta[3][nnu], rows HI, HeI, HeII."""
        HI, HeI, HeII, beta = map(_f64, (HI, HeI, HeII, beta))
        if beta.ndim != 2 or beta.shape[0] != 3:
            raise ValueError("beta must have shape [3][nnu]")
        self._ok(self._lib.ftte_set_species(self._ctx, beta.shape[1], _dp(HI), _dp(HeI), _dp(HeII), _dp(beta)))
        self.nnu = beta.shape[1]

    def set_emissivity(self, eta=None):
        """The reference's emission term (transportRoutinesModule.f90:676) with eta[nnu][ncell]; None switches it off."""
        eta = None if eta is None else _f64(eta)
        self._ok(self._lib.ftte_set_emissivity(self._ctx, None if eta is None else _dp(eta)))

    def set_source_function(self, S=None):
        """Source function S[nnu][ncell]: Iout = Iin exp(-tau) + S (1 - exp(-tau)) (not in the reference); None: off."""
        S = None if S is None else _f64(S)
        self._ok(self._lib.ftte_set_source_function(self._ctx, None if S is None else _dp(S)))

    def set_emissivity_device(self, device_ptr: int):
        self._ok(self._lib.ftte_set_emissivity_device(self._ctx, C.c_void_p(device_ptr)))

    def set_source_function_device(self, device_ptr: int):
        self._ok(self._lib.ftte_set_source_function_device(self._ctx, C.c_void_p(device_ptr)))

    def set_option(self, key: str, value: int):
        self._ok(self._lib.ftte_set_option(self._ctx, key.encode(), int(value)))

    # -- the sweep
    def transport(self, phi, theta, weight, uvb) -> np.ndarray:
        """One diffuse-transfer iteration; returns J[nnu][ncell] (host)."""
        phi, theta, weight, uvb = map(_f64, (phi, theta, weight, uvb))
        if not (len(phi) == len(theta) == len(weight)) or (self.nnu and len(uvb) != self.nnu):
            raise ValueError("direction arrays must have equal length and uvb one value per frequency group")
        J = np.empty((max(self.nnu, 1), max(self.ncell, 1)))
        self._ok(self._lib.ftte_diffuse_sweep(self._ctx, len(phi), _dp(phi), _dp(theta), _dp(weight), _dp(uvb), _dp(J)))
        return J

    def transport_device(self, phi, theta, weight, uvb, j_device_ptr: int, stream: int = 0):
        """Same with J[nnu][ncell] in device memory; asynchronous on `stream` (a hipStream_t handle, 0 = own)."""
        phi, theta, weight, uvb = map(_f64, (phi, theta, weight, uvb))
        self._ok(self._lib.ftte_diffuse_sweep_device(self._ctx, len(phi), _dp(phi), _dp(theta), _dp(weight), _dp(uvb),
                                                     C.c_void_p(j_device_ptr), C.c_void_p(stream)))

    # -- accelerated source iteration (the build's own: the reference has no enabled emission)
    def lambda_diagonal(self, phi, theta, weight) -> np.ndarray:
        """The diagonal of the Lambda operator of the sweep with a source function, [nnu][ncell] (host): J[c] of a sweep with
        S = 1 in cell c alone and no inflow, for every c at once (include/ftte.h: ftte_lambda_diagonal).  Stale after a new grid,
        new opacities or another direction list."""
        phi, theta, weight = map(_f64, (phi, theta, weight))
        if not (len(phi) == len(theta) == len(weight)):
            raise ValueError("direction arrays must have equal length")
        diag = np.empty((max(self.nnu, 1), max(self.ncell, 1)))
        self._ok(self._lib.ftte_lambda_diagonal(self._ctx, len(phi), _dp(phi), _dp(theta), _dp(weight), _dp(diag)))
        return diag

    def lambda_diagonal_device(self, phi, theta, weight, diag_device_ptr: int, stream: int = 0):
        """Same with the diagonal [nnu][ncell] in device memory; asynchronous on `stream` (0 = own)."""
        phi, theta, weight = map(_f64, (phi, theta, weight))
        if not (len(phi) == len(theta) == len(weight)):
            raise ValueError("direction arrays must have equal length")
        self._ok(self._lib.ftte_lambda_diagonal_device(self._ctx, len(phi), _dp(phi), _dp(theta), _dp(weight),
                                                       C.c_void_p(diag_device_ptr), C.c_void_p(stream)))

    def source_update_device(self, nnu: int, epsilon: float, b_device_ptr: int, b_per_cell: bool, j_device_ptr: int,
                             diag_device_ptr: Optional[int], s_device_ptr: int, stream: int = 0) -> Tuple[float, float]:
        """S <- S + ((1 - eps) J + eps B - S) / (1 - (1 - eps) diag) on device arrays [nnu][ncell] (diag None: the plain
        S <- (1 - eps) J + eps B); returns (max |S_new - S_old|, max |S_new|).  B: [nnu], or [nnu][ncell] with b_per_cell."""
        change = (C.c_double * 2)()
        self._ok(self._lib.ftte_source_update_device(self._ctx, int(nnu), float(epsilon), C.c_void_p(b_device_ptr), int(bool(b_per_cell)),
                                                     C.c_void_p(j_device_ptr), C.c_void_p(diag_device_ptr) if diag_device_ptr else None,
                                                     C.c_void_p(s_device_ptr), change, C.c_void_p(stream)))
        return change[0], change[1]

    def transport_into(self, phi, theta, weight, uvb, J: np.ndarray) -> np.ndarray:
        """Same as transport() into a caller-owned J[nnu][ncell] (e.g. one registered with host_register)."""
        phi, theta, weight, uvb = map(_f64, (phi, theta, weight, uvb))
        if J.dtype != np.float64 or not J.flags.c_contiguous or J.shape != (self.nnu, self.ncell):
            raise ValueError("J must be a C-contiguous float64 array of shape [nnu][ncell]")
        self._ok(self._lib.ftte_diffuse_sweep(self._ctx, len(phi), _dp(phi), _dp(theta), _dp(weight), _dp(uvb), _dp(J)))
        return J

    def iterate_into(self, kappa: np.ndarray, phi, theta, weight, uvb, J: np.ndarray) -> np.ndarray:
        """set_opacity(kappa) + transport_into(..., J) as one call (ftte_diffuse_iteration): on a uniform grid the frequency
        groups cross PCIe and are swept in overlapping lanes."""
        phi, theta, weight, uvb = map(_f64, (phi, theta, weight, uvb))
        kappa = _f64(kappa)
        if kappa.ndim != 2 or kappa.shape[1] != self.ncell:
            raise ValueError("kappa must have shape [nnu][ncell]")
        if J.dtype != np.float64 or not J.flags.c_contiguous or J.shape != kappa.shape:
            raise ValueError("J must be a C-contiguous float64 array of kappa's shape")
        self._ok(self._lib.ftte_diffuse_iteration(self._ctx, kappa.shape[0], _dp(kappa), len(phi), _dp(phi), _dp(theta), _dp(weight),
                                                  _dp(uvb), _dp(J)))
        self.nnu = kappa.shape[0]
        return J

    def host_register(self, a: np.ndarray):
        """Pin a host array the caller keeps (kappa, J): the library then moves it by DMA without a staging copy."""
        self._ok(self._lib.ftte_host_register(self._ctx, C.c_void_p(a.ctypes.data), a.nbytes))

    def host_unregister(self, a: np.ndarray):
        self._ok(self._lib.ftte_host_unregister(self._ctx, C.c_void_p(a.ctypes.data)))

    def multi_info(self) -> str:
        """How the last sweep of a multi-device context combined its devices' J ("" for one device)."""
        return self._lib.ftte_multi_info(self._ctx).decode()

    def counter(self, name: str) -> int:
        """grid_builds / plan_builds / forest_builds: how often the expensive host-side builds ran."""
        return int(self._lib.ftte_counter(self._ctx, name.encode()))

    def launch_records(self):
        """[(ms, updates)] of the sweep-kernel launches of the last sweep (synchronise first)."""
        out = []
        for i in range(self._lib.ftte_launch_count(self._ctx)):
            ms, upd = C.c_double(), C.c_int64()
            self._ok(self._lib.ftte_launch_info(self._ctx, i, C.byref(ms), C.byref(upd)))
            out.append((ms.value, upd.value))
        return out


# ---- point sources ---------------------------------------------------------------------------------------

TABLE_SHAPE = (6, 11, 11, 11, 11)  # reactionRate1..3, energyRate1..3; then [tauDust][tau3][tau2][tau1]
RATE_NAMES = ("krate24", "krate25", "krate26", "crate24", "crate25", "crate26")


def rmax() -> np.ndarray:
    """rmax(1:30) of equiSources.f90:296-309: path length (cells) after which a ray of pixel level L splits."""
    out = np.empty(30)
    _check(_lib.load().ftte_rmax(_dp(out)), "ftte_rmax")
    return out


def uvb_beta_table(alpha, nfreq: int = 400, freqdel: Optional[float] = None):
    """uvbBetaTable (uvbBetaTable.f90): returns (beta[3][3] = [species HI, HeI, HeII][group], ksi[3][3] = [group][24, 25, 26],
    gamma[3][3] = [group][HI, HeI, HeII]) for the three groups' power-law slopes alpha[3].  Defaults: the reference's nfbins
    and frequencyBinWidth (the default-real literal 0.02 widened, definitionsModule.f90:239-241)."""
    alpha = _f64(alpha).reshape(3)
    beta, ksi, gamma = np.empty((3, 3)), np.empty((3, 3)), np.empty((3, 3))
    _check(_lib.load().ftte_uvb_beta_table(int(nfreq), float(np.float32(0.02)) if freqdel is None else float(freqdel), _dp(alpha),
                                           _dp(beta), _dp(ksi), _dp(gamma)), "ftte_uvb_beta_table")
    return beta, ksi, gamma


def coll_rates(T: float, recombination_type: int = 2) -> np.ndarray:
    """coll_rates (coll_rates.f): k1..k6 at temperature T; recombination_type 1 = case A, 2 = case B."""
    k = np.empty(6)
    _check(_lib.load().ftte_coll_rates(float(T), int(recombination_type), _dp(k)), "ftte_coll_rates")
    return k


def rate_coefficient_tables(nratec: int = 5000, temstart: float = 1.0, temend: Optional[float] = None, recombination_type: int = 2):
    """k1a..k6a as the reference's driver tabulates them (calc_rates.f:324-337): returns (k[6][nratec], logtem0, logtem9, dlogtem),
    the arguments of StellarTransfer.set_rate_coefficients.  Defaults: the reference's nratec, temstart, temend = 1.e8 (a default-real
    literal), case B."""
    temend = float(np.float32(1.0e8)) if temend is None else float(temend)
    k = np.empty((6, nratec))
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    _check(_lib.load().ftte_rate_coefficient_tables(int(nratec), float(temstart), temend, int(recombination_type), _dp(k), C.byref(a),
                                                    C.byref(b), C.byref(c)), "ftte_rate_coefficient_tables")
    return k, a.value, b.value, c.value


def cooling_coefficient_tables(nratec: int = 5000, temstart: float = 1.0, temend: Optional[float] = None, recombination_type: int = 2,
                               mellema=None, gnedin=None):
    """The thirteen cooling coefficients as the reference's driver tabulates them (calc_rates.f:414-544) on the temperature grid of
    rate_coefficient_tables, and compa (:619): returns (c[13][nratec], compa), the arguments of
    StellarTransfer.set_cooling_coefficients.  Case B interpolates the reference's two data files, handed over as the files hold
    them: mellema[81][2] = columns 1, 3 of HII-ktbetas.tab, gnedin[201][3] = columns 1, 3, 5 of cratesHe.res; case A (1) needs neither."""
    temend = float(np.float32(1.0e8)) if temend is None else float(temend)
    c, compa = np.empty((13, nratec)), C.c_double()
    if mellema is not None:
        mellema = _f64(mellema)
        if mellema.shape != (81, 2):
            raise ValueError("mellema must have shape [81][2]")
    if gnedin is not None:
        gnedin = _f64(gnedin)
        if gnedin.shape != (201, 3):
            raise ValueError("gnedin must have shape [201][3]")
    _check(_lib.load().ftte_cooling_coefficient_tables(int(nratec), float(temstart), temend, int(recombination_type),
                                                       None if mellema is None else _dp(mellema), None if gnedin is None else _dp(gnedin),
                                                       _dp(c), C.byref(compa)), "ftte_cooling_coefficient_tables")
    return c, compa.value


def ground_recombination_tables(nratec: int = 5000, temstart: float = 1.0, temend: Optional[float] = None) -> np.ndarray:
    """g[3][nratec], the argument of StellarTransfer.set_ground_recombination: the coefficients of recombination to the ground
    states of HI, HeI, HeII on the temperature grid of rate_coefficient_tables, as the difference of the case-A and the case-B fit,
    max(k_A - k_B, 0).  Rows 0 and 2: of k2 and k6.  Row 1: of the RADIATIVE part of k4 alone, coll_rates' case-A
    3.92e-13 / T_eV**0.6353 without the dielectronic term it adds above 0.8 eV -- dielectronic recombination passes through an
    autoionising state and emits no ground-state continuum, and above 1e5 K it would make k4_A - k4_B 15 to 150 times k4_B.  This is
    the build's own choice, not the reference's, which enables no emission and has no such table."""
    temend = float(np.float32(1.0e8)) if temend is None else float(temend)
    ka, logtem0, _, dlogtem = rate_coefficient_tables(nratec, temstart, temend, 1)
    kb = rate_coefficient_tables(nratec, temstart, temend, 2)[0]
    # the tables' temperature nodes (calc_rates.f:324-326) in eV as coll_rates takes them, its literals default-real
    t_ev = np.exp(logtem0 + np.arange(nratec).astype(np.float32).astype(np.float64) * dlogtem) / float(np.float32(11605.0))
    k4_radiative = float(np.float32(3.92e-13)) / t_ev ** float(np.float32(0.6353))
    return np.maximum(np.stack([ka[1] - kb[1], k4_radiative - kb[3], ka[5] - kb[5]]), 0.0)


def uniform_table(alpha_quasar: float, alpha_stellar: float, nfreq: int = 400, freqdel: Optional[float] = None):
    """uniformTable (uniformTable.f90): (ksi[2][3], gamma[2][3]) of the quasar and the stellar power-law component."""
    ksi, gamma = np.empty((2, 3)), np.empty((2, 3))
    _check(_lib.load().ftte_uniform_table(int(nfreq), float(np.float32(0.02)) if freqdel is None else float(freqdel), float(alpha_quasar),
                                          float(alpha_stellar), _dp(ksi), _dp(gamma)), "ftte_uniform_table")
    return ksi, gamma


def dust_cross_section(lambda_micron: float, a_smc) -> float:
    """dustCrossSection (dustModule.f90:30-73), SMC curve; a_smc[7][5] as the rows of the reference's data file."""
    a = np.asfortranarray(_f64(a_smc).reshape(7, 5))
    return float(_lib.load().ftte_dust_cross_section(float(lambda_micron), a.ctypes.data_as(C.POINTER(C.c_double))))


def star_populations(metallicity, abun2) -> dict:
    """The metallicity bracket of every source (equiSources.f90:1282-1293) from its host cell's abun2 and the library's
    metallicity[nmetal] nodes, then one population slot per distinct (iMetal, coefMetal): dict of iMetal[nsrc] (1-based),
    coefMetal[nsrc], slot[nsrc], pop_first[npop] (a source that carries slot p's parameters), pop_iMetal[npop], pop_coefMetal[npop].
    Host only."""
    met, abun2 = _f64(metallicity).reshape(-1), _f64(abun2).reshape(-1)
    ns = abun2.size
    i_metal, slot = np.empty(ns, dtype=np.int32), np.empty(ns, dtype=np.int32)
    coef, first, npop = np.empty(ns), np.empty(max(ns, 1), dtype=np.int64), C.c_int64()
    i32 = C.POINTER(C.c_int32)
    _check(_lib.load().ftte_star_populations(met.size, _dp(met), ns, _dp(abun2), i_metal.ctypes.data_as(i32), _dp(coef),
                                             slot.ctypes.data_as(i32), C.byref(npop), first.ctypes.data_as(C.POINTER(C.c_int64))),
           "ftte_star_populations")
    first = first[:npop.value].copy()
    return dict(iMetal=i_metal, coefMetal=coef, slot=slot, pop_first=first, pop_iMetal=i_metal[first], pop_coefMetal=coef[first])


class StellarTransfer(DiffuseTransfer):
    """The `if (runStellarTransfer)` block of the reference driver (equiSources.f90:1256-1370) on one GPU.

        st = StellarTransfer(device=0)
        st.set_grid(n, level, box_cm)
        st.set_medium(HI, HeI, HeII, rho, abun2, dust_approximation)
        st.set_zero_rates()
        st.stellar_beta_table(a_smc, wavelength_cm, specific_luminosity, iSpectrum, cS, iMetal, cM)
        st.point_sources(cells, ndot)            # the stars of that population
        rates = st.rates()                       # [6][ncell]: krate24, 25, 26, crate24, 25, 26
    """

    def stellar_beta_table(self, a_smc, wavelength_cm, specific_luminosity, i_spectrum: int, coef_spectrum: float,
                           i_metal: int, coef_metal: float) -> float:
        """stellarBetaTable (stellarBetaTable.f90).  specific_luminosity[nmetal][nspectrum][nwave] (log10, as the
        reference's library); i_spectrum, i_metal 1-based.  Returns totalIntegral; the tables stay on the device."""
        a = np.asfortranarray(_f64(a_smc).reshape(7, 5))
        wl = _f64(wavelength_cm)
        sl = _f64(specific_luminosity)
        if sl.ndim != 3 or sl.shape[2] != wl.size:
            raise ValueError("specific_luminosity must have shape [nmetal][nspectrum][nwave]")
        slf = np.asfortranarray(sl)  # the Fortran array specificLuminosity(nmetal, nspectrum, nwave)
        total = C.c_double()
        self._ok(self._lib.ftte_stellar_beta_table(
            self._ctx, a.ctypes.data_as(C.POINTER(C.c_double)), wl.size, _dp(wl), sl.shape[1], sl.shape[0],
            slf.ctypes.data_as(C.POINTER(C.c_double)), int(i_spectrum), float(coef_spectrum), int(i_metal),
            float(coef_metal), C.byref(total)))
        return total.value

    def stellar_beta_tables(self, a_smc, wavelength_cm, specific_luminosity, i_spectrum, coef_spectrum, i_metal,
                            coef_metal) -> np.ndarray:
        """stellarBetaTable for the populations (i_spectrum, coef_spectrum, i_metal, coef_metal)[npop] into population slots
        0..npop-1, replacing earlier slots; each slot holds what stellar_beta_table stores for its population.  Returns
        totalIntegral[npop]; the tables stay on the device."""
        a = np.asfortranarray(_f64(a_smc).reshape(7, 5))
        wl = _f64(wavelength_cm)
        sl = _f64(specific_luminosity)
        if sl.ndim != 3 or sl.shape[2] != wl.size:
            raise ValueError("specific_luminosity must have shape [nmetal][nspectrum][nwave]")
        slf = np.asfortranarray(sl)
        i_s = np.ascontiguousarray(i_spectrum, dtype=np.intc).reshape(-1)
        i_m = np.ascontiguousarray(i_metal, dtype=np.intc).reshape(-1)
        c_s, c_m = _f64(coef_spectrum).reshape(-1), _f64(coef_metal).reshape(-1)
        if not (i_s.size == i_m.size == c_s.size == c_m.size):
            raise ValueError("the four population arrays must have equal length")
        totals = np.empty(i_s.size)
        self._ok(self._lib.ftte_stellar_beta_tables(
            self._ctx, a.ctypes.data_as(C.POINTER(C.c_double)), wl.size, _dp(wl), sl.shape[1], sl.shape[0],
            slf.ctypes.data_as(C.POINTER(C.c_double)), i_s.size, i_s.ctypes.data_as(C.POINTER(C.c_int)), _dp(c_s),
            i_m.ctypes.data_as(C.POINTER(C.c_int)), _dp(c_m), _dp(totals)))
        return totals

    def set_population_tables(self, tables):
        """tables[npop][6][11][11][11][11] computed elsewhere into population slots 0..npop-1, replacing earlier slots."""
        tables = _f64(tables)
        size = int(np.prod(TABLE_SHAPE))
        if tables.size == 0 or tables.size % size:
            raise ValueError("tables must have shape [npop][6][11][11][11][11]")
        self._ok(self._lib.ftte_set_population_tables(self._ctx, tables.size // size, _dp(tables)))

    def population_tables(self, slot: int) -> np.ndarray:
        """The tables of one population slot, [6][11][11][11][11]."""
        out = np.empty(TABLE_SHAPE)
        self._ok(self._lib.ftte_get_population_tables(self._ctx, int(slot), _dp(out)))
        return out

    def population_slots(self) -> int:
        return self.counter("population_slots")

    def set_rate_tables(self, tables):
        tables = _f64(tables)
        if tables.size != int(np.prod(TABLE_SHAPE)):
            raise ValueError("tables must have shape [6][11][11][11][11]")
        self._ok(self._lib.ftte_set_rate_tables(self._ctx, _dp(tables)))

    def rate_tables(self) -> np.ndarray:
        out = np.empty(TABLE_SHAPE)
        self._ok(self._lib.ftte_get_rate_tables(self._ctx, _dp(out)))
        return out

    def get_rates_hydrogen_helium(self, tau, dust_approximation: int = 0) -> np.ndarray:
        """getRatesHydrogenHelium (equiSources.f90:4157) for tau[nsample][4] = (tau1, tau2, tau3, tauDust);
        returns [nsample][3][2] = (numberRate, heatingRate) per reaction, evaluated on the device."""
        tau = _f64(tau).reshape(-1, 4)
        out = np.empty((tau.shape[0], 3, 2))
        self._ok(self._lib.ftte_get_rates_hydrogen_helium(self._ctx, int(dust_approximation), tau.shape[0], _dp(tau), _dp(out)))
        return out

    def set_medium(self, HI, HeI, HeII, rho=None, abun2=None, dust_approximation: int = 0):
        f = [None if a is None else _f64(a) for a in (HI, HeI, HeII, rho, abun2)]
        for a in f:
            if a is not None and self.ncell and a.size != self.ncell:
                raise ValueError("cell fields must have ncell elements")
        self._ok(self._lib.ftte_set_medium(self._ctx, *[None if a is None else _dp(a) for a in f], int(dust_approximation)))

    def set_medium_device(self, HI: int, HeI: int, HeII: int, rho: int = 0, abun2: int = 0, dust_approximation: int = 0):
        self._ok(self._lib.ftte_set_medium_device(self._ctx, *[C.c_void_p(p) if p else None for p in (HI, HeI, HeII, rho, abun2)],
                                                  int(dust_approximation)))

    def set_zero_rates(self):
        """setZeroRates (equiSources.f90:4128)."""
        self._ok(self._lib.ftte_set_zero_rates(self._ctx))

    def locate_cell(self, position: Sequence[int]) -> int:
        """localizeCellFromStar (equiSources.f90:2597): call sequence (1-based) -> 0-based cell-array index."""
        pos = np.ascontiguousarray(position, dtype=np.int32)
        if pos.size % 3 or pos.size < 3:
            raise ValueError("a call sequence has 3 (level + 1) entries")
        cell = C.c_int64()
        self._ok(self._lib.ftte_locate_cell(self._ctx, pos.size // 3 - 1, pos.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(cell)))
        return cell.value

    def star_catalogue(self, xyz, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), weight=None) -> dict:
        """Stars -> host leaves -> one source per leaf (equiSources.f90:746-769, :1169-1212) on the device.  xyz[nstars][3] in
        the units of the box corners lo, hi; weight[nstars] >= 0 (None: 1 each).  Returns star_cell[nstars] (-1 outside the box),
        outside, and per source in ascending cell: cell, weight, ndot = float32(weight), first_star (lowest star index with
        weight > 0 in the leaf), and abun2 where the medium has it.  Stars are merged by host leaf, not by the reference's key."""
        xyz = _f64(xyz).reshape(-1, 3)
        lo, hi = _f64(lo).reshape(3), _f64(hi).reshape(3)
        i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        if weight is not None:
            weight = np.ascontiguousarray(weight, dtype=np.int32).reshape(-1)
            if weight.size != xyz.shape[0]:
                raise ValueError("weight must have one entry per star")
        star_cell = np.empty(xyz.shape[0], dtype=np.int64)
        nsrc, outside = C.c_int64(), C.c_int64()
        self._ok(self._lib.ftte_star_catalogue(self._ctx, xyz.shape[0], _dp(xyz), _dp(lo), _dp(hi),
                                               None if weight is None else weight.ctypes.data_as(i32), star_cell.ctypes.data_as(i64),
                                               C.byref(nsrc), C.byref(outside)))
        ns = nsrc.value
        out = dict(star_cell=star_cell, outside=outside.value, cell=np.empty(ns, dtype=np.int64), weight=np.empty(ns, dtype=np.int32),
                   ndot=np.empty(ns), first_star=np.empty(ns, dtype=np.int64))
        args = (self._ctx, ns, out["cell"].ctypes.data_as(i64), out["weight"].ctypes.data_as(i32), _dp(out["ndot"]),
                out["first_star"].ctypes.data_as(i64))
        if self.counter("medium_abun2") == 1:
            out["abun2"] = np.empty(ns)
        self._ok(self._lib.ftte_star_sources(*args, _dp(out["abun2"]) if "abun2" in out else None))
        return out

    def cell_position(self, cell: int) -> np.ndarray:
        """The call sequence (1-based: base indices, then child indices per level) of a leaf: the inverse of locate_cell."""
        level = C.c_int()
        self._ok(self._lib.ftte_cell_position(self._ctx, int(cell), C.byref(level), None))
        pos = np.empty(3 * (level.value + 1), dtype=np.int32)
        self._ok(self._lib.ftte_cell_position(self._ctx, int(cell), C.byref(level), pos.ctypes.data_as(C.POINTER(C.c_int32))))
        return pos

    def point_sources(self, cells, ndot) -> int:
        """Trace the stars in `cells` (0-based cell-array indices) with photon rates `ndot` through the medium, adding
        to the rates on the device.  Returns highestPixelLevel."""
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        ndot = _f64(ndot)
        if cells.size != ndot.size:
            raise ValueError("cells and ndot must have equal length")
        highest = C.c_int()
        self._ok(self._lib.ftte_point_sources(self._ctx, cells.size, cells.ctypes.data_as(C.POINTER(C.c_int64)), _dp(ndot),
                                              C.byref(highest)))
        return highest.value

    def point_sources_populations(self, cells, ndot, slots) -> np.ndarray:
        """point_sources with star s reading the tables of population slot slots[s] instead of the current tables.  Returns
        each star's own highestPixelLevel."""
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        ndot = _f64(ndot)
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        if cells.size != ndot.size or cells.size != slots.size:
            raise ValueError("cells, ndot and slots must have equal length")
        highest = np.zeros(cells.size, dtype=np.intc)
        self._ok(self._lib.ftte_point_sources_populations(self._ctx, cells.size, cells.ctypes.data_as(C.POINTER(C.c_int64)), _dp(ndot),
                                                          slots.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          highest.ctypes.data_as(C.POINTER(C.c_int))))
        return highest

    def escape(self, nsrc: int) -> dict:
        """Escape bookkeeping of the last point_sources call (equiSources.f90:3198-3233, 1342-1348): dict of remaining [nsrc][7],
        boundary [nsrc][7], dust [nsrc], spectrum [nsrc][300], fraction [nsrc][7]."""
        out = dict(remaining=np.empty((nsrc, 7)), boundary=np.empty((nsrc, 7)), dust=np.empty(nsrc), spectrum=np.empty((nsrc, 300)),
                   fraction=np.empty((nsrc, 7)))
        self._ok(self._lib.ftte_point_escape(self._ctx, nsrc, _dp(out["remaining"]), _dp(out["boundary"]), _dp(out["dust"]),
                                             _dp(out["spectrum"]), _dp(out["fraction"])))
        return out

    def set_output_sigma(self, sigma):
        """outputSigma24, 25, 26, Dust [4][300] for tables handed over with set_rate_tables."""
        sigma = _f64(sigma)
        if sigma.shape != (4, 300):
            raise ValueError("sigma must have shape [4][300]")
        self._ok(self._lib.ftte_set_output_sigma(self._ctx, _dp(sigma)))

    def ray_steps(self) -> int:
        """Cell crossings of the last point_sources call, all rays."""
        return int(self._lib.ftte_point_ray_steps(self._ctx))

    def rates(self) -> np.ndarray:
        out = np.empty((6, max(self.ncell, 1)))
        self._ok(self._lib.ftte_get_point_rates(self._ctx, _dp(out)))
        return out

    def set_rates(self, rates):
        """Replace the device-resident rates (e.g. by their sum over the ranks that traced different stars)."""
        rates = _f64(rates)
        if rates.shape != (6, self.ncell):
            raise ValueError("rates must have shape [6][ncell]")
        self._ok(self._lib.ftte_set_point_rates(self._ctx, _dp(rates)))

    def rates_device_ptr(self) -> int:
        p = C.c_void_p()
        self._ok(self._lib.ftte_point_rates_device(self._ctx, C.byref(p)))
        return p.value

    # -- ionisation equilibrium: solveRateEquations (equiSources.f90:3459-3677) on the device-resident medium
    def set_rate_coefficients(self, logtem0: float, logtem9: float, dlogtem: float, k):
        """k[6][nratec] = k1a..k6a of the reference's calc_rates / coll_rates; table bounds of equiSources.f90:174-176."""
        k = _f64(k)
        if k.ndim != 2 or k.shape[0] != 6:
            raise ValueError("k must have shape [6][nratec]")
        self._ok(self._lib.ftte_set_rate_coefficients(self._ctx, k.shape[1], float(logtem0), float(logtem9), float(dlogtem),
                                                      *[_dp(k[r]) for r in range(6)]))

    def set_temperature(self, tgas):
        tgas = _f64(tgas)
        if self.ncell and tgas.size != self.ncell:
            raise ValueError("tgas must have ncell elements")
        self._ok(self._lib.ftte_set_temperature(self._ctx, _dp(tgas)))

    def _solve(self, fn, J, run_uvb, ksi, uniform, threshold, use_point_rates):
        ksi = None if ksi is None else _f64(ksi).reshape(3, 3)
        uniform = None if uniform is None else _f64(uniform).reshape(3)
        change = C.c_double()
        self._ok(fn(self._ctx, int(bool(run_uvb)), J, None if ksi is None else _dp(ksi), None if uniform is None else _dp(uniform),
                    float(threshold), int(bool(use_point_rates)), C.byref(change)))
        return change.value

    def solve_rate_equations(self, run_uvb: bool, J=None, ksi=None, uniform=None, threshold: float = 0.0,
                             use_point_rates: bool = False) -> float:
        """One equilibrium update of HI, HeI, HeII in the device-resident medium; J[3][ncell] host array (run_uvb) or the
        uniform background rates.  Returns the largest change of a species fraction."""
        J = None if J is None else _f64(J)
        if J is not None and J.shape != (3, self.ncell):
            raise ValueError("J must have shape [3][ncell]")
        return self._solve(self._lib.ftte_solve_rate_equations, None if J is None else _dp(J), run_uvb, ksi, uniform, threshold,
                           use_point_rates)

    def solve_rate_equations_device(self, j_device_ptr: int, ksi, use_point_rates: bool = False) -> float:
        """Same with J[3][ncell] in device memory (e.g. what transport_device wrote)."""
        return self._solve(self._lib.ftte_solve_rate_equations_device, C.c_void_p(j_device_ptr), True, ksi, None, 0.0, use_point_rates)

    # -- time-dependent ionisation: the same rates, the species advanced over dt instead of replaced by their equilibrium
    def advance_rate_equations(self, dt: float, run_uvb: bool, J=None, ksi=None, uniform=None, threshold: float = 0.0,
                               use_point_rates: bool = False, substeps: int = 1) -> float:
        """HI, HeI, HeII of the device-resident medium advanced over dt seconds in `substeps` implicit steps at the rates of the
        state on entry (arguments as solve_rate_equations).  Returns the largest change of a species fraction."""
        J = None if J is None else _f64(J)
        if J is not None and J.shape != (3, self.ncell):
            raise ValueError("J must have shape [3][ncell]")
        fn = self._lib.ftte_advance_rate_equations
        return self._solve(lambda ctx, *rest: fn(ctx, float(dt), int(substeps), *rest), None if J is None else _dp(J), run_uvb, ksi, uniform,
                           threshold, use_point_rates)

    def advance_rate_equations_device(self, dt: float, j_device_ptr: int, ksi, use_point_rates: bool = False, substeps: int = 1) -> float:
        """Same with J[3][ncell] in device memory (e.g. what transport_device wrote)."""
        fn = self._lib.ftte_advance_rate_equations_device
        return self._solve(lambda ctx, *rest: fn(ctx, float(dt), int(substeps), *rest), C.c_void_p(j_device_ptr), True, ksi, None, 0.0,
                           use_point_rates)

    # -- thermal balance: thermalEquilibrium (equiSources.f90:3870-4042) and the temperature advanced over dt
    def set_cooling_coefficients(self, c, compa: float, redshift: float):
        """c[13][nratec] and compa of cooling_coefficient_tables, on the temperature grid of set_rate_coefficients (call that
        first); redshift: currentRedshift of the Compton term."""
        c = _f64(c)
        if c.ndim != 2 or c.shape[0] != 13:
            raise ValueError("c must have shape [13][nratec]")
        self._ok(self._lib.ftte_set_cooling_coefficients(self._ctx, c.shape[1], _dp(c), float(compa), float(redshift)))

    def temperature(self) -> np.ndarray:
        """tgas per leaf as it stands on the device."""
        out = np.empty(max(self.ncell, 1))
        self._ok(self._lib.ftte_get_temperature(self._ctx, _dp(out)))
        return out

    def _thermal_rates(self, J, run_uvb, gamma, uniform_gamma, threshold, use_point_rates):
        gamma = None if gamma is None else _f64(gamma).reshape(3, 3)
        uniform_gamma = None if uniform_gamma is None else _f64(uniform_gamma).reshape(3)
        return (int(bool(run_uvb)), J, None if gamma is None else _dp(gamma), None if uniform_gamma is None else _dp(uniform_gamma),
                float(threshold), int(bool(use_point_rates))), (gamma, uniform_gamma)

    def _host_J(self, J):
        J = None if J is None else _f64(J)
        if J is not None and J.shape != (3, self.ncell):
            raise ValueError("J must have shape [3][ncell]")
        return J

    def thermal_equilibrium(self, run_uvb: bool = False, J=None, gamma=None, uniform_gamma=None, threshold: float = 0.0,
                            use_point_rates: bool = False, j_device_ptr: Optional[int] = None):
        """thermalEquilibrium for every leaf: returns (heating, cooling, hydroHeating) [erg/(s cm^3)]; hydroHeating stays on the
        device for advance_temperature(hydro_heating=True).  J[3][ncell] (or j_device_ptr) with gamma[3][3] of uvb_beta_table, or
        uniform_gamma[3] = the gammas of HI, HeII, HeI of the uniform background behind the self-shielding threshold."""
        J = self._host_J(J)
        out = [np.empty(max(self.ncell, 1)) for _ in range(3)]
        fn = self._lib.ftte_thermal_equilibrium if j_device_ptr is None else self._lib.ftte_thermal_equilibrium_device
        Jarg = (None if J is None else _dp(J)) if j_device_ptr is None else C.c_void_p(j_device_ptr)
        args, keep = self._thermal_rates(Jarg, run_uvb, gamma, uniform_gamma, threshold, use_point_rates)
        self._ok(fn(self._ctx, *args, *[_dp(a) for a in out]))
        return tuple(out)

    def advance_temperature(self, dt: float, run_uvb: bool = False, J=None, gamma=None, uniform_gamma=None, threshold: float = 0.0,
                            use_point_rates: bool = False, substeps: int = 1, tmin: float = 1.0, tmax: float = 1.0e9,
                            hydro_heating: bool = False) -> float:
        """The temperature of every leaf advanced over dt seconds in `substeps` implicit steps at fixed species and at the rates of
        the state on entry (arguments as thermal_equilibrium), clipped to [tmin, tmax]; hydro_heating adds the hydroHeating of the
        last thermal_equilibrium.  Returns the largest |T1 - T0| / T0."""
        J = self._host_J(J)
        args, keep = self._thermal_rates(None if J is None else _dp(J), run_uvb, gamma, uniform_gamma, threshold, use_point_rates)
        change = C.c_double()
        self._ok(self._lib.ftte_advance_temperature(self._ctx, float(dt), int(substeps), float(tmin), float(tmax), int(bool(hydro_heating)), *args,
                                                    C.byref(change)))
        return change.value

    def advance_temperature_device(self, dt: float, j_device_ptr: int, gamma, use_point_rates: bool = False, substeps: int = 1,
                                   tmin: float = 1.0, tmax: float = 1.0e9, hydro_heating: bool = False) -> float:
        """Same with J[3][ncell] in device memory (e.g. what transport_device wrote)."""
        args, keep = self._thermal_rates(C.c_void_p(j_device_ptr), True, gamma, None, 0.0, use_point_rates)
        change = C.c_double()
        self._ok(self._lib.ftte_advance_temperature_device(self._ctx, float(dt), int(substeps), float(tmin), float(tmax), int(bool(hydro_heating)),
                                                           *args, C.byref(change)))
        return change.value

    # -- species and temperature together over dt, each leaf in subcycles of its own (csrc/ftte_thermochem_math.h)
    def _thermochemistry(self, fn, dt, eta, max_subcycles, tmin, tmax, hydro_heating, Jarg, run_uvb, ksi, gamma, uniform, uniform_gamma, threshold,
                         use_point_rates):
        tables = [None if a is None else _f64(a).reshape(shape) for a, shape in ((ksi, (3, 3)), (gamma, (3, 3)), (uniform, 3), (uniform_gamma, 3))]
        ptr = [None if a is None else _dp(a) for a in tables]
        change = (C.c_double * 2)()
        sub = (C.c_int64 * 3)()
        self._ok(fn(self._ctx, float(dt), float(eta), int(max_subcycles), float(tmin), float(tmax), int(bool(hydro_heating)), int(bool(run_uvb)), Jarg,
                    *ptr, float(threshold), int(bool(use_point_rates)), change, sub))
        return dict(species_change=change[0], temperature_change=change[1], subcycles=int(sub[0]), largest=int(sub[1]), capped=int(sub[2]))

    def advance_thermochemistry(self, dt: float, run_uvb: bool = False, J=None, ksi=None, gamma=None, uniform=None, uniform_gamma=None,
                                threshold: float = 0.0, use_point_rates: bool = False, eta: float = 0.1, max_subcycles: int = 64,
                                tmin: float = 1.0, tmax: float = 1.0e9, hydro_heating: bool = False) -> dict:
        """HI, HeI, HeII and T of every leaf advanced together over dt seconds: per leaf, the chemistry's and the temperature's implicit
        steps in turn over subcycles of h = min(remaining, max(eta tau, remaining / (max_subcycles - s))), tau the leaf's own time scale
        (eta = 0: max_subcycles equal subcycles).  Rates as advance_rate_equations (ksi, uniform) and advance_temperature (gamma,
        uniform_gamma) take them, held fixed over the call.  Returns dict(species_change, temperature_change -- the largest of each --,
        subcycles -- summed over the leaves --, largest -- of a leaf --, capped -- leaves the cap bounded)."""
        J = self._host_J(J)
        return self._thermochemistry(self._lib.ftte_advance_thermochemistry, dt, eta, max_subcycles, tmin, tmax, hydro_heating,
                                     None if J is None else _dp(J), run_uvb, ksi, gamma, uniform, uniform_gamma, threshold, use_point_rates)

    def advance_thermochemistry_device(self, dt: float, j_device_ptr: int, ksi, gamma, use_point_rates: bool = False, eta: float = 0.1,
                                       max_subcycles: int = 64, tmin: float = 1.0, tmax: float = 1.0e9, hydro_heating: bool = False) -> dict:
        """Same with J[3][ncell] in device memory (e.g. what transport_device wrote)."""
        return self._thermochemistry(self._lib.ftte_advance_thermochemistry_device, dt, eta, max_subcycles, tmin, tmax, hydro_heating,
                                     C.c_void_p(j_device_ptr), True, ksi, gamma, None, None, 0.0, use_point_rates)

    def subcycles(self) -> np.ndarray:
        """int32 per leaf: the subcycles it took in the last advance_thermochemistry that got through."""
        out = np.empty(max(self.ncell, 1), dtype=np.int32)
        self._ok(self._lib.ftte_get_subcycles(self._ctx, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    # -- diffuse recombination radiation: a source function from the gas state (csrc/ftte_recombination_math.h)
    def set_ground_recombination(self, g):
        """g[3][nratec] of ground_recombination_tables (or the caller's own): the coefficients of recombination to the ground states
        of HI, HeI, HeII on the temperature grid of set_rate_coefficients (call that first)."""
        g = _f64(g)
        if g.ndim != 2 or g.shape[0] != 3:
            raise ValueError("g must have shape [3][nratec]")
        self._ok(self._lib.ftte_set_ground_recombination(self._ctx, g.shape[1], _dp(g)))

    def _recombination(self, fn, ksi, share, S):
        ksi, share = _f64(ksi).reshape(3, 3), _f64(share).reshape(3, 3)
        lost = C.c_int64()
        self._ok(fn(self._ctx, _dp(ksi), _dp(share), S, C.byref(lost)))
        return int(lost.value)

    def recombination_source(self, ksi, share, want_S: bool = True):
        """The source function of the ground-state recombination photons from the device-resident gas state, written into the
        context's emission field: the next transport carries it, exactly as after set_source_function with the same values.
        ksi[3][3] = [group][ksi24, ksi25, ksi26]; share[3][3] = [ion HII, HeII, HeIII recombining][group], entries in [0, 1], row
        sums <= 1.  Needs the medium with rho, the temperature, the rate coefficients, set_ground_recombination and opacities in
        three groups.  Returns (S[3][ncell] or None, lost): lost counts the (leaf, group) pairs that emit where nothing absorbs."""
        S = np.empty((3, max(self.ncell, 1))) if want_S else None
        lost = self._recombination(self._lib.ftte_recombination_source, ksi, share, None if S is None else _dp(S))
        return S, lost

    def recombination_source_device(self, ksi, share, s_device_ptr: int = 0) -> int:
        """Same; a copy of S[3][ncell] goes to device memory at s_device_ptr unless that is 0.  Returns lost."""
        return self._recombination(self._lib.ftte_recombination_source_device, ksi, share, C.c_void_p(s_device_ptr) if s_device_ptr else None)

    def medium(self):
        out = [np.empty(max(self.ncell, 1)) for _ in range(3)]
        self._ok(self._lib.ftte_get_medium(self._ctx, *[_dp(a) for a in out]))
        return out

    def compute_opacities_from_medium(self, beta):
        """computeOpacities (equiSources.f90:4956) on the device-resident HI, HeI, HeII; beta[3][nnu]."""
        beta = _f64(beta)
        if beta.ndim != 2 or beta.shape[0] != 3:
            raise ValueError("beta must have shape [3][nnu]")
        self._ok(self._lib.ftte_compute_opacities(self._ctx, beta.shape[1], _dp(beta)))
        self.nnu = beta.shape[1]

    def assign_uvb_radiation(self, uvb, threshold: float) -> np.ndarray:
        """assignUvbRadiation (transportRoutinesModule.f90:1056): J[nnu][ncell] = uvb where the medium is not self-shielded."""
        uvb = _f64(uvb)
        J = np.empty((uvb.size, max(self.ncell, 1)))
        self._ok(self._lib.ftte_assign_uvb_radiation(self._ctx, uvb.size, _dp(uvb), float(threshold), _dp(J)))
        return J

    def rate_equation_steps(self) -> int:
        return int(self._lib.ftte_rate_equation_steps(self._ctx))

    # -- the start-up equilibrium (equiSources.f90:1008-1022) and computeMass (:4369-4393)
    def initial_ionization_equilibrium(self, uniform, threshold: float, passes: int = 2) -> float:
        """initialIonizationEquilibrium `passes` times per leaf on the device-resident medium, uniform[3] the background rates
        behind the self-shielding threshold.  Returns neutralHydrogenMass / totalHydrogenMass of the result."""
        uniform = _f64(uniform).reshape(3)
        frac = C.c_double()
        self._ok(self._lib.ftte_initial_ionization_equilibrium(self._ctx, _dp(uniform), float(threshold), int(passes), C.byref(frac)))
        return frac.value

    def hydrogen_mass(self) -> Tuple[float, float]:
        """(neutralHydrogenMass, totalHydrogenMass) [msun] of the device-resident medium."""
        neutral, total = C.c_double(), C.c_double()
        self._ok(self._lib.ftte_hydrogen_mass(self._ctx, C.byref(neutral), C.byref(total)))
        return neutral.value, total.value

    # -- the start-up expansion of HII regions (equiSources.f90:1035-1069; off in the shipped reference, expansionFlag)
    @staticmethod
    def expansion_parameters(nh: float) -> Tuple[float, float]:
        """computeExpansionParameters(nh) (equiSources.f90:4395): (finalRadius [cm], densityCoefficient); host, no context."""
        radius, coef = C.c_double(), C.c_double()
        _check(_lib.load().ftte_expansion_parameters(float(nh), C.byref(radius), C.byref(coef)), "ftte_expansion_parameters")
        return radius.value, coef.value

    def expand_hii_regions(self, src_cells, params=None, want_rho_coef: bool = True) -> Tuple[Optional[np.ndarray], int]:
        """findExpansion for every star and leaf, then applyExpansion, on the device-resident medium: src_cells are the host
        leaves of the stars with weight > 0 (locate_cell); params[nsrc][3] = finalRadius [cm], densityCoefficient,
        sourceTotalHydrogenDensity per star, or None to have them computed from the host leaves' densities.  Returns
        (rhoCoef[ncell], number of leaves with rhoCoef < 1); want_rho_coef = False leaves rhoCoef on the device and returns None
        in its place."""
        cells = np.ascontiguousarray(src_cells, dtype=np.int64).reshape(-1)
        if params is not None:
            params = _f64(params)
            if params.shape != (cells.size, 3):
                raise ValueError("params must have shape [nsrc][3]")
        coef = np.empty(max(self.ncell, 1)) if want_rho_coef else None
        changed = C.c_int64()
        self._ok(self._lib.ftte_expand_hii_regions(self._ctx, cells.size, cells.ctypes.data_as(C.POINTER(C.c_int64)),
                                                   None if params is None else _dp(params), None if coef is None else _dp(coef),
                                                   C.byref(changed)))
        return coef, changed.value

    def density(self) -> np.ndarray:
        """rho of the device-resident medium."""
        out = np.empty(max(self.ncell, 1))
        self._ok(self._lib.ftte_get_density(self._ctx, _dp(out)))
        return out

    # -- analysis: the reference's ways of looking at a result (readCellArray.f90:116-140; equiSources.f90:661-731, :785-836)
    def _map(self, host_fn, device_fn, izone, shape, centre, zoom, extra, value, value_device_ptr):
        nxmap, nymap = int(shape[0]), int(shape[1])
        out = np.empty((max(nymap, 1), max(nxmap, 1)), dtype=np.float32)  # the reference's mapArray(nxmap,nymap) as it lies in memory
        centre = _f64(centre).reshape(-1)
        args = (self._ctx, int(izone), nxmap, nymap, _dp(centre), float(zoom), extra)
        mp = out.ctypes.data_as(C.POINTER(C.c_float))
        if value_device_ptr is not None:
            self._ok(device_fn(*args, C.c_void_p(int(value_device_ptr)), mp))
        else:
            if value is not None:
                value = _f64(value).reshape(-1)
                if value.size != self.ncell:
                    raise ValueError("value must have one entry per leaf")
            self._ok(host_fn(*args, None if value is None else _dp(value), mp))
        return out.T  # [nxmap][nymap]: map[i, j] is mapArray(i+1, j+1)

    def slice_map(self, izone: int, shape, zslice: float, centre=(0.5, 0.5), zoom: float = 1.0, value=None,
                  value_device_ptr: Optional[int] = None) -> np.ndarray:
        """The reader's slice map (readCellArray.f90:116-140): float32 [nxmap][nymap], pixel = the value of the leaf at
        (x0, y0, zslice) of izone's sweep frame.  value[ncell] (or a device array); None = HI of the medium."""
        if len(centre) != 2:
            raise ValueError("centre must have two entries")
        return self._map(self._lib.ftte_slice_map, self._lib.ftte_slice_map_device, izone, shape, centre, zoom, float(zslice), value,
                         value_device_ptr)

    def project_map(self, izone: int, shape, centre=(0.5, 0.5, 0.5), zoom: float = 1.0, mode: int = 0, value=None,
                    value_device_ptr: Optional[int] = None) -> np.ndarray:
        """mode 0: the mass-weighted projection of mode initialConfiguration (equiSources.f90:678-719), float32 [nxmap][nymap];
        mode 1 (not in the reference): the path integral sum value * leaf size [cm].  None = abun2 of the medium."""
        if len(centre) != 3:
            raise ValueError("centre must have three entries")
        return self._map(self._lib.ftte_project_map, self._lib.ftte_project_map_device, izone, shape, centre, zoom, int(mode), value,
                         value_device_ptr)

    def clumping(self) -> dict:
        """mode clumpingFactor (equiSources.f90:661-676): clumping, volume (volSum) and mean_nh (volSumDensity/volSum)."""
        a, b, d = C.c_double(), C.c_double(), C.c_double()
        self._ok(self._lib.ftte_clumping(self._ctx, C.byref(a), C.byref(b), C.byref(d)))
        return dict(clumping=a.value, volume=b.value, mean_nh=d.value)

    def gas_pdf(self) -> Tuple[np.ndarray, float]:
        """(pdfGas[50], pdfGasOutside) of mode plotPDFs (equiSources.f90:814-822)."""
        pdf, outside = np.empty(50), C.c_double()
        self._ok(self._lib.ftte_gas_pdf(self._ctx, _dp(pdf), C.byref(outside)))
        return pdf, outside.value

    def star_pdf(self, src_cells) -> Tuple[np.ndarray, int, float]:
        """(pdfStar[50], pdfStarOutside, mean HI of the host leaves) of :787-813; src_cells: the stars' host leaves."""
        cells = np.ascontiguousarray(src_cells, dtype=np.int64).reshape(-1)
        pdf, outside, mean = np.zeros(50, dtype=np.int32), C.c_int32(), C.c_double()
        self._ok(self._lib.ftte_star_pdf(self._ctx, cells.size, cells.ctypes.data_as(C.POINTER(C.c_int64)),
                                         pdf.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(outside), C.byref(mean)))
        return pdf, outside.value, mean.value

    # -- absorption spectra along the projected map's pixel columns (the library's own: include/ftte.h, csrc/ftte_spectra_math.h)
    def set_velocity(self, velx=None, vely=None, velz=None, device_ptrs=None):
        """The velocity field [cm/s], per leaf in cell-array order: velx along storage-i, vely along storage-j, velz along storage-k
        (what cellarray fields hand out).  Three None drop the field (zero peculiar velocity).  device_ptrs: three device addresses
        in place of the host arrays."""
        if device_ptrs is not None:
            self._ok(self._lib.ftte_set_velocity_device(self._ctx, *[C.c_void_p(int(p)) for p in device_ptrs]))
            return
        v = [None if a is None else _f64(a).reshape(-1) for a in (velx, vely, velz)]
        for a in v:
            if a is not None and self.ncell and a.size != self.ncell:
                raise ValueError("a velocity component must have ncell elements")
        self._ok(self._lib.ftte_set_velocity(self._ctx, *[None if a is None else _dp(a) for a in v]))

    def sightline_spectra(self, izone: int, shape, nvel: int, v0: float, dv: float, line, centre=(0.5, 0.5, 0.5), zoom: float = 1.0,
                          hubble: float = 0.0, period: float = 0.0, value=None, value_device_ptr: int = 0, want_tau: bool = True,
                          want_summary: bool = True, tau_device_ptr: int = 0, summary_device_ptr: int = 0) -> dict:
        """tau(v) of one line along every pixel column of project_map's map: dict(tau [nxmap][nymap][nvel] (None unless want_tau), N,
        W, dv90 [nxmap][nymap] (None unless want_summary), velocity [nvel] the pixels' centres).  line = (sigma_line, damping, mass, b_turb), e.g. LYMAN_ALPHA;
        value[ncell] the absorber's density (or value_device_ptr), None = HI of the medium.  With tau_device_ptr or
        summary_device_ptr the _device variant writes there ([nymap][nxmap][nvel] and [nymap][nxmap][3] doubles as they lie in
        memory) and the dict holds None for what went to the device."""
        if len(centre) != 3:
            raise ValueError("centre must have three entries")
        nxmap, nymap, nvel = int(shape[0]), int(shape[1]), int(nvel)
        centre, line = _f64(centre).reshape(-1), _f64(line).reshape(-1)
        if line.size != 4:
            raise ValueError("line must have four entries: sigma_line, damping, mass, b_turb")
        head = (self._ctx, int(izone), nxmap, nymap, _dp(centre), float(zoom), nvel, float(v0), float(dv), float(hubble), float(period), _dp(line))
        tau = summary = None
        if value_device_ptr or tau_device_ptr or summary_device_ptr:
            if value is not None:
                raise ValueError("the device variant takes value_device_ptr, not a host value array")
            if not tau_device_ptr and not summary_device_ptr:
                raise ValueError("the device variant writes to tau_device_ptr or summary_device_ptr")
            self._ok(self._lib.ftte_sightline_spectra_device(*head, C.c_void_p(int(value_device_ptr) or None), C.c_void_p(int(tau_device_ptr) or None),
                                                             C.c_void_p(int(summary_device_ptr) or None)))
        else:
            if value is not None:
                value = _f64(value).reshape(-1)
                if value.size != self.ncell:
                    raise ValueError("value must have one entry per leaf")
            shape3 = (max(nymap, 1), max(nxmap, 1))
            tau = np.empty(shape3 + (max(nvel, 1),)) if want_tau else None
            summary = np.empty(shape3 + (3,)) if want_summary else None
            self._ok(self._lib.ftte_sightline_spectra(*head, None if value is None else _dp(value), None if tau is None else _dp(tau),
                                                      None if summary is None else _dp(summary)))
        out = dict(tau=None if tau is None else tau.transpose(1, 0, 2), N=None, W=None, dv90=None,
                   velocity=float(v0) + (np.arange(max(nvel, 0)) + 0.5) * float(dv))
        if summary is not None:
            out.update(N=summary[:, :, 0].T, W=summary[:, :, 1].T, dv90=summary[:, :, 2].T)
        return out

    # -- the same along rays of any origin and direction (include/ftte.h, csrc/ftte_ray_math.h)
    @staticmethod
    def _rays(origins, directions, tmax, periodic=False):
        o, d = _f64(origins).reshape(-1, 3), _f64(directions).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("origins and directions must both be [nray][3]")
        if periodic and tmax is None:
            raise ValueError("a periodic ray needs its tmax")
        if tmax is not None:
            tmax = _f64(tmax).reshape(-1)
            if tmax.size != o.shape[0]:
                raise ValueError("tmax must have one entry per ray")
        return o, d, tmax

    def ray_spectra(self, origins, directions, nvel: int, v0: float, dv: float, line, tmax=None, hubble: float = 0.0, period: float = 0.0,
                    value=None, want_tau: bool = True, want_summary: bool = True, tau_device_ptr=None, summary_device_ptr=None,
                    value_device_ptr=None, periodic: bool = False) -> dict:
        """tau(v) of one line along rays through the refined grid: dict(tau [nray][nvel] (None unless want_tau), N, W, dv90 [nray]
        (None unless want_summary), velocity [nvel]).  origins, directions [nray][3] in the storage frame, base cells (the box is
        [0, n]^3), directions unit vectors; tmax [nray] the rays' ends from their origins (None or <= 0: the box's far side).  A ray
        that misses the box has N = 0 and tau = 0.  line, value, hubble, period as sightline_spectra.  With tau_device_ptr or
        summary_device_ptr the _device variant writes there ([nray][nvel] and [nray][3] doubles) and the dict holds None for what
        went to the device.  periodic: the box tiles space and every ray goes on through the opposite face from its origin (anywhere)
        to its tmax, which is then required and > 0; s, and with it the Hubble velocity, keeps growing across images."""
        o, d, tmax = self._rays(origins, directions, tmax, periodic)
        host, device = (self._lib.ftte_ray_spectra_periodic, self._lib.ftte_ray_spectra_periodic_device) if periodic else \
            (self._lib.ftte_ray_spectra, self._lib.ftte_ray_spectra_device)
        nray, nvel = o.shape[0], int(nvel)
        line = _f64(line).reshape(-1)
        if line.size != 4:
            raise ValueError("line must have four entries: sigma_line, damping, mass, b_turb")
        head = (self._ctx, nray, _dp(o), _dp(d), None if tmax is None else _dp(tmax), nvel, float(v0), float(dv), float(hubble), float(period), _dp(line))
        tau = summary = None
        if value_device_ptr or tau_device_ptr or summary_device_ptr:
            if value is not None:
                raise ValueError("the device variant takes value_device_ptr, not a host value array")
            if not tau_device_ptr and not summary_device_ptr:
                raise ValueError("the device variant writes to tau_device_ptr or summary_device_ptr")
            self._ok(device(*head, C.c_void_p(int(value_device_ptr or 0) or None), C.c_void_p(int(tau_device_ptr or 0) or None),
                            C.c_void_p(int(summary_device_ptr or 0) or None)))
        else:
            if value is not None:
                value = _f64(value).reshape(-1)
                if value.size != self.ncell:
                    raise ValueError("value must have one entry per leaf")
            tau = np.empty((max(nray, 1), max(nvel, 1))) if want_tau else None
            summary = np.empty((max(nray, 1), 3)) if want_summary else None
            self._ok(host(*head, None if value is None else _dp(value), None if tau is None else _dp(tau), None if summary is None else _dp(summary)))
        out = dict(tau=tau, N=None, W=None, dv90=None, velocity=float(v0) + (np.arange(max(nvel, 0)) + 0.5) * float(dv))
        if summary is not None:
            out.update(N=summary[:, 0].copy(), W=summary[:, 1].copy(), dv90=summary[:, 2].copy())
        return out

    def ray_segments(self, origins, directions, tmax=None, periodic: bool = False) -> dict:
        """The leaves the rays cross, in their order: dict(offset [nray + 1], leaf, t_in, t_out per segment); ray r's segments are
        offset[r] .. offset[r + 1] - 1, t in base cells from the ray's origin.  periodic: as ray_spectra; the segments tile [0, tmax]."""
        o, d, tmax = self._rays(origins, directions, tmax, periodic)
        segments = self._lib.ftte_ray_segments_periodic if periodic else self._lib.ftte_ray_segments
        nray = o.shape[0]
        lp = C.POINTER(C.c_int64)
        offset = np.zeros(max(nray, 1) + 1, dtype=np.int64)
        head = (self._ctx, nray, _dp(o), _dp(d), None if tmax is None else _dp(tmax), offset.ctypes.data_as(lp))
        self._ok(segments(*head, 0, None, None, None))
        total = int(offset[-1])
        leaf, t_in, t_out = np.zeros(total, dtype=np.int64), np.zeros(total), np.zeros(total)
        if total:
            self._ok(segments(*head, total, leaf.ctypes.data_as(lp), _dp(t_in), _dp(t_out)))
        return dict(offset=offset, leaf=leaf, t_in=t_in, t_out=t_out)


expansion_parameters = StellarTransfer.expansion_parameters
