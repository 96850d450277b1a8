"""What the tests of the sightline spectra share (test_spectra_host.py, test_spectra_gpu.py):

  segments      the sightlines of a map as segment lists, from the numpy walk of tests/_analysis.py (its Tree, its axes, its child
                choice): per pixel column the leaves in the order project_map meets them, with their sizes, the distance of their
                centres from the entry face and the velocity component along the line of sight;
  lines         the g++ evaluation of csrc/ftte_spectra_math.h over such lists (tests/host/spectra_check.cpp through _hostlib.HostLib):
                tau, N, W, dv90 -- what the GPU is compared with bit for bit;
  profile       H(a, x) of the header;
  numpy_tau     the same formula in plain numpy (np.exp), the same order, for a = 0.
"""
import ctypes as C

import numpy as np

import _analysis as A
from _hostlib import CSRC, ROOT, SANITIZE, HostLib, dp as _dp, f64 as _f64  # noqa: F401

KB = 1.380649e-16
INV_SQRTPI = float.fromhex("0x1.20dd750429b6dp-1")
LYMAN_ALPHA = (1.3435e-7, 606.08, 1.6735e-24, 0.0)


def _declare(L):
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    L.sp_profile.argtypes, L.sp_profile.restype = [C.c_longlong, dp, C.c_double, dp], None
    L.sp_wing.argtypes, L.sp_wing.restype = [C.c_longlong, dp, C.c_double, dp, dp], None
    L.sp_lines.argtypes, L.sp_lines.restype = [C.c_longlong, lp, dp, dp, dp, dp, dp, dp, C.c_longlong, dp, dp], C.c_longlong
    L.sp_summarise.argtypes, L.sp_summarise.restype = [C.c_longlong, dp, C.c_double, dp], None


lib = HostLib("spectra", "spectra_check.cpp", ("ftte_spectra_math.h", "ftte_math.h"), "the sightline spectra", _declare)
SOURCE = lib.source


def profile(x, a):
    x = _f64(x).reshape(-1)
    H = np.empty_like(x)
    lib().sp_profile(x.size, _dp(x), float(a), _dp(H))
    return H


def wing(x2, a):
    """(spectra_wing, spectra_voigt with H0 = 0) of the header over x^2"""
    x2 = _f64(x2).reshape(-1)
    w, whole = np.empty_like(x2), np.empty_like(x2)
    lib().sp_wing(x2.size, _dp(x2), float(a), _dp(w), _dp(whole))
    return w, whole


def depth_axis(izone):
    """(storage axis the sweep frame's depth feeds, whether it is mirrored)"""
    src, mirror = A.zone(izone)
    a = src.index(2)
    return a, mirror[a]


class Segments:
    """off[npix + 1], and per segment leaf, size [cm], s [cm]; pixel q = i * nymap + j (the maps' [nxmap][nymap] raveled)"""

    def __init__(self, tree, box, izone, shape, centre=(0.5, 0.5, 0.5), zoom=1.0):
        n = tree.n
        i0, xn = A.map_axis(n, shape[0], centre[0], zoom)
        j0, yn = A.map_axis(n, shape[1], centre[1], zoom)
        kstart, kend = A.map_depth(n, centre[2], zoom)
        I0, J0 = (a.ravel() for a in np.meshgrid(i0, j0, indexing="ij"))
        X, Y = (a.ravel() for a in np.meshgrid(xn, yn, indexing="ij"))
        npix = X.size
        cmap = A.child_map(izone)
        cell = box / float(n)
        found = []  # (pixels, leaves, size, centre as a fraction of the base cell + base cells behind kstart) in visiting order

        def visit(node, x, y, size, lo, half, idx, behind):
            ref = tree.child0[node] >= 0
            if (~ref).any():
                found.append((idx[~ref], tree.leaf[node[~ref]], size, behind + (lo + half)))
            if ref.any():
                a, xr = A._half(x[ref])
                b, yr = A._half(y[ref])
                for c in (0, 1):
                    visit(tree.child0[node[ref]] + cmap[4 * a + 2 * b + c], xr, yr, size / 2.0, lo + half if c else lo, half * 0.5, idx[ref], behind)

        everyone = np.arange(npix)
        for k0 in range(kstart, kend + 1):
            visit(A._base_nodes(izone, n, I0, J0, np.full(npix, k0, dtype=np.int64)), X, Y, cell, 0.0, 0.5, everyone, float(k0 - kstart))
        pix = np.concatenate([f[0] for f in found])
        order = np.argsort(pix, kind="stable")  # each pixel keeps its own visiting order
        self.leaf = np.concatenate([f[1] for f in found])[order]
        self.size = np.concatenate([np.full(f[0].size, f[2]) for f in found])[order]
        self.s = np.concatenate([np.full(f[0].size, f[3]) for f in found])[order] * cell
        self.off = np.concatenate([[0], np.cumsum(np.bincount(pix, minlength=npix))]).astype(np.int64)
        self.shape, self.npix, self.izone = tuple(shape), npix, izone

    def velocity(self, vel):
        """u per segment from vel = (velx, vely, velz) per leaf, or zeros for None"""
        if vel is None:
            return np.zeros(self.leaf.size)
        a, mirrored = depth_axis(self.izone)
        u = _f64(vel[a])[self.leaf]
        return -u if mirrored else u


def lines(off, dens, size, tgas, s, u, nvel, v0, dv, line, hubble=0.0, period=0.0, want_tau=True):
    """(status, tau [nline][nvel] or None, summary [nline][3]) of the header over segment lists"""
    off = np.ascontiguousarray(off, dtype=np.int64)
    nline = off.size - 1
    arrays = [_f64(a).reshape(-1) for a in (dens, size, tgas, s, u)]
    assert all(a.size == off[-1] for a in arrays)
    par = _f64([v0, dv, hubble, period, *line, 0.0])
    tau = np.full((nline, nvel), -7.0) if want_tau else None
    summary = np.full((nline, 3), -7.0)
    status = lib().sp_lines(nline, off.ctypes.data_as(C.POINTER(C.c_longlong)), *[_dp(a) for a in arrays], _dp(par), int(nvel),
                            None if tau is None else _dp(tau), _dp(summary))
    return int(status), tau, summary


def map_lines(seg, value, tgas, vel, nvel, v0, dv, line, hubble=0.0, period=0.0):
    """the header over the sightlines of a Segments: dict(tau [nxmap][nymap][nvel], N, W, dv90 [nxmap][nymap])"""
    status, tau, summary = lines(seg.off, _f64(value)[seg.leaf], seg.size, _f64(tgas)[seg.leaf], seg.s, seg.velocity(vel), nvel, v0, dv, line, hubble, period)
    assert status == 0, status
    sh = seg.shape
    return dict(tau=tau.reshape(sh + (nvel,)), N=summary[:, 0].reshape(sh), W=summary[:, 1].reshape(sh), dv90=summary[:, 2].reshape(sh))


def summarise(tau, dv):
    tau = _f64(tau).reshape(-1)
    out = np.empty(2)
    lib().sp_summarise(tau.size, _dp(tau), float(dv), _dp(out))
    return float(out[0]), float(out[1])


def numpy_tau(dens, size, tgas, s, u, nvel, v0, dv, line, hubble=0.0, period=0.0):
    """one sightline with a = 0 in plain numpy: the header's formula in its order with np.exp"""
    sigma, damping, mass, bturb = line
    assert damping == 0.0
    vp = v0 + (np.arange(nvel) + 0.5) * dv
    tau = np.zeros(nvel)
    for q in range(len(dens)):
        b = np.sqrt((2.0 * KB * tgas[q]) / mass + bturb * bturb)
        inv_b = 1.0 / b
        amp = ((dens[q] * size[q]) * sigma) * INV_SQRTPI * inv_b
        d = vp - (hubble * s[q] + u[q])
        if period > 0.0:
            d = d - period * np.rint(d * (1.0 / period))
        x = d * inv_b
        x2 = x * x
        tau = tau + np.where(x2 <= 64.0, amp * np.exp(-np.minimum(x2, 64.0)), 0.0)
    return tau


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
