"""What the tests of the sightline spectra share (test_spectra_host.py, test_spectra_gpu.py):

  segments      the sightlines of a map as segment lists, from the numpy walk of tests/_analysis.py (its Tree, its axes, its child
                choice): per pixel column the leaves in the order project_map meets them, with their sizes, the distance of their
                centres from the entry face and the velocity component along the line of sight;
  lines         the g++ evaluation of csrc/ftte_spectra_math.h over such lists (tests/host/spectra_check.cpp through _hostlib.HostLib):
                tau, N, W, dv90 -- what the GPU is compared with bit for bit;
  profile       H(a, x) of the header;
  numpy_tau     the same formula in plain numpy (np.exp), the same order, for a = 0;
  uniform_segments  the segments of a uniform grid too large for the walk's Tree;
  batch_lines   the host's batch rule restated, for the GPU tests to place their seams by (held to the library's by
                tests/host/spectra_batch_check.cpp);
  deep_levels   level lists whose chosen sightlines cross a wanted number of leaves.
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


class _Lists:
    """what map_lines reads of a Segments, from arrays"""
    velocity = Segments.velocity

    def __init__(self, off, leaf, size, s, shape, izone):
        self.off, self.leaf, self.size, self.s = off, leaf, size, s
        self.shape, self.npix, self.izone = tuple(shape), off.size - 1, izone


def uniform_segments(n, box, izone, shape, centre=(0.5, 0.5, 0.5), zoom=1.0):
    """Segments of a uniform grid without its Tree (a Python loop over base cells): a base cell is its own leaf, its size the
    cell's, its centre half a cell behind its entry face.  Held to Segments(Tree(n, zeros)) by test_spectra_host.py."""
    i0, _ = A.map_axis(n, shape[0], centre[0], zoom)
    j0, _ = A.map_axis(n, shape[1], centre[1], zoom)
    kstart, kend = A.map_depth(n, centre[2], zoom)
    depth = kend - kstart + 1
    I0, J0 = (a.ravel() for a in np.meshgrid(i0, j0, indexing="ij"))
    k0 = np.arange(kstart, kend + 1, dtype=np.int64)
    leaf = A._base_nodes(izone, n, I0[:, None], J0[:, None], k0[None, :]).ravel()
    cell = box / float(n)
    s = np.tile((k0 - kstart).astype(np.float64) + 0.5, I0.size) * cell
    return _Lists(np.arange(I0.size + 1, dtype=np.int64) * depth, leaf, np.full(leaf.size, cell), s, shape, izone)


# ---- the batch rule and the kernel's sizes, restated (held to csrc/ftte_spectra.h by tests/host/spectra_batch_check.cpp)

WORK_BYTES, CHUNK, LANES, PASS_PIXELS = 1 << 26, 512, 256, 1024


def batch_lines(nlines, nvel, stage_tau, most):
    """sightlines per launch: ftte::spectra_batch_lines"""
    per_line = 24 + (8 * max(nvel, 0) if stage_tau else 0) + (32 * most if most > CHUNK else 0)
    return 1 if nlines < 1 else max(1, min(WORK_BYTES // per_line, nlines))


def batches(nlines, nvel, stage_tau, most):
    """[(line0, lines)] of the launches of one call"""
    step = batch_lines(nlines, nvel, stage_tau, most)
    return [(at, min(step, nlines - at)) for at in range(0, nlines, step)]


def line_counts(seg):
    """segments per sightline in the order the kernel numbers them: line = i + nxmap j"""
    return np.diff(seg.off).reshape(seg.shape).T.ravel()


# ---- trees with sightlines of a wanted length

def deep_column(crossings, level, first):
    """the depth-first level list of a cell the sightline crosses `crossings` times: the two depth children on the line (the upper
    children along the map axes below a base cell, the lower ones further down: a pixel at the centre of its base cell) share them"""
    if crossings == 1:
        return [level]
    a = b = 1 if first else 0
    out = []
    for child in range(8):
        ca, cb, cc = child >> 2, (child >> 1) & 1, child & 1
        if (ca, cb) == (a, b):
            out += deep_column(crossings // 2 if cc == 0 else crossings - crossings // 2, level + 1, False)
        else:
            out.append(level + 1)
    return out


def deep_levels(n, columns):
    """the level list of an n^3 base grid whose storage columns (icell, jcell) of `columns` = {(i, j): crossings} are refined until a
    sightline along storage k through the centre of the column crosses that many leaves, dealt over the column's n base cells;
    every other base cell is a leaf.  For the izones whose depth is storage k and whose map axes are not mirrored (1 and 5)."""
    parts = []
    plain = np.zeros(n, dtype=np.int32)
    for i in range(n):
        for j in range(n):
            want = columns.get((i, j))
            if want is None:
                parts.append(plain)
            else:
                assert want >= n
                for k in range(n):
                    parts.append(np.array(deep_column(want // n + (1 if k < want % n else 0), 0, True), dtype=np.int32))
    return np.concatenate(parts)


def seam_lines(fit, most):
    """{line: segments} that puts spilled sightlines of differing lengths on both sides of the seams of batches of `fit` lines in a
    map of 4096, at its first and last line, and three lengths above a chunk into the first batch"""
    return {0: most, 330: CHUNK, 700: 700, fit - 1: CHUNK + 1, fit: most, 2 * fit - 1: 700, 2 * fit: 2 * CHUNK, 4095: most}


def seam_columns(n, nvel, most):
    """deep_levels' columns of an n x n map over an n^3 grid for the seams of both paths -- tau staged (host arrays, tau absent) and
    not (tau to the caller's device array: the spill alone decides) -- under izone 1 (map pixel (i, j) is storage column (i, j)) and
    under izone 5 (it is column (j, i))"""
    columns = {}
    for stage_tau in (False, True):
        fit = batch_lines(n * n, nvel, stage_tau, most)
        for line, count in seam_lines(fit, most).items():
            i, j = line % n, line // n
            for at in ((i, j), (j, i)):
                assert columns.setdefault(at, count) == count, "two lengths asked of one column"
    return columns


def seam_conditions(counts, nvel, stage_tau):
    """what makes a call a test of the batch loop, asserted of the reference's segment counts per line (line_counts): at least three
    batches, the last one short, a spilled line in the first, a middle and the last, spilled lines on both sides of every seam,
    three lengths above a chunk in one launch.  Returns the batches."""
    bs = batches(counts.size, nvel, stage_tau, int(counts.max()))
    assert len(bs) >= 3 and bs[-1][1] < bs[0][1] and all(b[1] == bs[0][1] for b in bs[:-1]), bs
    deep = counts > CHUNK
    for at, nl in (bs[0], bs[len(bs) // 2], bs[-1]):
        assert deep[at:at + nl].any(), (at, nl)
    for at, _ in bs[1:]:
        assert deep[at - 1] and deep[at] and counts[at - 1] != counts[at], at
    assert max(len(set(counts[at:at + nl][deep[at:at + nl]].tolist())) for at, nl in bs) >= 3
    assert (counts == CHUNK).any() and (counts == CHUNK + 1).any()
    return bs


def random_medium(ncell, seed, box=3.0e24):
    """HI, tgas and three velocity components per leaf"""
    rng = np.random.default_rng(seed)
    return dict(box=box, HI=10.0 ** rng.uniform(-9, -5, ncell), tgas=10.0 ** rng.uniform(3.5, 5.0, ncell),
                vel=[rng.uniform(-2e7, 2e7, ncell) for _ in range(3)])


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
