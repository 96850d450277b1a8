"""What the tests of the oblique rays share (test_rays_host.py, test_rays_gpu.py):

  walk          the g++ evaluation of csrc/ftte_ray_math.h (tests/host/ray_check.cpp through _hostlib.HostLib) over a node array
                built from tests/_analysis.Tree: per ray its segments (leaf, t_in, t_out) -- what the GPU is compared with bit for bit;
  brute         the independent statement in numpy: the slab intersection of a ray with every leaf's box, sorted by t_in;
  compare       the two against each other under the stated condition;
  line_inputs   what a segment gives the line (size, s, u), by the header; spectra() then is tests/_spectra.lines over them;
  axis_rays     the rays that coincide with the pixel columns of a map under an izone;
  batch_rays    the host's batch rule restated (held to csrc/ftte_rays.h by tests/host/ray_batch_check.cpp);
  cases         the named rays of the issue and the fixed-seed random ones.
"""
import ctypes as C

import numpy as np

import _analysis as A
import _spectra as S
from _hostlib import CSRC, ROOT, SANITIZE, HostLib, dp as _dp, f64 as _f64  # noqa: F401

TINY = 1.0e-9        # [cells] a leaf whose chord is below this may be missing from either list
WORK_BYTES, CHUNK = S.WORK_BYTES, S.CHUNK
RECORD_BYTES, LIST_BYTES = 32, 24


def _lp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_longlong))


def _declare(L):
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_int32)
    L.ry_arguments_ok.argtypes, L.ry_arguments_ok.restype = [dp, dp, dp], C.c_int
    L.ry_step_bound.argtypes, L.ry_step_bound.restype = [C.c_int, C.c_int], C.c_longlong
    L.ry_first_exit.argtypes, L.ry_first_exit.restype = [C.c_int, ip, dp, dp, dp], C.c_int
    L.ry_walk.argtypes, L.ry_walk.restype = [C.c_int, C.c_int, ip, C.c_longlong, dp, dp, dp, lp, dp, C.c_longlong, lp, dp, dp], C.c_longlong
    L.ry_line_inputs.argtypes, L.ry_line_inputs.restype = [C.c_longlong, dp, dp, C.c_int, lp, lp, dp, dp, C.c_double, dp, dp, dp, dp, dp, dp], None


lib = HostLib("rays", "ray_check.cpp", ("ftte_ray_math.h", "ftte_math.h"), "the ray walk", _declare)
SOURCE = lib.source


def node_array(tree):
    """{child0, leaf, parent, level} int32 records of an _analysis.Tree (the walk reads the first two), or None for a uniform grid"""
    if tree.max_level == 0:
        return None
    out = np.full((tree.child0.size, 4), -1, dtype=np.int32)
    out[:, 0], out[:, 1], out[:, 3] = tree.child0, tree.leaf, 0
    return np.ascontiguousarray(out)


def rays(origins, directions, tmax=None):
    o, d = _f64(origins).reshape(-1, 3).copy(), _f64(directions).reshape(-1, 3).copy()
    assert o.shape == d.shape
    return o, d, None if tmax is None else _f64(tmax).reshape(-1).copy()


def arguments_ok(o, d, tmax=None):
    o, d = _f64(o), _f64(d)
    t = None if tmax is None else _f64([tmax])
    return bool(lib().ry_arguments_ok(_dp(o), _dp(d), _dp(t)))


def first_exit(tree, o, d):
    """(exit axis, t_out) of the first leaf a ray is in; axis -1: it misses"""
    o, d, nodes, t = _f64(o), _f64(d), node_array(tree), np.zeros(1)
    axis = lib().ry_first_exit(tree.n, None if nodes is None else nodes.ctypes.data_as(C.POINTER(C.c_int32)), _dp(o), _dp(d), _dp(t))
    return int(axis), float(t[0])


class Walk:
    """off[nray + 1], leaf, t_in, t_out per segment, start[nray][2] = t_start, t_end: the header's walk"""

    def __init__(self, tree, origins, directions, tmax=None):
        o, d, t = rays(origins, directions, tmax)
        nodes = node_array(tree)
        ip = C.POINTER(C.c_int32)
        nray = o.shape[0]
        self.off, self.start = np.zeros(nray + 1, dtype=np.int64), np.zeros((nray, 2))
        args = (tree.n, tree.max_level, None if nodes is None else nodes.ctypes.data_as(ip), nray, _dp(o), _dp(d), _dp(t), _lp(self.off), _dp(self.start))
        total = lib().ry_walk(*args, 0, None, None, None)
        assert total >= 0, f"ray {-1 - total} passed the step bound"
        self.leaf, self.t_in, self.t_out = np.zeros(total, dtype=np.int64), np.zeros(total), np.zeros(total)
        if total:
            assert lib().ry_walk(*args, total, _lp(self.leaf), _dp(self.t_in), _dp(self.t_out)) == total
        self.o, self.d, self.tmax, self.n, self.nray = o, d, t, tree.n, nray

    def of(self, r):
        a, b = self.off[r], self.off[r + 1]
        return self.leaf[a:b], self.t_in[a:b], self.t_out[a:b]

    def line_inputs(self, box, vel=None):
        """(size [cm], s [cm], u) per segment"""
        size, s, u = (np.zeros(self.leaf.size) for _ in range(3))
        v = [None] * 3 if vel is None else [_f64(a) for a in vel]
        lib().ry_line_inputs(self.nray, _dp(self.o), _dp(self.d), self.n, _lp(self.off), _lp(self.leaf), _dp(self.t_in), _dp(self.t_out), box / float(self.n),
                             _dp(v[0]), _dp(v[1]), _dp(v[2]), _dp(size), _dp(s), _dp(u))
        return size, s, u

    def spectra(self, box, value, tgas, vel, nvel, v0, dv, line, hubble=0.0, period=0.0):
        """dict(tau [nray][nvel], N, W, dv90 [nray]): the line's header over the walk's segments"""
        size, s, u = self.line_inputs(box, vel)
        status, tau, summary = S.lines(self.off, _f64(value)[self.leaf], size, _f64(tgas)[self.leaf], s, u, nvel, v0, dv, line, hubble, period)
        assert status == 0, status
        return dict(tau=tau, N=summary[:, 0], W=summary[:, 1], dv90=summary[:, 2])


# ---- the independent statement

def leaf_boxes(tree):
    """(lo [ncell][3], h [ncell]) in base cells, storage frame"""
    n = tree.n
    lo, h = np.zeros((tree.ncell, 3)), np.zeros(tree.ncell)
    stack = [(b, (float(b // (n * n)), float((b // n) % n), float(b % n)), 1.0) for b in range(n ** 3)]
    while stack:
        node, at, size = stack.pop()
        if tree.child0[node] < 0:
            lo[tree.leaf[node]], h[tree.leaf[node]] = at, size
        else:
            for q in range(8):
                half = size / 2.0
                stack.append((tree.child0[node] + q, (at[0] + half * (q >> 2), at[1] + half * ((q >> 1) & 1), at[2] + half * (q & 1)), half))
    return lo, h


def _slabs(lo, hi, o, d, tmax):
    """[t_lo, t_hi] of one ray in boxes [lo, hi] (arrays [m][3]); an axis with d == 0 holds the ray where lo <= o < hi"""
    t_lo, t_hi = np.zeros(lo.shape[0]), np.full(lo.shape[0], np.inf if tmax is None or not tmax > 0 else tmax)
    inside = np.ones(lo.shape[0], dtype=bool)
    for a in range(3):
        if d[a] == 0.0:
            inside &= (lo[:, a] <= o[a]) & (o[a] < hi[:, a])
        else:
            t1, t2 = (lo[:, a] - o[a]) / d[a], (hi[:, a] - o[a]) / d[a]
            t_lo, t_hi = np.maximum(t_lo, np.minimum(t1, t2)), np.minimum(t_hi, np.maximum(t1, t2))
    return t_lo, t_hi, inside


def brute(boxes, n, o, d, tmax=None):
    """(leaf, t_in, t_out) of one ray over all leaves, sorted by t_in, chords > 0; and (t_start, t_end) of the box"""
    lo, h = boxes
    t_lo, t_hi, inside = _slabs(lo, lo + h[:, None], o, d, tmax)
    keep = np.nonzero(inside & (t_hi - t_lo > 0.0))[0]
    keep = keep[np.argsort(t_lo[keep], kind="stable")]
    b_lo, b_hi, b_in = _slabs(np.zeros((1, 3)), np.full((1, 3), float(n)), o, d, tmax)
    span = (float(b_lo[0]), float(b_hi[0])) if b_in[0] and b_hi[0] > b_lo[0] else (0.0, 0.0)
    return keep, t_lo[keep], t_hi[keep], span


def compare(walk, boxes, r):
    """Ray r of the walk against the brute-force list under the stated condition: leaves of chord < TINY may be missing from either
    list, all others match in identity and order, t and chords within 1e-12 n, the chords add up to t_end - t_start.  Returns
    (segments, tiny leaves dropped from either list, largest difference in t or a chord [cells])."""
    n = walk.n
    tol = 1e-12 * n
    leaf, a, b = walk.of(r)
    want_leaf, wa, wb, span = brute(boxes, n, walk.o[r], walk.d[r], None if walk.tmax is None else walk.tmax[r])
    big, want_big = (b - a) >= TINY, (wb - wa) >= TINY
    assert np.array_equal(leaf[big], want_leaf[want_big]), (r, leaf, want_leaf)
    worst = 0.0
    if big.any():
        worst = max(np.abs(a[big] - wa[want_big]).max(), np.abs(b[big] - wb[want_big]).max(), np.abs((b - a)[big] - (wb - wa)[want_big]).max())
    assert worst <= tol, (r, worst)
    assert abs((b - a).sum() - (span[1] - span[0])) <= tol, (r, (b - a).sum(), span)
    assert abs((walk.start[r, 1] - walk.start[r, 0]) - (span[1] - span[0])) <= tol, (r, walk.start[r], span)
    assert np.all(b > a) and np.all(a[1:] == b[:-1]), r  # no gap, by construction
    if leaf.size:
        assert a[0] == walk.start[r, 0] and b[-1] == walk.start[r, 1], r
    return leaf.size, int((~big).sum() + (~want_big).sum()), worst


# ---- rays along the pixel columns of a map

def axis_rays(tree, izone, shape, centre=(0.5, 0.5, 0.5), zoom=1.0):
    """(origins, directions, tmax) [nxmap * nymap] in the order of _spectra.Segments' pixels q = i nymap + j: transverse i0 - 1 + frac,
    mirrored axes n - v, direction +-e of the depth's storage axis, from the entry face of base cell kstart over kend - kstart + 1
    cells.  A mirrored transverse coordinate that lies exactly on a leaf face goes one ulp down: the map's half-open cell
    [v, v + h) is (n - v - h, n - v] in storage, and the ray's rule for a face with d = 0 is the half-open cell above it."""
    n = tree.n
    i0, xn = A.map_axis(n, shape[0], centre[0], zoom)
    j0, yn = A.map_axis(n, shape[1], centre[1], zoom)
    kstart, kend = A.map_depth(n, centre[2], zoom)
    X, Y = (a.ravel() for a in np.meshgrid((i0 - 1) + xn, (j0 - 1) + yn, indexing="ij"))
    sweep = [X, Y, np.full(X.size, float(kstart - 1))]
    src, mirror = A.zone(izone)
    o, d = np.zeros((X.size, 3)), np.zeros((X.size, 3))
    for a in range(3):
        v = sweep[src[a]]
        if mirror[a]:
            v = n - v
            if src[a] != 2:
                fine = np.ldexp(v, tree.max_level)
                v = np.where(fine == np.floor(fine), np.nextafter(v, -np.inf), v)
        o[:, a] = v
        if src[a] == 2:
            d[:, a] = -1.0 if mirror[a] else 1.0
    return o, d, np.full(X.size, float(kend - kstart + 1))


# ---- the batch rule, restated (held to csrc/ftte_rays.h by tests/host/ray_batch_check.cpp)

def batch_rays(offset, ray0, nvel, stage_tau, per_segment):
    """rays per launch from ray0 on: ftte::ray_batch_rays"""
    nray = len(offset) - 1
    if nray < 1 or ray0 < 0 or ray0 >= nray:
        return 1
    per_ray = 24 + (8 * max(nvel, 0) if stage_tau else 0)
    m = 0
    while ray0 + m < nray and (int(offset[ray0 + m + 1]) - int(offset[ray0])) * per_segment + (m + 1) * per_ray <= WORK_BYTES:
        m += 1
    return max(m, 1)


def batches(offset, nvel, stage_tau, per_segment=RECORD_BYTES):
    """[(ray0, rays)] of the launches of one call"""
    out, at, nray = [], 0, len(offset) - 1
    while at < nray:
        m = batch_rays(offset, at, nvel, stage_tau, per_segment)
        out.append((at, m))
        at += m
    return out


# ---- the cases

def unit(v):
    v = _f64(v)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def named_rays(n):
    """the issue's named rays on an n^3 base grid (n >= 4): (what, origin, direction, tmax)"""
    r3, r2 = 1.0 / np.sqrt(3.0), 1.0 / np.sqrt(2.0)
    out = [("the body diagonal", (0, 0, 0), (r3, r3, r3), 0.0),
           ("the other way along it", (n, n, n), (-r3, -r3, -r3), 0.0),
           ("in a face plane", (0.1, 2.0, 0.3), (r2, 0.0, r2), 0.0),
           ("in a face plane of the refined corner", (0.05, 0.25, 0.02), (r2, 0.0, r2), 0.0),
           ("along an edge", (1.0, 2.0, -1.0), (0.0, 0.0, 1.0), 0.0),
           ("along an edge of the refined corner", (0.5, 0.25, n + 1.0), (0.0, 0.0, -1.0), 0.0),
           ("a miss", (-1.0, n + 1.0, 0.5), (1.0, 0.0, 0.0), 0.0),
           ("pointing away", (n + 5.0, n + 5.0, n + 5.0), (r3, r3, r3), 0.0),
           ("a miss on an axis without direction", (0.5, float(n), 0.5), (1.0, 0.0, 0.0), 0.0),
           ("a tmax inside a leaf", (0.3, 0.2, 0.1), (r3, r3, r3), 1.7),
           ("a tmax before the box", (-3.0, 0.5, 0.5), (1.0, 0.0, 0.0), 2.0),
           ("an origin inside a deepest leaf", (0.01, 0.02, 0.03), (-r3, r3, -r3), 0.0),
           ("negative zeros", (0.5, 0.5, float(n)), (-0.0, -0.0, -1.0), 0.0),
           ("on the far face, outwards", (float(n), 0.5, 0.5), (1.0, 0.0, 0.0), 0.0)]
    for a in range(3):
        for sign in (1.0, -1.0):
            o = [0.125, 0.625, n - 0.5]
            o[a] = n / 2.0 - sign * (n / 2.0 + 1.0)
            d = [0.0, 0.0, 0.0]
            d[a] = sign
            out.append((f"{'+' if sign > 0 else '-'}e_{a}", tuple(o), tuple(d), 0.0))
    return out


def random_rays(n, count, seed):
    """origins inside and outside the box, directions over the sphere, every fifth ray with a tmax"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.5 * n, 1.5 * n, (count, 3))
    inside = rng.random(count) < 0.5
    o[inside] = rng.uniform(0.0, n, (int(inside.sum()), 3))
    d = unit(rng.normal(size=(count, 3)))
    tmax = np.where(np.arange(count) % 5 == 0, rng.uniform(0.0, 1.5 * n, count), 0.0)
    return o, d, tmax
