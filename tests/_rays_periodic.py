"""What the tests of the periodic rays share (test_rays_periodic_host.py, test_rays_periodic_gpu.py), beside tests/_rays.py:

  Walk          the g++ evaluation of the periodic walk of csrc/ftte_ray_math.h (tests/host/ray_periodic_check.cpp through
                _hostlib.HostLib): per ray its segments (leaf, t_in, t_out) -- what the GPU is compared with bit for bit; line_inputs
                and spectra are _rays.Walk's (size and s from t, which runs from the caller's origin across images);
  brute         the independent statement in numpy: the slab intersection of a ray with every leaf's box in every image of the box
                the ray can reach, sorted by t_in;
  compare       the two against each other under the stated condition;
  cases         the named rays of the issue and the fixed-seed random ones.
"""
import ctypes as C

import numpy as np

import _rays as R
from _hostlib import HostLib, dp as _dp, f64 as _f64

TINY = R.TINY


def _declare(L):
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_int32)
    L.ryp_step_bound.argtypes, L.ryp_step_bound.restype = [C.c_int, C.c_int, C.c_double], C.c_longlong
    L.ryp_refusal.argtypes, L.ryp_refusal.restype = [dp, dp, C.c_int], C.c_int
    L.ryp_image.argtypes, L.ryp_image.restype = [C.c_int, dp, dp, lp, dp], None
    L.ryp_walk.argtypes, L.ryp_walk.restype = [C.c_int, C.c_int, ip, C.c_longlong, dp, dp, dp, lp, lp, C.c_longlong, lp, dp, dp], C.c_longlong


lib = HostLib("rays_periodic", "ray_periodic_check.cpp", ("ftte_ray_math.h", "ftte_math.h"), "the periodic ray walk", _declare)
SOURCE = lib.source


def step_bound(n, max_level, tmax):
    return int(lib().ryp_step_bound(n, max_level, float(tmax)))


def refusal(o, tmax, n):
    """0 a good ray, 1 a tmax absent or not > 0, 2 an origin too far away"""
    o = _f64(o)
    return int(lib().ryp_refusal(_dp(o), _dp(None if tmax is None else _f64([tmax])), n))


def image(n, o, d):
    """(w [3], o' [3]) a periodic ray starts in"""
    o, d, w, local = _f64(o), _f64(d), np.zeros(3, dtype=np.int64), np.zeros(3)
    lib().ryp_image(n, _dp(o), _dp(d), R._lp(w), _dp(local))
    return w, local


class Walk(R.Walk):
    """off[nray + 1], leaf, t_in, t_out per segment, steps[nray], start[nray][2] = 0, tmax: the header's periodic walk"""

    def __init__(self, tree, origins, directions, tmax):
        o, d, t = R.rays(origins, directions, tmax)
        assert t is not None and t.size == o.shape[0]
        nodes = R.node_array(tree)
        nray = o.shape[0]
        self.off, self.steps = np.zeros(nray + 1, dtype=np.int64), np.zeros(nray, dtype=np.int64)
        args = (tree.n, tree.max_level, None if nodes is None else nodes.ctypes.data_as(C.POINTER(C.c_int32)), nray, _dp(o), _dp(d), _dp(t), R._lp(self.off),
                R._lp(self.steps))
        total = lib().ryp_walk(*args, 0, None, None, None)
        assert total >= 0, f"ray {-1 - total} is refused or passed its step bound"
        self.leaf, self.t_in, self.t_out = np.zeros(total, dtype=np.int64), np.zeros(total), np.zeros(total)
        if total:
            assert lib().ryp_walk(*args, total, R._lp(self.leaf), _dp(self.t_in), _dp(self.t_out)) == total
        self.start = np.stack([np.zeros(nray), t], axis=1)
        self.o, self.d, self.tmax, self.n, self.nray = o, d, t, tree.n, nray


# ---- the independent statement

def brute(boxes, n, o, d, tmax):
    """(leaf, t_in, t_out) of one periodic ray over all leaves of all images of the box it can reach, sorted by t_in, chords > 0"""
    lo, h = boxes
    end = o + tmax * d
    spans = [range(int(np.floor(min(o[a], end[a]) / n)) - 1, int(np.floor(max(o[a], end[a]) / n)) + 2) for a in range(3)]
    shifts = np.array([(i, j, k) for i in spans[0] for j in spans[1] for k in spans[2]], dtype=np.float64) * n
    # the images first, with a margin (their boxes closed and a little more: this only spares work), then all their leaves
    reach = np.ones(shifts.shape[0], dtype=bool)
    for a in range(3):
        if d[a] == 0.0:
            reach &= (shifts[:, a] <= o[a]) & (o[a] <= shifts[:, a] + n)
    t_img_lo, t_img_hi, _ = R._slabs(shifts, shifts + n, o, d, tmax)
    reach &= t_img_hi >= t_img_lo - 1e-6
    shifts = shifts[reach]
    all_lo = (lo[None, :, :] + shifts[:, None, :]).reshape(-1, 3)
    all_h = np.tile(h, shifts.shape[0])
    t_lo, t_hi, inside = R._slabs(all_lo, all_lo + all_h[:, None], o, d, tmax)
    keep = np.nonzero(inside & (t_hi - t_lo > 0.0))[0]
    keep = keep[np.argsort(t_lo[keep], kind="stable")]
    return keep % lo.shape[0], t_lo[keep], t_hi[keep]


def compare(walk, boxes, r):
    """Ray r of the walk against the brute-force list under the stated condition: leaves of chord < TINY may be missing from either
    list, all others match in identity and order, t and chords within 1e-12 (tmax + n), the chords add up to tmax, the segments
    tile [0, tmax].  Returns (segments, tiny leaves dropped from either list, largest difference in t or a chord [cells])."""
    n, tmax = walk.n, walk.tmax[r]
    tol = 1e-12 * (tmax + n)
    leaf, a, b = walk.of(r)
    want_leaf, wa, wb = brute(boxes, n, walk.o[r], walk.d[r], tmax)
    big, want_big = (b - a) >= TINY, (wb - wa) >= TINY
    assert np.array_equal(leaf[big], want_leaf[want_big]), (r, leaf, want_leaf)
    worst = 0.0
    if big.any():
        worst = max(np.abs(a[big] - wa[want_big]).max(), np.abs(b[big] - wb[want_big]).max(), np.abs((b - a)[big] - (wb - wa)[want_big]).max())
    assert worst <= tol, (r, worst)
    assert abs((b - a).sum() - tmax) <= tol and abs((wb - wa).sum() - tmax) <= tol, (r, (b - a).sum(), (wb - wa).sum(), tmax)
    assert leaf.size and a[0] == 0.0 and b[-1] == tmax, r
    assert np.all(b > a) and np.all(a[1:] == b[:-1]), r
    return leaf.size, int((~big).sum() + (~want_big).sum()), worst


# ---- the cases

def diagonal_length(n, boxes=2):
    """t of the far corner of the last box on the body diagonal from a corner, by the walk's own expression (far - o') inv"""
    return (float(boxes) * n) * (1.0 / (1.0 / np.sqrt(3.0)))


def named_rays(n):
    """the issue's named rays on an n^3 base grid (n >= 4): (what, origin, direction, tmax)"""
    r3, r2 = 1.0 / np.sqrt(3.0), 1.0 / np.sqrt(2.0)
    n = float(n)
    out = [("the body diagonal over two boxes", (0, 0, 0), (r3, r3, r3), diagonal_length(n)),
           ("the other way along it", (n, n, n), (-r3, -r3, -r3), diagonal_length(n)),
           ("in a face plane", (0.1, 2.0, 0.3), (r2, 0.0, r2), 3.3 * n),
           ("in a face plane of the refined corner", (0.05, 0.25, 0.02), (-r2, 0.0, r2), 2.7 * n),
           ("in the box's face plane", (0.1, 0.0, 0.3), (r2, 0.0, -r2), 2.2 * n),
           ("along a box edge", (0.0, 0.0, 0.5), (0.0, 0.0, 1.0), 2.5 * n),
           ("along the opposite edge", (n, n, 1.5), (0.0, 0.0, -1.0), 2.5 * n),
           ("on the box's face, outwards", (n, 0.5, 0.5), (1.0, 0.0, 0.0), 1.5 * n),
           ("on the box's face, inwards", (n, 0.5, 0.5), (-1.0, 0.0, 0.0), 1.5 * n),
           ("on the near face, outwards", (0.0, 0.3, 0.6), unit((-1.0, 0.2, 0.1)), 1.5 * n),
           ("on the corner, outwards", (n, n, n), (r3, r3, r3), 5.0),
           ("on the corner, inwards", (n, n, n), (-r3, -r3, -r3), 5.0),
           ("on the opposite corner, outwards", (0, 0, 0), (-r3, -r3, -r3), 5.0),
           ("negative zeros", (0.5, 0.5, n), (-0.0, -0.0, -1.0), 2.0 * n),
           ("a negative zero for an origin", (-0.0, 0.5, 0.5), (-1.0, -0.0, 0.0), 2.0 * n),
           ("a tmax inside a leaf", (0.3, 0.2, 0.1), (r3, r3, r3), 2.0 * n + 1.7),
           ("a tmax on a box face", (0.5, 0.5, 0.0), (0.0, 0.0, 1.0), 2.0 * n),
           ("a tmax shorter than the first leaf", (0.3, 0.2, 0.1), (r3, r3, r3), 0.01),
           ("1 000 boxes away, o' exact", (1000.0 * n + 0.5, -1000.0 * n + 0.25, 0.375), (r3, -r3, r3), 3.0 * n),
           ("1 000 boxes away, o' rounded", (1000.0 * n + 0.3, -1000.0 * n + 0.6, -0.45), (-r3, r3, r3), 3.0 * n)]
    for what, o, d, tmax in axis_rays(n):
        out.append((what, o, d, tmax))
    return out


def axis_rays(n, boxes=3):
    """all six +-e_a of `boxes` boxes from a base cell's face through dyadic transverse coordinates: (what, origin, direction, tmax)"""
    out = []
    for a in range(3):
        for sign in (1.0, -1.0):
            o = [0.125, 0.625, n - 0.5]
            o[a] = 0.0 if sign > 0 else float(n)
            d = [0.0, 0.0, 0.0]
            d[a] = sign
            out.append((f"{'+' if sign > 0 else '-'}e_{a}", tuple(o), tuple(d), float(boxes) * n))
    return out


def unit(v):
    return tuple(R.unit(v).tolist())


def random_rays(n, count, seed, shortest=0.01, longest=5.0):
    """origins inside and up to a box outside, directions over the sphere with one zero component in every tenth ray, lengths up to
    `longest` boxes"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.0 * n, 2.0 * n, (count, 3))
    inside = rng.random(count) < 0.5
    o[inside] = rng.uniform(0.0, n, (int(inside.sum()), 3))
    d = rng.normal(size=(count, 3))
    tenth = np.arange(0, count, 10)
    d[tenth, (tenth // 10) % 3] = 0.0
    d = R.unit(d)
    tmax = rng.uniform(shortest * n, longest * n, count)
    return o, d, tmax
