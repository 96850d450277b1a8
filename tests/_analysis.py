"""A numpy restatement of the reference's analysis modes, vectorised over pixels, for the tests of the device kernels:

  slice_map     readCellArray.f90:116-140 with sliceCell :189-230
  project_map   equiSources.f90:685-719 with projectVariableToMap :4914-4954 (mode 0), and the library's own path integral (mode 1)
  clumping      :661-676 with computeClumping :4711-4735
  gas_pdf       :814-822 with computeGasPDF :4682-4709
  star_pdf      :787-813

Every operation of the maps is the reference's, in its order and its precision: numpy rounds every product and every sum on its
own, the projection's pixel is a float32 that is widened and rounded again for every leaf, and a pixel meets its leaves in the
reference's order (base cells kstart..kend, below a refined cell the depth child k = 1 before k = 2).  tests/test_analysis_host.py
holds it against the reference's own compiled lines (tests/golden/analysis_*.npz).
"""
import numpy as np

F32 = np.float32
MH = float(F32(1.6726231e-24))
MSUN = float(F32(1.98892e33))
PSI = float(F32(0.76))
PC = float(F32(3.08568025e18))
NPDF, APDF, BPDF = 50, -8.0, 3.0

# rotateIndicesModule.f90:14-111 as data: per storage index (icell, jcell, kcell) the sweep index (0 i, 1 j, 2 k) it takes, +4 mirrored
_ZONES = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1 | 4), (1, 0, 2 | 4), (2, 1, 0 | 4), (0, 1 | 4, 2 | 4), (1, 2 | 4, 0 | 4),
          (2, 0 | 4, 1 | 4), (0, 2 | 4, 1), (1, 0 | 4, 2), (2, 1 | 4, 0)]


def zone(izone):
    """(src[3], mirror[3]) of an izone 1..24"""
    row = _ZONES[(izone - 1) % 12]
    src = [r & 3 for r in row]
    mirror = [bool(r & 4) for r in row]
    if izone > 12:
        mirror[0] = not mirror[0]
    return src, mirror


def rotate(izone, ijk, ext):
    """rotateIndices on 1-based (arrays of) sweep indices -> storage indices"""
    src, mirror = zone(izone)
    return [ext + 1 - ijk[src[a]] if mirror[a] else ijk[src[a]] for a in range(3)]


def child_map(izone):
    """storage position 4(a-1)+2(b-1)+(c-1) of sweep child 4(i-1)+2(j-1)+(k-1): is/js/ks of equiSources.f90:690-696"""
    out = np.zeros(8, dtype=np.int64)
    for i in (1, 2):
        for j in (1, 2):
            for k in (1, 2):
                a, b, c = rotate(izone, (i, j, k), 2)
                out[4 * (i - 1) + 2 * (j - 1) + (k - 1)] = 4 * (a - 1) + 2 * (b - 1) + (c - 1)
    return out


class Tree:
    """The tree of a depth-first level list (readCellArray.f90:154-187): nodes 0..n^3-1 are the base cells in storage order (kcell
    fastest), the eight children of a refined node are contiguous in storage order; child0[node] or -1, leaf[node] or -1."""

    def __init__(self, n, level):
        level = np.asarray(level, dtype=np.int64)
        self.n, self.ncell = int(n), level.size
        child0, leaf = [-1] * n ** 3, [-1] * n ** 3
        base_of_leaf = np.zeros(level.size, dtype=np.int64)
        cursor = 0
        for base in range(n ** 3):
            stack = [(base, 0)]
            while stack:
                node, lev = stack.pop()
                if level[cursor] == lev:
                    leaf[node] = cursor
                    base_of_leaf[cursor] = base
                    cursor += 1
                else:
                    assert level[cursor] > lev, "error in levels"
                    first = len(child0)
                    child0[node] = first
                    child0 += [-1] * 8
                    leaf += [-1] * 8
                    stack += [(first + q, lev + 1) for q in range(7, -1, -1)]
        assert cursor == level.size
        self.child0, self.leaf = np.array(child0, dtype=np.int64), np.array(leaf, dtype=np.int64)
        self.level, self.base_of_leaf = level, base_of_leaf
        self.max_level = int(level.max())


def _window(centre, zoom):
    start = max(centre - 0.5 / zoom, 0.0)
    end = min(start + 1.0 / zoom, 1.0)
    return start, end


def map_axis(n, nmap, centre=0.5, zoom=1.0):
    """i0 (1-based) and xnew of equiSources.f90:703-709: the product and the quotient left to right in double"""
    start, end = _window(centre, zoom)
    fi = (np.arange(1, nmap + 1).astype(F32) - F32(0.5)).astype(np.float64)
    x0 = (end - start) * fi / float(F32(nmap)) + start
    i0 = (x0 * n).astype(np.int64) + 1
    return i0, x0 * float(F32(n)) - (i0 - 1).astype(F32).astype(np.float64)


def slice_axis(n, nmap, centre=0.5, zoom=1.0):
    """the same with the reader's x0, the single-precision quotient of readCellArray.f90:126, inside the window"""
    start, end = _window(centre, zoom)
    q = ((np.arange(1, nmap + 1).astype(F32) - F32(0.5)) / F32(nmap)).astype(np.float64)
    x0 = (end - start) * q + start
    i0 = (x0 * n).astype(np.int64) + 1
    return i0, x0 * float(F32(n)) - (i0 - 1).astype(F32).astype(np.float64)


def map_depth(n, centre=0.5, zoom=1.0):
    zstart, zend = max(centre - 0.5 / zoom, 0.0), min(centre + 0.5 / zoom, 1.0)
    return max(int(zstart * n) + 1, 1), min(int(zend * n) + 1, n)


def _half(x):
    upper = ~(x < 0.5)
    return upper.astype(np.int64), np.where(upper, 2.0 * x - 1.0, 2.0 * x)


def _base_nodes(izone, n, i0, j0, k0):
    a, b, c = rotate(izone, (i0, j0, k0), n)
    return ((a - 1) * n + (b - 1)) * n + (c - 1)


def slice_map(tree, value, izone, shape, zslice, centre=(0.5, 0.5), zoom=1.0):
    """float32 [nxmap][nymap]"""
    n = tree.n
    i0, xn = slice_axis(n, shape[0], centre[0], zoom)
    j0, yn = slice_axis(n, shape[1], centre[1], zoom)
    k0 = int(zslice * n) + 1
    zn = zslice * float(F32(n)) - float(F32(k0 - 1))
    I0, J0 = np.meshgrid(i0, j0, indexing="ij")
    x, y = (a.copy().ravel() for a in np.meshgrid(xn, yn, indexing="ij"))
    z = np.full(x.shape, zn)
    node = _base_nodes(izone, n, I0.ravel(), J0.ravel(), np.full(x.shape, k0, dtype=np.int64))
    cmap = child_map(izone)
    while True:
        ref = tree.child0[node] >= 0
        if not ref.any():
            break
        a, xr = _half(x[ref])
        b, yr = _half(y[ref])
        c, zr = _half(z[ref])
        node[ref] = tree.child0[node[ref]] + cmap[4 * a + 2 * b + c]
        x[ref], y[ref], z[ref] = xr, yr, zr
    return np.asarray(value, dtype=np.float64)[tree.leaf[node]].astype(F32).reshape(shape)


def project_map(tree, value, rho, box, izone, shape, centre=(0.5, 0.5, 0.5), zoom=1.0, mode=0):
    """float32 [nxmap][nymap]; mode 0 the reference's mass-weighted mean, mode 1 the path integral sum value * leaf size [cm]"""
    n = tree.n
    value, rho = np.asarray(value, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    i0, xn = map_axis(n, shape[0], centre[0], zoom)
    j0, yn = map_axis(n, shape[1], centre[1], zoom)
    kstart, kend = map_depth(n, centre[2], zoom)
    I0, J0 = (a.ravel() for a in np.meshgrid(i0, j0, indexing="ij"))
    X, Y = (a.ravel() for a in np.meshgrid(xn, yn, indexing="ij"))
    npix = X.size
    pixel, total, path = np.zeros(npix, dtype=F32), np.zeros(npix), np.zeros(npix)
    cmap = child_map(izone)
    e25, e21 = float(F32(1.e25)), float(F32(1.e21))

    def visit(node, x, y, size, idx):
        ref = tree.child0[node] >= 0
        if (~ref).any():
            at, cell = idx[~ref], tree.leaf[node[~ref]]
            if mode == 0:
                s = size / e21
                tmp = (rho[cell] * e25) * (s * s * s)
                pixel[at] = (pixel[at].astype(np.float64) + value[cell] * tmp).astype(F32)
                total[at] = total[at] + tmp
            else:
                path[at] = path[at] + value[cell] * size
        if ref.any():
            a, xr = _half(x[ref])
            b, yr = _half(y[ref])
            for c in (0, 1):
                visit(tree.child0[node[ref]] + cmap[4 * a + 2 * b + c], xr, yr, size / 2.0, idx[ref])

    everyone = np.arange(npix)
    for k0 in range(kstart, kend + 1):
        visit(_base_nodes(izone, n, I0, J0, np.full(npix, k0, dtype=np.int64)), X, Y, box / float(n), everyone)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (pixel.astype(np.float64) / total).astype(F32) if mode == 0 else path.astype(F32)
    return out.reshape(shape)


def clumping(level, rho):
    """volSum, sum nh 2^-3L, sum nh^2 2^-3L (each term as :4729-4732; the sums pairwise) and the printed ratio of :672-674"""
    level, rho = np.asarray(level, dtype=np.int64), np.asarray(rho, dtype=np.float64)
    nh = PSI * rho / MH
    p = np.ldexp(1.0, 3 * level)
    vol, dens, dens2 = float(np.sum(1.0 / p)), float(np.sum(nh / p)), float(np.sum(nh * nh / p))
    d, d2 = dens / vol, dens2 / vol
    return dict(volSum=vol, volSumDensity=dens, volSumDensity2=dens2, clumping=d2 / (d * d), volume=vol, mean_nh=d)


def pdf_log(rho):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log10(np.asarray(rho, dtype=np.float64) / MSUN * (PC * PC * PC))


def pdf_bins(tmp):
    """the bin 0..49 of :4701-4702, or 50 for `outside`"""
    inside = (tmp > APDF) & (tmp < BPDF)
    with np.errstate(invalid="ignore"):
        b = ((np.where(inside, tmp, APDF) - APDF) / (BPDF - APDF) * float(F32(NPDF))).astype(np.int64)
    return np.where(inside, np.clip(b, 0, NPDF - 1), NPDF)


def gas_pdf(level, rho):
    """(pdfGas[50], pdfGasOutside): every term 2^-3L and every sum is exact"""
    bins = pdf_bins(pdf_log(rho))
    full = np.bincount(bins, weights=np.ldexp(1.0, -3 * np.asarray(level, dtype=np.int64)), minlength=NPDF + 1)
    return full[:NPDF], float(full[NPDF])


def star_pdf(rho, HI, cells):
    """(pdfStar[50], pdfStarOutside, meanHostDensity / float(nStarsSpecificAge))"""
    cells = np.asarray(cells, dtype=np.int64)
    full = np.bincount(pdf_bins(pdf_log(np.asarray(rho)[cells])), minlength=NPDF + 1)
    mean = 0.0
    for h in np.asarray(HI, dtype=np.float64)[cells]:
        mean = mean + float(h)
    return full[:NPDF].astype(np.int32), int(full[NPDF]), mean / float(F32(cells.size))
