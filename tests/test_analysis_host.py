"""The analysis modes (slice and projected maps, clumping, gas PDF) without a GPU: the numpy restatement of tests/_analysis.py --
the yardstick of the GPU tests -- against the reference's own compiled lines (tests/golden/analysis_*.npz,
make_golden_analysis.py), the library's context-free axis arithmetic against the same tables, and the refusals that need no
device.  Maps, axis tables and the PDF bit for bit; the clumping sums to 1e-12 relative, the bound DESIGN.md 3d' uses for
computeMass against the reference's sequential sums."""
import ctypes as C

import numpy as np
import pytest

import _analysis as A
import radiativetransfer_amd as rt
from radiativetransfer_amd import _lib

GOLDENS = ["analysis_refined6", "analysis_ingested12", "analysis_uniform16", "analysis_uniform12"]
_TREES = {}


def jobs(g):
    for q in range(g["jobs_kind"].size):
        yield q, int(g["jobs_kind"][q]), int(g["jobs_izone"][q]), tuple(int(s) for s in g["jobs_shape"][q]), [float(v) for v in g["jobs_p"][q]]


def tree_of(name, g):
    if name not in _TREES:
        _TREES[name] = A.Tree(int(g["n"]), g["level"])
    return _TREES[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_entry_points_are_exported_and_check_their_arguments():
    lib = _lib.load()
    for name in ("ftte_map_axis", "ftte_slice_axis", "ftte_map_depth", "ftte_slice_map", "ftte_slice_map_device", "ftte_project_map",
                 "ftte_project_map_device", "ftte_clumping", "ftte_gas_pdf", "ftte_star_pdf"):
        assert hasattr(lib, name)
    base, frac = (C.c_int32 * 4)(), (C.c_double * 4)()
    for fn in (lib.ftte_map_axis, lib.ftte_slice_axis):
        assert fn(6, 4, 0.5, 1.0, base, frac) == 0
        assert fn(0, 4, 0.5, 1.0, base, frac) == -1
        assert fn(6, 0, 0.5, 1.0, base, frac) == -1
        assert fn(6, 4, 0.5, 0.0, base, frac) == -1       # zoom <= 0
        assert fn(6, 4, 0.5, -2.0, base, frac) == -1
        assert fn(6, 4, 0.5, float("nan"), base, frac) == -1
        assert fn(6, 4, 1.7, 2.0, base, frac) == -1       # the window starts beyond the box: i0 > n
        assert fn(6, 4, 0.5, 1.0, None, frac) == -1
        assert fn(6, 4, 0.5, 1.0, base, None) == -1
    a, b = C.c_int32(), C.c_int32()
    assert lib.ftte_map_depth(6, 0.5, 0.0, C.byref(a), C.byref(b)) == -1
    assert lib.ftte_map_depth(6, 0.5, 1.0, None, C.byref(b)) == -1
    centre = (C.c_double * 3)(0.5, 0.5, 0.5)
    out = (C.c_float * 4)()
    assert lib.ftte_slice_map(None, 1, 2, 2, centre, 1.0, 0.5, None, out) == -1
    assert lib.ftte_project_map(None, 1, 2, 2, centre, 1.0, 0, None, out) == -1
    assert lib.ftte_slice_map_device(None, 1, 2, 2, centre, 1.0, 0.5, None, out) == -1
    assert lib.ftte_project_map_device(None, 1, 2, 2, centre, 1.0, 0, None, out) == -1
    assert lib.ftte_clumping(None, None, None, None) == -1
    assert lib.ftte_gas_pdf(None, None, None) == -1
    assert lib.ftte_star_pdf(None, 0, None, None, None, None) == -1


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_every_golden_map(golden, name):
    g = golden(name)
    T, box = tree_of(name, g), float(g["box"])
    nan_pixels = 0
    for q, kind, izone, shape, p in jobs(g):
        if kind == 1:
            got = A.slice_map(T, g["HI"], izone, shape, p[0])
        else:
            got = A.project_map(T, g["abun2"], g["rho"], box, izone, shape, p[:3], p[3])
        want = g[f"job{q}_map"]
        nan_pixels += int(np.isnan(want).sum())
        assert got.dtype == np.float32 and same_bits(got, want), f"{name} job {q}: kind {kind} izone {izone} {shape} {p}"
    if name == "analysis_refined6":
        assert nan_pixels > 0  # the column of rho = 0: totalMass = 0 and the reference's pixel is NaN


@pytest.mark.parametrize("name", GOLDENS)
def test_map_axis_equals_the_reference_tables_bit_for_bit(golden, name):
    """ftte_map_axis against the driver's i0, xnew (equiSources.f90:703-709), ftte_slice_axis against the reader's
    (readCellArray.f90:126-132), ftte_map_depth against kstart, kend, for every window and map size of the goldens"""
    g = golden(name)
    n = int(g["n"])
    seen = set()
    for q, kind, izone, shape, p in jobs(g):
        centre, zoom = ((0.5, 0.5), 1.0) if kind == 1 else (p[:2], p[3])
        lib_axis, own_axis = (rt.slice_axis, A.slice_axis) if kind == 1 else (rt.map_axis, A.map_axis)
        for nmap, c, i0, xnew in ((shape[0], centre[0], g[f"job{q}_i0"], g[f"job{q}_xnew"]), (shape[1], centre[1], g[f"job{q}_j0"], g[f"job{q}_ynew"])):
            base, frac = lib_axis(n, nmap, c, zoom)
            assert np.array_equal(base, i0) and base.dtype == np.int32
            assert np.array_equal(frac.view(np.uint64), xnew.view(np.uint64))
            own = own_axis(n, nmap, c, zoom)
            assert np.array_equal(own[0], i0) and np.array_equal(own[1].view(np.uint64), xnew.view(np.uint64))
            seen.add((kind, nmap, c, zoom))
        if kind == 2:
            assert rt.map_depth(n, p[2], p[3]) == tuple(int(k) for k in g[f"job{q}_k"]) == A.map_depth(n, p[2], p[3])
    assert len(seen) >= 4


def test_the_two_axis_forms_are_two():
    """the reader divides in single precision, the driver multiplies and divides in double: the same cells, other last bits"""
    a, b = rt.map_axis(6, 37), rt.slice_axis(6, 37)
    assert np.array_equal(a[0], b[0])
    assert not np.array_equal(a[1], b[1])
    assert np.allclose(a[1], b[1], rtol=0, atol=1e-6)


def test_depth_clamps(golden):
    assert rt.map_depth(6, 0.5, 1.0) == (1, 6)        # zend = 1: int(1*nz)+1 = nz+1, clamped to nz
    assert rt.map_depth(6, 0.5, 2.0) == (2, 5)
    assert rt.map_depth(12, 0.9, 3.0) == (9, 12)
    assert rt.map_depth(12, 0.05, 3.0) == (1, 3)


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_censuses(golden, name):
    g = golden(name)
    c = A.clumping(g["level"], g["rho"])
    for key in ("volSum", "volSumDensity", "volSumDensity2", "clumping"):
        want = float(g[key])
        print(f"{name}: {key} {c[key]!r} against the reference's {want!r}, relative {abs(c[key] / want - 1):.2e}")
        assert abs(c[key] - want) <= 1e-12 * abs(want)
    pdf, outside = A.gas_pdf(g["level"], g["rho"])
    assert np.array_equal(pdf, g["pdfGas"]) and outside == float(g["pdfGasOutside"])
    assert pdf.sum() + outside == c["volSum"] == float(int(g["n"]) ** 3)


def test_the_pdf_goldens_keep_away_from_the_bin_edges(golden):
    """what lets the GPU test demand the reference's PDF exactly: no leaf within 8 ulp of a place where its bin changes"""
    kinds = set()
    for name in GOLDENS:
        g = golden(name)
        tmp = A.pdf_log(g["rho"])
        bins = A.pdf_bins(tmp)
        finite = np.isfinite(tmp)
        lo, hi = tmp.copy(), tmp.copy()
        for _ in range(8):
            lo[finite], hi[finite] = np.nextafter(lo[finite], -np.inf), np.nextafter(hi[finite], np.inf)
        assert np.array_equal(A.pdf_bins(lo), bins) and np.array_equal(A.pdf_bins(hi), bins)
        if (g["rho"] == 0).any():
            kinds.add("zero")
        if (tmp[finite] < A.APDF).any():
            kinds.add("below")
        if (tmp[finite] > A.BPDF).any():
            kinds.add("above")
    assert kinds == {"zero", "below", "above"}


def test_star_pdf_restatement_counts_every_star(golden):
    g = golden("analysis_refined6")
    cells = np.arange(0, g["level"].size, 7)
    pdf, outside, mean = A.star_pdf(g["rho"], g["HI"], cells)
    assert pdf.sum() + outside == cells.size and outside > 0
    assert mean == pytest.approx(float(np.mean(g["HI"][cells])), rel=1e-6)
