"""The analysis modes on the GPU -- slice and projected maps, the clumping factor, the gas and the stellar PDF of the
device-resident medium -- against the reference's own compiled lines (tests/golden/analysis_*.npz, make_golden_analysis.py) and
the numpy restatement of tests/_analysis.py (held against the same goldens by test_analysis_host.py): maps bit for bit (NaN where
the reference has NaN), the PDF exactly, the clumping sums to 1e-12 relative (the bound DESIGN.md 3d' uses for computeMass against
the reference's sequential sums) and the same bits call after call; a grid beyond one workgroup; freshness after the medium
changes; the _device variants; the refusals; the owner's buffers; the Fortran host."""
import os
import subprocess

import numpy as np
import pytest

import _analysis as A
import radiativetransfer_amd as rt
from radiativetransfer_amd import synthetic

pytestmark = pytest.mark.gpu

GOLDENS = ["analysis_refined6", "analysis_ingested12", "analysis_uniform16", "analysis_uniform12"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stellar():
    st = rt.StellarTransfer()
    yield st
    st.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(np.isnan(a), np.isnan(b))
            and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32)))


def jobs(g):
    for q in range(g["jobs_kind"].size):
        yield q, int(g["jobs_kind"][q]), int(g["jobs_izone"][q]), tuple(int(s) for s in g["jobs_shape"][q]), [float(v) for v in g["jobs_p"][q]]


def load(st, g, rho="rho"):
    st.set_grid(int(g["n"]), g["level"], float(g["box"]))
    st.set_medium(g["HI"], g["HI"], g["HI"], None if rho is None else g[rho], g["abun2"], 0)  # (the helium species are not read)


def close(a, b, rel=1e-12):
    return abs(a - b) <= rel * abs(b)


@pytest.mark.parametrize("name", GOLDENS)
def test_every_golden_map_bit_for_bit(stellar, golden, name):
    """every slice and projection of the goldens: 50x37 (a partly filled wavefront), 7x5 (a map smaller than a wavefront and coarser
    than the base grid), 200x3 (more pixels than leaves along a row), 13x11 under all 24 izones; the column of rho = 0 gives NaN"""
    g = golden(name)
    load(stellar, g)
    izones, nans = set(), 0
    for q, kind, izone, shape, p in jobs(g):
        if kind == 1:
            got = stellar.slice_map(izone, shape, p[0])
        else:
            got = stellar.project_map(izone, shape, p[:3], p[3])
        want = g[f"job{q}_map"]
        assert got.shape == shape and same_bits(got, want), f"{name} job {q}: kind {kind} izone {izone} {shape} {p}"
        izones.add((kind, izone))
        nans += int(np.isnan(got).sum())
    if name == "analysis_refined6":
        assert {(k, z) for k in (1, 2) for z in range(1, 25)} <= izones and nans > 0


@pytest.mark.parametrize("name", GOLDENS[:3])
def test_path_integral_equals_the_restatement(stellar, golden, name):
    g = golden(name)
    load(stellar, g)
    T, box = A.Tree(int(g["n"]), g["level"]), float(g["box"])
    done = 0
    for q, kind, izone, shape, p in jobs(g):
        if kind != 2 or (shape == (13, 11) and izone % 5):
            continue
        for value in (None, g["HI"]):
            got = stellar.project_map(izone, shape, p[:3], p[3], mode=1, value=value)
            want = A.project_map(T, g["abun2"] if value is None else value, g["rho"], box, izone, shape, p[:3], p[3], mode=1)
            assert same_bits(got, want) and np.isfinite(got).all() and (got > 0).all()
        # a value array of the caller's in the reference's mode, and in a slice
        got = stellar.project_map(izone, shape, p[:3], p[3], value=g["HI"])
        assert same_bits(got, A.project_map(T, g["HI"], g["rho"], box, izone, shape, p[:3], p[3]))
        assert same_bits(stellar.slice_map(izone, shape, 0.37, value=g["abun2"]), A.slice_map(T, g["abun2"], izone, shape, 0.37))
        done += 1
    assert done >= 3


def test_windowed_slice_equals_the_restatement(stellar, golden):
    """the reader has no window; the library's follows ftte_slice_axis"""
    g = golden("analysis_refined6")
    load(stellar, g)
    T = A.Tree(int(g["n"]), g["level"])
    for izone, centre, zoom in ((2, (0.5, 0.5), 2.0), (19, (0.1, 0.93), 3.0)):
        got = stellar.slice_map(izone, (50, 37), 0.6180339887498949, centre, zoom)
        assert same_bits(got, A.slice_map(T, g["HI"], izone, (50, 37), 0.6180339887498949, centre, zoom))


@pytest.mark.parametrize("name", GOLDENS[:3])
def test_censuses_against_the_reference(stellar, golden, name):
    g = golden(name)
    load(stellar, g)
    first = stellar.clumping()
    sums = dict(volSum=first["volume"], volSumDensity=first["mean_nh"] * first["volume"],
                volSumDensity2=first["clumping"] * first["mean_nh"] ** 2 * first["volume"], clumping=first["clumping"])
    for key, got in sums.items():
        print(f"{name}: {key} {got!r} against the reference's {float(g[key])!r}, relative {abs(got / float(g[key]) - 1):.2e}")
        assert close(got, float(g[key]))
    assert first["volume"] == float(g["volSum"])                       # powers of two: exact in any order
    assert close(first["mean_nh"], float(g["volSumDensity"]) / float(g["volSum"]))
    assert stellar.clumping() == first                                 # identical bits across two calls
    pdf, outside = stellar.gas_pdf()
    assert np.array_equal(pdf, g["pdfGas"]) and outside == float(g["pdfGasOutside"])
    assert stellar.gas_pdf()[1] == outside
    cells = np.arange(0, g["level"].size, 7)[::-1].copy()
    got = stellar.star_pdf(cells)
    want = A.star_pdf(g["rho"], g["HI"], cells)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:] and got[0].sum() + got[1] == cells.size
    empty = stellar.star_pdf([])
    assert empty[0].sum() == 0 and empty[1] == 0 and np.isnan(empty[2])


def test_beyond_one_workgroup(stellar):
    """64^3 base with the central 16^3 block refined once: 290816 leaves, 256x256 maps (256 workgroups), censuses over 1136
    workgroups"""
    n, box = 64, 4.0e24
    level = synthetic.refine_levels(n, [(i, j, k) for i in range(24, 40) for j in range(24, 40) for k in range(24, 40)])
    T = A.Tree(n, level)
    rng = np.random.default_rng(4711)
    rho = A.MSUN / A.PC ** 3 * 10.0 ** rng.normal(-3.0, 1.0, level.size)
    HI, abun2 = 10.0 ** rng.uniform(-9.0, 1.0, level.size), 0.02 * 10.0 ** rng.normal(0.0, 0.5, level.size)
    stellar.set_grid(n, level, box)
    stellar.set_medium(HI, HI, HI, rho, abun2, 0)
    for izone in (3, 14):
        assert same_bits(stellar.slice_map(izone, (256, 256), 0.47), A.slice_map(T, HI, izone, (256, 256), 0.47))
        for mode in (0, 1):
            got = stellar.project_map(izone, (256, 256), (0.5, 0.5, 0.5), 2.0, mode)
            assert same_bits(got, A.project_map(T, abun2, rho, box, izone, (256, 256), (0.5, 0.5, 0.5), 2.0, mode))
    want = A.clumping(level, rho)
    got = stellar.clumping()
    for key in ("clumping", "volume", "mean_nh"):
        assert close(got[key], want[key]), key
    assert got["volume"] == float(n ** 3)
    # the PDF is exact where no leaf lies within 8 ulp of a bin edge (a device log10 may differ from the host's in the last bit)
    tmp = A.pdf_log(rho)
    lo, hi = tmp.copy(), tmp.copy()
    for _ in range(8):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    assert np.array_equal(A.pdf_bins(lo), A.pdf_bins(tmp)) and np.array_equal(A.pdf_bins(hi), A.pdf_bins(tmp))
    pdf, outside = stellar.gas_pdf()
    want_pdf, want_outside = A.gas_pdf(level, rho)
    assert np.array_equal(pdf, want_pdf) and outside == want_outside and pdf.sum() + outside == float(n ** 3)


def test_maps_follow_the_medium(stellar, golden):
    """no copy can go stale: after set_medium with other species and after an expansion the maps show the new medium"""
    g = golden("analysis_refined6")
    T, box = A.Tree(int(g["n"]), g["level"]), float(g["box"])
    load(stellar, g)
    shape = (50, 37)
    first_slice = stellar.slice_map(2, shape, 0.31)
    first_map = stellar.project_map(3, shape, (0.5, 0.5, 0.5), 1.0)
    HI2, abun2 = g["HI"][::-1].copy(), g["abun2"][::-1].copy()
    stellar.set_medium(HI2, HI2, HI2, g["rho"], abun2, 0)
    second_slice = stellar.slice_map(2, shape, 0.31)
    second_map = stellar.project_map(3, shape, (0.5, 0.5, 0.5), 1.0)
    assert same_bits(second_slice, A.slice_map(T, HI2, 2, shape, 0.31)) and not same_bits(second_slice, first_slice)
    assert same_bits(second_map, A.project_map(T, abun2, g["rho"], box, 3, shape, (0.5, 0.5, 0.5), 1.0)) and not same_bits(second_map, first_map)
    # an expansion scales rho and the species of the leaves around a star
    nh = A.PSI * g["rho"] / A.MH
    src = int(np.argmax(nh))
    before = stellar.clumping()
    coef, changed = stellar.expand_hii_regions([src], np.array([[0.3 * box, 0.25, float(nh[src])]]))
    assert changed > 0
    rho3, HI3 = stellar.density(), stellar.medium()[0]
    assert not np.array_equal(rho3, g["rho"])
    assert same_bits(stellar.slice_map(2, shape, 0.31), A.slice_map(T, HI3, 2, shape, 0.31))
    third_map = stellar.project_map(3, shape, (0.5, 0.5, 0.5), 1.0)
    assert same_bits(third_map, A.project_map(T, abun2, rho3, box, 3, shape, (0.5, 0.5, 0.5), 1.0)) and not same_bits(third_map, second_map)
    after = stellar.clumping()
    assert after != before and close(after["clumping"], A.clumping(g["level"], rho3)["clumping"])
    pdf, outside = stellar.gas_pdf()
    assert pdf.sum() + outside == before["volume"]


def test_device_arrays_give_the_host_arrays_maps(golden):
    """one frequency group of a swept J and one plane of the point-source rates, read where they lie"""
    import torch
    g, tables = golden("analysis_refined6"), golden("point16_homogeneous")["tables"]
    n, nc, box = int(g["n"]), g["level"].size, float(g["box"])
    beta = np.array([[6.3e-18, 1.2e-18, 2.0e-19], [0.0, 7.4e-18, 1.5e-18], [0.0, 0.0, 1.6e-18]])
    HI = 1e-7 * g["HI"]                     # cells around optical depth one; photon rates that leave the rates inside float32's range
    with rt.StellarTransfer() as st:
        st.set_grid(n, g["level"], box)
        st.set_medium(HI, 0.08 * HI, 0.01 * HI, g["rho"], g["abun2"], 0)
        st.set_rate_tables(tables)
        st.set_zero_rates()
        st.point_sources([10, 200], np.array([1e-40, 4e-41]))
        st.compute_opacities_from_medium(beta)
        J = torch.zeros((3, nc), dtype=torch.float64, device=torch.device("cuda", 0))
        st.transport_device(*rt.healpix_directions(1), np.array([2e-22, 1e-22, 3e-23]), J.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        J.div_(J.abs().max())               # (a map is float32: keep the values inside its range whatever the units)
        torch.cuda.synchronize()
        J_host, rates_host = J.cpu().numpy(), st.rates()
        assert J_host[1].max() > 0 and rates_host[0].max() > 0
        for ptr, host in ((J.data_ptr() + 8 * nc, J_host[1]), (st.rates_device_ptr(), rates_host[0])):
            for izone, shape in ((2, (50, 37)), (21, (7, 5))):
                a = st.slice_map(izone, shape, 0.43, value_device_ptr=ptr)
                assert same_bits(a, st.slice_map(izone, shape, 0.43, value=host)) and np.unique(a).size > 1 and np.isfinite(a).all()
                for mode in (0, 1):
                    a = st.project_map(izone, shape, (0.5, 0.5, 0.5), 1.0, mode, value_device_ptr=ptr)
                    assert same_bits(a, st.project_map(izone, shape, (0.5, 0.5, 0.5), 1.0, mode, value=host))


def _expect(code, fn, *args, **kw):
    with pytest.raises(rt.FtteError) as err:
        fn(*args, **kw)
    assert err.value.status == code, str(err.value)
    return str(err.value)


def test_refusals_and_the_owner(golden):
    g, u = golden("analysis_refined6"), golden("analysis_uniform16")
    shape, centre = (13, 11), (0.5, 0.5, 0.5)
    with rt.StellarTransfer() as probe:
        idle = probe.counter("device_objects")
    with rt.StellarTransfer() as st:
        assert "ftte_set_grid" in _expect("FTTE_ERR_STATE", st.slice_map, 1, shape, 0.5)                  # no grid
        st.set_grid(int(g["n"]), g["level"], float(g["box"]))
        for call in (lambda: st.slice_map(1, shape, 0.5), lambda: st.project_map(1, shape), st.clumping, st.gas_pdf,
                     lambda: st.star_pdf([0])):
            assert "medium" in _expect("FTTE_ERR_STATE", call)                                            # no medium
        st.set_medium(g["HI"], g["HI"], g["HI"], None, g["abun2"], 0)
        assert st.slice_map(1, shape, 0.5).shape == shape                                                 # only the value is read
        for call in (lambda: st.project_map(1, shape), st.clumping, st.gas_pdf, lambda: st.star_pdf([0])):
            assert "density" in _expect("FTTE_ERR_STATE", call)                                           # a medium without rho
        load(st, g)
        for izone in (0, 25, -3):
            _expect("FTTE_ERR_IZONE", st.slice_map, izone, shape, 0.5)
            _expect("FTTE_ERR_IZONE", st.project_map, izone, shape)
        for zslice in (-1e-9, 1.0, 1.5, float("nan")):
            _expect("FTTE_ERR_ARG", st.slice_map, 1, shape, zslice)
        for zoom in (0.0, -1.0, float("nan"), float("inf")):
            _expect("FTTE_ERR_ARG", st.slice_map, 1, shape, 0.5, (0.5, 0.5), zoom)
            _expect("FTTE_ERR_ARG", st.project_map, 1, shape, centre, zoom)
        for bad in ((0, 5), (5, 0), (-1, 5)):
            _expect("FTTE_ERR_ARG", st.slice_map, 1, bad, 0.5)
            _expect("FTTE_ERR_ARG", st.project_map, 1, bad)
        _expect("FTTE_ERR_ARG", st.project_map, 1, shape, centre, 1.0, 2)                                 # no such mode
        _expect("FTTE_ERR_ARG", st.project_map, 1, shape, (1.7, 0.5, 0.5), 2.0)                           # the window leaves the box
        _expect("FTTE_ERR_ARG", st.star_pdf, [0, g["level"].size])
        good = st.project_map(3, shape)                                                                   # and the context is still good
        assert np.isfinite(good).any()
        st.clumping(), st.gas_pdf(), st.star_pdf([1, 2])
        held = st.counter("device_objects")
        assert held > idle
        # another grid: the owner's buffers go, and nothing answers until a medium is set
        st.set_grid(int(u["n"]), u["level"], float(u["box"]))
        assert st.counter("device_objects") < held
        for call in (lambda: st.slice_map(1, shape, 0.5), lambda: st.project_map(1, shape), st.clumping, st.gas_pdf):
            _expect("FTTE_ERR_STATE", call)
        load(st, u)
        assert same_bits(st.project_map(3, (50, 37), centre, 2.0), u["job2_map"])
    with rt.StellarTransfer() as probe:
        assert probe.counter("device_objects") == idle                                                    # close() released everything


def test_multi_device_context_refuses(golden):
    """a multi-device context never holds a medium (set_medium is refused on it): FTTE_ERR_UNSUPPORTED"""
    g = golden("analysis_uniform16")
    with rt.StellarTransfer(devices=[0, 0]) as st:
        st.set_grid(int(g["n"]), g["level"], float(g["box"]))
        _expect("FTTE_ERR_UNSUPPORTED", st.slice_map, 1, (4, 4), 0.5)
        _expect("FTTE_ERR_UNSUPPORTED", st.project_map, 1, (4, 4))
        _expect("FTTE_ERR_UNSUPPORTED", st.clumping)
        _expect("FTTE_ERR_UNSUPPORTED", st.gas_pdf)
        _expect("FTTE_ERR_UNSUPPORTED", st.star_pdf, [0])


def test_fortran_host(stellar, golden, tmp_path):
    """fortran/ftte_demo_analysis on the refined golden: its clumping line and its raw maps equal the Python results"""
    exe = os.path.join(ROOT, "fortran", "ftte_demo_analysis")
    if not os.path.exists(exe):
        pytest.skip("fortran/ftte_demo_analysis not built (no Fortran compiler at build time)")
    g = golden("analysis_refined6")
    izone, shape, zslice, centre, zoom = 8, (50, 37), 0.6180339887498949, (0.5, 0.5, 0.5), 2.0
    case, out = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(case, "wb") as f:
        f.write(np.array([int(g["n"]), g["level"].size, izone, *shape], "<i4").tobytes())
        f.write(np.array([float(g["box"]), zslice, *centre, zoom], "<f8").tobytes())
        f.write(g["level"].astype("<i4").tobytes())
        for k in ("rho", "abun2", "HI"):
            f.write(g[k].astype("<f8").tobytes())
    res = subprocess.run([exe, str(case), str(out)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "ftte_demo_analysis OK" in res.stdout, res.stdout + res.stderr
    load(stellar, g)
    want = stellar.clumping()
    npix = shape[0] * shape[1]
    raw = open(out, "rb").read()
    maps = np.frombuffer(raw, "<f4", 2 * npix).reshape(2, shape[1], shape[0])
    sums = np.frombuffer(raw, "<f8", 3, 8 * npix)
    assert same_bits(maps[0].T, stellar.slice_map(izone, shape, zslice, centre[:2], zoom))
    assert same_bits(maps[1].T, stellar.project_map(izone, shape, centre, zoom))
    assert tuple(sums) == (want["clumping"], want["volume"], want["mean_nh"])
    line = [ln for ln in res.stdout.splitlines() if "clumping =" in ln]
    assert len(line) == 1
    printed = [float(v) for v in line[0].split("=")[1].split()]
    assert len(printed) == 2 and close(printed[0], want["clumping"], 1e-9) and printed[1] == want["volume"]
