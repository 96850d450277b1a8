"""CPU-side checks of the product: the C-ABI library loads and exports exactly what include/ftte.h declares,
its host geometry reproduces the reference's vectors, and it fails loudly (never falls back) without a GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    import radiativetransfer_amd
    from radiativetransfer_amd import build
    build.build_library()  # hipcc cross-compiles without a GPU
    return radiativetransfer_amd


def header_functions():
    text = open(os.path.join(ROOT, "include", "ftte.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ftte_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(rt):
    from radiativetransfer_amd import _lib
    names = header_functions()
    assert len(names) >= 19
    # through the package's loader: a bare CDLL here would map the system HIP runtime ahead of torch's, and every later test
    # in this process that opens a device would find none
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name), f"libftte.so does not export {name}"
    # and the Python binding table covers exactly the header
    assert sorted(_lib.SIGNATURES) == names


def test_no_device_is_an_error_not_a_fallback(rt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(rt.FtteError) as e:
        rt.DiffuseTransfer()
    assert e.value.status == "FTTE_ERR_NO_DEVICE"


def test_product_never_references_the_oracle():
    """Neither the package, nor the Fortran host, nor the tools import, link or run anything under oracle/ (the tools may
    name tests/compare_with_reference.py, which does)."""
    for top in ("radiativetransfer_amd", "fortran", "tools", "include"):
        for base, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".cpp", ".h", ".hip", ".f90", ".sh")):
                    text = open(os.path.join(base, f), errors="ignore").read()
                    text = text.replace("oracle evaluated", "")
                    if top == "fortran":
                        # the compile-only drop-in check reads the reference's .mod files where the checker's build left them
                        text = text.replace("oracle/_ref", "")
                    assert "oracle" not in text and "make_golden" not in text, f"{top}/{f} refers to the checker"


def test_host_geometry_matches_reference_vectors(rt, golden):
    g = golden("rotate_indices")
    nx, ny, nz = map(int, g["extents"])
    for z in range(24):
        for i in range(3):
            for j in range(4):
                for k in range(5):
                    assert rt.rotate_indices(i + 1, j + 1, k + 1, nx, ny, nz, z + 1) == tuple(g["table"][z, i, j, k])
    for name in ("geometry_192dir_16layers", "geometry_12dir_256layers"):
        g = golden(name)
        n = int(g["n"])
        for d in range(len(g["phi_in"])):
            p, t, z = rt.fold_direction(g["phi_in"][d], g["theta_in"][d])
            assert (p, t, z) == (g["phi"][d], g["theta"][d], g["izone"][d])
            L = rt.layer_patterns(n, p, t)
            for i in range(n):
                r, P = g["layers"][d][i], L[i]
                assert (P.xz_active, P.yz_active, P.xy_top, P.xz_top, P.yz_top) == tuple(r["flags"])
                assert (P.xy_x0, P.xy_y0, P.xy_len) == tuple(r["xy"])
                if P.xz_active:
                    assert (P.xz_x0, P.xz_z0, P.xz_len) == tuple(r["xz"])
                if P.yz_active:
                    assert (P.yz_y0, P.yz_z0, P.yz_len) == tuple(r["yz"])


def test_healpix_directions_match_oracle(rt):
    for level in (1, 2, 3):
        a, b = rt.healpix_directions(level), O.healpix_directions(level)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_error_codes_where_the_reference_stops(rt):
    pi = O.lib().fo_pi()
    for args, status in (((0.5 * pi, 0.3), "FTTE_ERR_PHI"), ((0.0, 0.3), "FTTE_ERR_PHI"),
                         ((0.3, 0.0), "FTTE_ERR_THETA"), ((0.3, 2.0), "FTTE_ERR_THETA"),
                         ((0.25 * np.pi, np.arctan(np.sqrt(0.5))), None)):  # near-diagonal: must fold or tie
        try:
            rt.fold_direction(*args)
            assert status is None
        except rt.FtteError as e:
            assert status is None or e.status == status
    with pytest.raises(rt.FtteError) as e:
        rt.rotate_indices(1, 1, 1, 4, 4, 4, 25)
    assert e.value.status == "FTTE_ERR_IZONE"
    with pytest.raises(rt.FtteError) as e:
        rt.pix2ang_nest(2, 48)
    assert e.value.status == "FTTE_ERR_PIXEL"


def test_compute_cell_intensity_is_the_reference_formula(rt):
    assert rt.compute_cell_intensity(1.0, 2.0, 1.0) == 1.0 + (2.0 - 1.0) / np.log(2.0)
    assert rt.compute_cell_intensity(0.0, 1.0, 1.0) == 1.0
    assert rt.compute_cell_intensity(0.0, 3e-21, 0.0) == 0.0  # Iout underflowed: (Iin-0)/log(inf) = 0


def test_shard_bounds():
    from radiativetransfer_amd.distributed import shard_bounds
    for count in (0, 1, 7, 96, 768):
        for world in (1, 2, 3, 8):
            cover = []
            for r in range(world):
                lo, hi = shard_bounds(count, r, world)
                cover.extend(range(lo, hi))
                assert 0 <= hi - lo - count // world <= 1
            assert cover == list(range(count))


def test_point_source_host_pieces_match_reference_vectors(rt, golden):
    """rmax (equiSources.f90:296-309) and dustCrossSection (dustModule.f90:30-73) of the product's host side against
    what the reference's compiled code wrote (tests/golden/point16_homogeneous.npz)."""
    import math
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_point as M
    g = golden("point16_homogeneous")
    assert np.array_equal(rt.rmax(), g["rmax"])
    a_smc = M.synthetic_population()[0]
    f32 = lambda x: float(np.float32(x))  # noqa: E731  a default-real literal of the reference, widened
    nu1 = f32(13.598)
    ev_to_hz = 1.60217646e-12 / f32(6.6260693e-27)
    lower, upper = nu1, 10.0 * nu1
    for ie in range(1, 301, 13):
        frac = float(np.float32(ie - 1) / np.float32(299))
        freq = lower * math.exp(frac * (math.log(upper) - math.log(lower)))   # stellarBetaTable.f90:122
        lam = f32(2.99792458e10) / (freq * ev_to_hz) * f32(1.e8)
        assert rt.dust_cross_section(lam / f32(1.e4), a_smc) * f32(1.e-22) == g["outputSigma"][3][ie - 1]


def test_uvb_beta_table_of_the_product_matches_reference_vectors(rt, golden):
    """ftte_uvb_beta_table (host code of the product, row A9's table) against the reference's own uvbBetaTable output."""
    g = golden("uvb_beta_table")
    for a, beta, ksi, gamma in zip(g["alpha"], g["beta"], g["ksi"], g["gamma"]):
        b, k, h = rt.uvb_beta_table(a)
        # the library hands beta over as [species HI, HeI, HeII][group]; the reference's fields are (24, 25, 26) per group
        assert np.array_equal(b[0], beta[:, 0]) and np.array_equal(b[1], beta[:, 2]) and np.array_equal(b[2], beta[:, 1])
        assert np.array_equal(k, ksi) and np.array_equal(h, gamma)
    for a, ksi, gamma in zip(g["alpha"], g["uniform_ksi"], g["uniform_gamma"]):   # ftte_uniform_table vs uniformTable(alpha1, alpha2)
        k, h = rt.uniform_table(a[0], a[1])
        assert np.array_equal(k, ksi) and np.array_equal(h, gamma)


def test_coll_rates_of_the_product_match_reference_vectors(rt, golden):
    """ftte_coll_rates / ftte_rate_coefficient_tables (host code of the product) against the reference's own coll_rates."""
    g = golden("uvb_beta_table")
    for rtype in (1, 2):
        for T, ref in zip(g["coll_temperature"], g["coll_rates"][rtype - 1]):
            assert np.array_equal(rt.coll_rates(T, rtype), ref), (rtype, T)
    c = golden("chem_uvb_refined")
    k, l0, l9, dl = rt.rate_coefficient_tables()
    assert (l0, l9, dl) == (float(c["logtem0"]), float(c["logtem9"]), float(c["dlogtem"])) and np.array_equal(k, c["k"])
