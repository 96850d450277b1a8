"""The start-up ionisation equilibrium and computeMass (equiSources.f90:1008-1022, :3679-3868, :4369-4393) without a GPU: the
entry points are exported and check their context, and the numpy restatement of tests/_initial_equilibrium.py -- the
yardstick of the GPU tests -- reproduces the reference's own compiled routine (tests/golden/initial_*.npz,
make_golden_initial.py) bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _initial_equilibrium as R
from radiativetransfer_amd import _lib

GOLDENS = ["initial_refined", "initial_ingested"]


def test_entry_points_are_exported():
    lib = _lib.load()
    for name in ("ftte_initial_ionization_equilibrium", "ftte_hydrogen_mass"):
        assert hasattr(lib, name)


def test_null_context_is_an_argument_error():
    lib = _lib.load()
    uniform = (C.c_double * 3)(3e-14, 1e-16, 2e-14)
    frac, a, b = C.c_double(), C.c_double(), C.c_double()
    assert lib.ftte_initial_ionization_equilibrium(None, uniform, 0.0, 2, C.byref(frac)) == -1
    assert lib.ftte_initial_ionization_equilibrium(None, uniform, 0.0, 2, None) == -1
    assert lib.ftte_hydrogen_mass(None, C.byref(a), C.byref(b)) == -1


def _restate(g, tab, passes=2):
    return R.initial_equilibrium(g["rho"], g["tgas"], g["HI"], g["HeI"], g["HeII"], g["uniform"], float(g["threshold"]),
                                 float(tab["logtem0"]), float(tab["logtem9"]), float(tab["dlogtem"]), tab["k"], passes)


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_reference(golden, name):
    g, tab = golden(name), golden("chem_uvb_refined")
    HI, HeI, HeII, steps, ok = _restate(g, tab)
    assert ok.all()
    assert np.array_equal(HI, g["HI_out"]) and np.array_equal(HeI, g["HeI_out"]) and np.array_equal(HeII, g["HeII_out"])
    # to exact stagnation: some fifty to seventy residuals per cell and pass, not solveRateEquations' forty
    assert 40 < steps.mean() < 80 and steps.max() < 128
    # computeMass: every term is the reference's; added in cell-array order (the reference's tree walk) they give its sums exactly
    neutral, total = R.mass_terms(int(g["n"]), g["level"], float(g["box"]), HI, g["rho"])
    s_n = s_t = 0.0
    for a, b in zip(neutral, total):
        s_n += a
        s_t += b
    assert s_n == float(g["neutral_mass"]) and s_t == float(g["total_mass"])
    fn, ft = R.hydrogen_mass(int(g["n"]), g["level"], float(g["box"]), HI, g["rho"])
    assert abs(fn / float(g["neutral_mass"]) - 1) < 1e-13 and abs(ft / float(g["total_mass"]) - 1) < 1e-13


def test_golden_covers_the_branches(golden):
    """case (a) reaches every branch the issue lists: temperatures off both ends of the table, HI > nh, both HeIII clips,
    lit and self-shielded cells"""
    g, tab = golden("initial_refined"), golden("chem_uvb_refined")
    rho, HI, HeI, HeII = g["rho"], g["HI"], g["HeI"], g["HeII"]
    nh, nhe = R.PSI * rho / R.MH, (1 - R.PSI) * rho / R.MHE
    lt = R.logtem_of(g["tgas"])
    assert (lt < float(tab["logtem0"])).any() and (lt > float(tab["logtem9"])).any()
    assert (HI > nh).any()
    outer = nhe - HeI - HeII < 0
    assert (outer & (nhe - HeI < 0)).any() and (outer & ~(nhe - HeI < 0)).any()
    mfp = 1.0 / (np.fmin(HI, nh) * R.F32(6.3e-18) + HeI * R.F32(7.42e-18) + np.where(outer & (nhe - HeI < 0), 0.0, HeII) * R.F32(1.58e-18))
    lit = mfp >= float(g["threshold"])
    assert lit.any() and (~lit).any()


def test_passes_compose(golden):
    g, tab = golden("initial_refined"), golden("chem_uvb_refined")
    one = _restate(g, tab, 1)
    again = R.initial_equilibrium(g["rho"], g["tgas"], one[0], one[1], one[2], g["uniform"], float(g["threshold"]),
                                  float(tab["logtem0"]), float(tab["logtem9"]), float(tab["dlogtem"]), tab["k"], 1)
    two = _restate(g, tab, 2)
    assert all(np.array_equal(a, b) for a, b in zip(again[:3], two[:3]))
