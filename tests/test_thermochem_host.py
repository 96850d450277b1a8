"""The coupled step on the host (no GPU): radiativetransfer_amd/csrc/ftte_thermochem_math.h compiled by g++ -- under the sanitizers
as a program (tests/host/thermochem_check.cpp), and as the small library of tests/_thermochem.py against the two statements it is
made of (chem_advance_cell, thermal_advance_cell through tests/_chem_advance.py, tests/_thermal.py and tc_pair), on the front cells
it was written for, on a leaf in balance, at the cap, and for the photon budget.  Parity with the compiled reference is not
established for this feature (the reference has no time step): the host statement is the yardstick."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _chem_advance as A
import _thermal as T
import _thermochem as TC

ROOT = T.ROOT
EPS = T.EPS
SYMBOLS = ["ftte_advance_thermochemistry", "ftte_advance_thermochemistry_device", "ftte_get_subcycles"]


@pytest.fixture(scope="module")
def chem(golden):
    return golden("chem_uvb_refined")


@pytest.fixture(scope="module")
def grid(chem):
    return float(chem["logtem0"]), float(chem["logtem9"]), float(chem["dlogtem"])


@pytest.fixture(scope="module")
def cases(golden, grid):
    return {name: TC.case(golden, name, grid) for name in TC.NAMES}


def test_step_under_the_sanitizers(tmp_path):
    """tests/host/thermochem_check.cpp's main(): in every rate mode and schedule the fraction bounds, the clip and the cap in every leaf;
    the uniform schedule as a chain of pairs, with the root property of its last temperature step; NaN inputs and an empty cell
    named -- with AddressSanitizer and UBSan, as a stand-alone program"""
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "thermochem_check")
    subprocess.check_call([gxx, *TC.SANITIZE, "-I" + TC.CSRC, TC.SOURCE, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:])
    assert res.returncode == 0 and "coupled step under the sanitizers: ok" in res.stdout, res.stdout[-4000:] + res.stderr[-4000:]


def _chem_args(case, chem):
    n, level, box, rho, tgas, HI, HeI, HeII = case["head"]
    krate = None if case["rates"] is None else case["rates"][:3]
    return (n, level, box, rho, tgas, HI, HeI, HeII, krate, case["run_uvb"], case["J"], case["ksi"], case["uniform"], case["threshold"], *case["grid"],
            chem["k"])


@pytest.mark.parametrize("name", TC.NAMES)
def test_anchor_one_subcycle_is_the_pair(cases, chem, name):
    """Anchor A.  max_subcycles = 1: the species are chem_advance_cell(dt, 1)'s bit for bit in every rate mode.  With J and no point
    rates the heating per absorber does not depend on the state, and the temperature is thermal_advance_cell(dt, 1)'s on the new
    species bit for bit.  In the other modes (point rates over the absorbers, the self-shielding test) the pair forms the heating per
    absorber from the NEW species and the statement from the incoming ones: there the temperature may differ, and is not compared."""
    tab = T.tables()
    for case in TC.modes(cases[name]):
        for dt in (1e9, 1e13, 1e40):
            got = TC.advance(case, tab, chem, dt, 0.1, 1)
            want = A.advance(*_chem_args(case, chem), dt, 1)
            assert got["status"] == 0 and want[3] == 0
            assert all(np.array_equal(got[s], w) for s, w in zip(("HI", "HeI", "HeII"), want[:3])), (name, dt)
            assert np.array_equal(got["change"], want[5]) and np.all(got["subcycles"] == 1)
            if case["run_uvb"] and case["rates"] is None:
                th = T.advance(*case["head"][:5], *want[:3], *T.rate_args(case, tab), dt, 1)
                assert th[2] == 0
                assert np.array_equal(got["T"], th[0]) and np.array_equal(got["logtem"], th[1]) and np.array_equal(got["tchange"], th[4])
                assert np.array_equal(got["steps"], want[4] + th[3])


@pytest.mark.parametrize("N", [3, 16])
@pytest.mark.parametrize("name", ["chem_uvb_refined", "wide"])
def test_anchor_uniform_schedule_is_a_chain_of_pairs(cases, chem, name, N):
    """Anchor B.  eta = 0, max_subcycles = N, J and no point rates: N successive pairs of host calls over the h-sequence of the
    statement (computed here in its arithmetic), the first chemistry at the stored logarithm and the later ones at ftte_log(T): species
    and temperature bit for bit"""
    tab, case, dt = T.tables(), TC.without_rates(cases[name]), 1e13
    got = TC.advance(case, tab, chem, dt, 0.0, N)
    assert got["status"] == 0 and np.all(got["subcycles"] == N) and np.all(got["capped"] == 1)
    hs = TC.schedule(dt, 0.0, N)
    assert len(hs) == N
    tgas, HI, HeI, HeII = case["head"][4:]
    logtem = None
    for h in hs:
        HI, HeI, HeII, tgas, logtem, status = TC.pair(case, tab, chem, h, logtem=logtem, state=(tgas, HI, HeI, HeII))
        assert status == 0
    for what, a, b in zip(("HI", "HeI", "HeII", "T", "logtem"), (HI, HeI, HeII, tgas, logtem), (got[s] for s in ("HI", "HeI", "HeII", "T", "logtem"))):
        assert np.array_equal(a, b), what


# ---- the front cells -----------------------------------------------------------------------------------------------------------
# Four cells, n_H = 1e-4 .. 1e-1 cm^-3, 100 K, neutral, lit at Gamma24 ~ 1e-12 /s.  The yardstick is the header's own uniform schedule,
# eta = 0 in 4096 subcycles.  Measured on the host when this was written (errors against the yardstick: |dT|/T, |d log10(HI/n_H)|):
#
#   dt = 1e13 s              n_H = 1e-4          1e-3          1e-2          1e-1
#   the pair                 0.297, 3.54     0.300, 2.88     0.247, 2.02     0.0335, 1.29
#   eta = 0.5  (21 subc.)    0.0343, 1.51    0.0420, 0.869   0.0526, 0.225   0.00473, 0.0236
#   eta = 0.1  (74)          0.00881, 0.562  0.0109, 0.185   0.0143, 0.0319  0.000444, 0.000485
#   eta = 0.02 (277)         0.00164, 0.128  0.00210, 0.0288 0.00292, 0.00500 6.5e-6, 0.000316
#   dt = 1e14 s
#   the pair                 0.225, 3.03     0.223, 2.26     0.153, 1.72     0.0445, 1.22
#   eta = 0.5  (22)          0.0294, 0.0153  0.0350, 0.0231  0.00319, 0.00625 0.000524, 0.00339
#   eta = 0.1  (74)          0.00598, 0.00304 0.00748, 0.00517 0.00191, 0.00527 8.8e-5, 0.000458
#   eta = 0.02 (275)         0.000696, 0.000489 0.000863, 0.000754 0.00114, 0.00385 2.9e-5, 0.000118
#
# The pair against eta = 0.1: the smallest factor is 6.31 (log10 HI/n_H at n_H = 1e-4, dt = 1e13 s), in T 17.3; FACTOR is half of it.
# The figures are those of THERMOCHEM_FLOOR = 0.2.  The floor was retuned from the prototype's 0.1 on these measurements: with 0.1 the
# smallest factor is 8.16 but the errors are not monotonic in eta in three of the eight (dt, cell) cases below (cells that end the step
# close to their equilibrium, e.g. dt = 1e14 s, n_H = 1e-2: the error in T went 0.00109, 0.00280, 0.00120); DESIGN.md has the scan.
FRONT_NH = (1e-4, 1e-3, 1e-2, 1e-1)
FRONT_DT = (1e13, 1e14)
FACTOR = 3.15

_front = {}


def _front_errors(chem, grid, dt):
    """per eta (and "pair"): (|dT|/T, |d log10 HI/n_H|) of the four cells against the yardstick; computed once per dt"""
    if dt not in _front:
        tab, case = T.tables(), TC.front_case(grid, chem["ksi"], FRONT_NH)
        ref = TC.advance(case, tab, chem, dt, 0.0, 4096)
        assert ref["status"] == 0 and np.all(ref["subcycles"] == 4096)

        def err(HI, temp):
            return np.abs(temp - ref["T"]) / ref["T"], np.abs(np.log10(HI / ref["HI"]))
        out = {"pair": err(*TC.existing_pair(case, tab, chem, dt))}
        for eta in (0.5, 0.1, 0.02):
            r = TC.advance(case, tab, chem, dt, eta, 4096)
            assert r["status"] == 0      # (the even split of 4096 decides the first subcycles of a 100 K cell: T / |dT/dt| is short there)
            out[eta] = err(r["HI"], r["T"])
            out[eta, "subcycles"] = r["subcycles"]
        _front[dt] = out
    return _front[dt]


@pytest.mark.parametrize("dt", FRONT_DT)
def test_front_cell_against_the_pair(chem, grid, dt):
    """at eta = 0.1 the error is smaller than the existing pair's by FACTOR wherever the pair is off by more than 1 % in T or 0.1 dex in
    HI/n_H -- which it is in all four cells, in both.  (This fails on the code before the coupled step: there is no such call.)"""
    e = _front_errors(chem, grid, dt)
    (pT, pX), (aT, aX) = e["pair"], e[0.1]
    print(f"dt {dt:g}: the pair off by T {pT}, dex {pX}; eta = 0.1 by T {aT}, dex {aX}; factors T {pT / aT}, dex {pX / aX}; subcycles {e[0.1, 'subcycles']}")
    assert np.all(pT[:3] > 0.01) and np.all(pX[:3] > 0.1)      # the table's first three columns, at the least
    assert np.all(aT[pT > 0.01] * FACTOR <= pT[pT > 0.01])
    assert np.all(aX[pX > 0.1] * FACTOR <= pX[pX > 0.1])
    assert e[0.1, "subcycles"].max() < 4096 // 8


@pytest.mark.parametrize("cell", range(4))
@pytest.mark.parametrize("dt", FRONT_DT)
def test_front_cell_errors_do_not_increase_as_eta_falls(chem, grid, dt, cell):
    """The errors in T and in log10(HI/n_H) at eta = 0.5, 0.1, 0.02 against the yardstick do not increase as eta falls, in each of
    the four cells.  The thinnest step is dt = 1e14 s, n_H = 1e-2, log10(HI/n_H): 0.00625, 0.00527, 0.00385 (a cell that ends the step
    close to its equilibrium, where the error is a small difference of contributions of either sign); in the cells the front crosses
    late in the step the errors fall by a factor of four to eight per step of eta."""
    e = _front_errors(chem, grid, dt)
    for what, i in (("T", 0), ("log10 HI/n_H", 1)):
        seq = [e[eta][i][cell] for eta in (0.5, 0.1, 0.02)]
        print(f"dt {dt:g} n_H {FRONT_NH[cell]:g} {what}: {seq}")
        assert seq[0] >= seq[1] >= seq[2], (what, seq)


# ---- a leaf in balance, the cap, the photon budget ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["initial_refined", "chem_uniform_background", "wide_uniform"])
def test_leaf_in_balance(cases, chem, name):
    """A state the pair leaves unchanged: the chemistry step over dt repeated until it returns its input bit for bit (in the leaves
    where it does), thermalEquilibrium there and its hydroHeating added -- as the stationarity test of tests/test_thermal_host.py.  The
    coupled call takes one subcycle in every such leaf and leaves species and temperature exactly where they are."""
    tab, case, dt = T.tables(), TC.without_rates(cases[name]), 1e17
    n, level, box, rho, tgas = case["head"][:5]
    state = case["head"][5:]
    for _ in range(40):
        got = A.advance(n, level, box, rho, tgas, *state, *_chem_args(case, chem)[8:], dt, 1)
        assert got[3] == 0
        fixed = (got[0] == state[0]) & (got[1] == state[1]) & (got[2] == state[2])
        state = got[:3]
    case = dict(case, head=(n, level, box, rho, tgas, *state))
    heating, cooling, hydro, status = T.equilibrium(*case["head"], *T.rate_args(case, tab))
    assert status == 0
    th = T.advance(*case["head"], *T.rate_args(case, tab), dt, 1, tmin=0.1, hydro=hydro)
    held = fixed & (th[0] == tgas)
    print(f"{name}: {held.sum()} of {held.size} leaves in balance")
    assert held.sum() > held.size // 4
    got = TC.advance(case, tab, chem, dt, 0.1, 64, tmin=0.1, hydro=hydro)
    assert got["status"] == 0
    assert np.all(got["subcycles"][held] == 1) and not got["capped"][held].any()
    for s, want in zip(("HI", "HeI", "HeII", "T"), (*state, tgas)):
        assert np.array_equal(got[s][held], want[held]), s
    assert not got["tchange"][held].any() and not got["change"][held].any()


def test_cap(cases, chem):
    """eta = 1e-6, max_subcycles = 8 on the wide medium: every leaf ends in at most 8 subcycles with `remaining` at exactly 0 (a leaf
    that ends with time left fails, and none does; the schedule's arithmetic itself: _thermochem.schedule), and the flag is set in
    every leaf that took 8.  Where eta tau never reached the even split the leaf took the uniform schedule: the bits of eta = 0."""
    tab, case = T.tables(), cases["wide"]
    got = TC.advance(case, tab, chem, 1e13, 1e-6, 8)
    assert got["status"] == 0
    sub, cap = got["subcycles"], got["capped"]
    print(f"subcycles: {np.bincount(sub)}")
    assert sub.min() >= 1 and sub.max() == 8
    assert np.all(cap[sub == 8] == 1)
    # a leaf whose own step eta * tau never reached the even split took the uniform schedule: the same bits as eta = 0
    uni = TC.advance(case, tab, chem, 1e13, 0.0, 8)
    same = np.ones(sub.size, bool)
    for s in ("HI", "HeI", "HeII", "T"):
        same &= got[s] == uni[s]
    print(f"{same.sum()} of {sub.size} leaves took the uniform schedule")
    assert same.sum() > sub.size // 2 and np.all(sub[same] == 8)
    for dt in (1e13, 1e9, 3.3e11):
        assert len(TC.schedule(dt, 0.0, 8)) == 8 and len(TC.schedule(dt, dt / 1e4, 8)) == 8      # (both end: remaining got to 0.0)


def test_photon_budget(cases, chem):
    """Point sources alone (no background), no collisional ionisation (k1 = 0): the rate per absorber G = krate24 / (vol HI0) is fixed
    at entry, each subcycle gives HI' >= HI / (1 + h G), so HI_end >= HI0 / prod(1 + h_s G) >= HI0 exp(-G dt) >= HI0 (1 - G dt): a leaf
    loses no more neutral atoms than ionising photons were absorbed in it, vol (HI0 - HI') <= dt krate24, with HI0 the clipped
    incoming HI.  Rounding: each subcycle's HI' carries a few roundings, allowed for as 8 eps HI0 per subcycle."""
    tab = T.tables()
    case = dict(cases["wide_uniform"])
    case["uniform"], case["threshold"] = np.zeros(3), 0.0
    k = np.array(chem["k"], dtype=np.float64)
    k[0] = 0.0
    n, level, box, rho, tgas, HI = case["head"][:6]
    vol = (box / n) ** 3
    HI0 = np.minimum(HI, T.PSI * rho / T.MH)
    for dt, eta, cap in ((1e9, 0.1, 64), (1e11, 0.1, 64), (1e13, 0.0, 16)):
        got = TC.advance(case, tab, dict(k=k), dt, eta, cap)
        assert got["status"] == 0
        lost, paid = vol * (HI0 - got["HI"]), dt * case["rates"][0]
        slack = 8 * EPS * got["subcycles"] * vol * HI0
        assert np.all(lost <= paid * (1 + 8 * EPS) + slack)
        assert np.any(lost > 0.5 * paid) and np.all(got["HI"] >= 0)


def test_failures_are_named(cases, chem):
    """a NaN temperature, a NaN density and an empty cell: the first of them is named"""
    tab, case = T.tables(), cases["chem_uvb_refined"]
    n, level, box, rho, tgas, HI, HeI, HeII = case["head"]
    logtem = T.libm_log(tgas)
    for where, change in ((7, "tgas"), (11, "rho"), (13, "empty")):
        r2, t2 = rho.copy(), tgas.copy()
        if change == "tgas":
            t2[where] = np.nan
        else:
            r2[where] = np.nan if change == "rho" else 0.0
        bad = dict(case, head=(n, level, box, r2, t2, HI, HeI, HeII))
        got = TC.advance(bad, tab, chem, 1e13, 0.1, 16, logtem=logtem)
        assert got["status"] == where + 1, change
        assert np.all((got["subcycles"] >= 0) & (got["subcycles"] <= 16))


# ---- the entry points exist everywhere a host reaches them (as tests/test_thermal_host.py) ------------------------------------------

def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_named_where_hosts_look(name):
    lib = C.CDLL(os.path.join(ROOT, "radiativetransfer_amd", "libftte.so"))
    assert getattr(lib, name) is not None
    assert re.search(r"^\s*%s;" % name, _read("radiativetransfer_amd", "csrc", "ftte.map"), re.M)
    assert re.search(r"^int %s\(" % name, _read("include", "ftte.h"), re.M)
    assert "bind(C, name='%s')" % name in _read("fortran", "ftte_binding.f90")
    from radiativetransfer_amd import _lib
    assert name in _lib.SIGNATURES


def test_null_context_is_an_argument_error():
    from radiativetransfer_amd import _lib
    lib = _lib.load()
    for fn in (lib.ftte_advance_thermochemistry, lib.ftte_advance_thermochemistry_device):
        assert _lib.STATUS[fn(None, 1.0, 0.1, 8, 1.0, 2.0, 0, 0, None, None, None, None, None, 0.0, 0, None, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_get_subcycles(None, None)] == "FTTE_ERR_ARG"
