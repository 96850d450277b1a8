"""The thermal balance on the host (no GPU): radiativetransfer_amd/csrc/ftte_thermal_math.h compiled by g++ -- under the sanitizers as
a program (tests/host/thermal_check.cpp), and as the small library of tests/_thermal.py against a numpy restatement of
thermalEquilibrium, against libm's logarithm, against the closed-form Compton limit and for stationarity -- and the host helper
ftte_cooling_coefficient_tables of libftte.so against a numpy restatement of calc_rates.f:414-544.  Parity with the compiled
reference is not established for this feature (calc_rates needs its two data files); these stand in for it."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _thermal as T

ROOT = T.ROOT
EPS = T.EPS
SYMBOLS = ["ftte_get_temperature", "ftte_set_cooling_coefficients", "ftte_thermal_equilibrium", "ftte_thermal_equilibrium_device",
           "ftte_advance_temperature", "ftte_advance_temperature_device"]


@pytest.fixture(scope="module")
def grid(golden):
    g = golden("chem_uvb_refined")
    return float(g["logtem0"]), float(g["logtem9"]), float(g["dlogtem"])


@pytest.fixture(scope="module")
def cases(golden, grid):
    out = {name: T.golden_case(golden(name), name, grid) for name in ("initial_refined", "chem_uniform_background", "chem_uvb_refined")}
    out["wide"] = T.wide_medium(grid)
    out["wide_uniform"] = T.wide_medium(grid, uniform=True)
    return out


def test_step_under_the_sanitizers(tmp_path):
    """tests/host/thermal_check.cpp's main(): the root property of the step or its documented clamp in every cell, steps below the
    cap, NaN inputs named -- with AddressSanitizer and UBSan"""
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "thermal_check")
    subprocess.check_call([gxx, *T.SANITIZE, "-I" + T.CSRC, T.SOURCE, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:])
    assert res.returncode == 0 and "thermal step under the sanitizers: ok" in res.stdout, res.stdout[-4000:] + res.stderr[-4000:]


@pytest.mark.parametrize("name", ["initial_refined", "chem_uniform_background", "chem_uvb_refined", "wide", "wide_uniform"])
def test_restatement_of_thermal_equilibrium(cases, name):
    """heating, cooling and hydroHeating of the header against the numpy restatement at the same logtem: |difference| <= 32 eps
    sum|terms| per cell (each term carries at most eight roundings; a sum of sixteen in another order adds at most 16 eps sum|terms|)"""
    case, tab = cases[name], T.tables()
    head = case["head"]
    ok = head[4] > 0
    logtem = np.where(ok, T.libm_log(np.where(ok, head[4], 1.0)), 0.0)
    got = T.equilibrium(*head, *T.rate_args(case, tab), logtem=logtem)
    assert got[3] == 0
    crate = None if case["rates"] is None else case["rates"][3:]
    want = T.equilibrium_numpy(*head[:5], logtem, *head[5:], crate, case["run_uvb"], case["J"], tab["gamma"], tab["uniform_gamma"], case["threshold"],
                               *case["grid"], tab["cool"], tab["comp1"], tab["comp2"])
    bound = 32 * EPS * want[3]
    for what, a, b in zip(("heating", "cooling", "hydroHeating"), got[:3], want[:3]):
        worst = np.max(np.abs(a - b) / np.where(bound > 0, bound, 1.0))
        print(f"{name} {what}: worst difference / bound {worst:.3f}")
        assert np.all(np.abs(a - b) <= bound), what
    assert np.any(got[2] > 0) or name == "chem_uvb_refined"
    assert np.any(got[0] > 0) and np.all(got[1] != 0)


def test_log_against_libm(grid):
    """ftte_log against the C library's log over 1e-3 .. 1e12, the table's ends and powers of two.  Measured when it was written:
    worst 2 ulp from libm's result; 3.2 % of the values differ from it at all, 191 of the million by 2 ulp.  All of those have
    0.64 < x < 1.53: there |k| = 1 and k ln2 and log m partly cancel (log 0.643 = log 1.286 - ln2), so the rounding of the two parts,
    at half an ulp of 0.69 each, is up to an ulp each of a result below 0.5.  Elsewhere the worst is 1 ulp."""
    x = np.concatenate([10 ** np.linspace(-3.0, 12.0, 1_000_000), np.exp([grid[0], grid[1]]), [1.0, float(np.float32(1.0e8))],
                        2.0 ** np.arange(-10, 41), np.nextafter(2.0 ** np.arange(-10, 41), 0), np.nextafter(2.0 ** np.arange(-10, 41), np.inf)])
    got, want = T.log(x), T.libm_log(x)
    ulp = np.abs(got - want) / np.spacing(np.abs(np.where(want == 0, 1.0, want)))
    ulp = np.where(want == 0, np.abs(got) / np.spacing(1.0), ulp)
    print(f"ftte_log vs libm: worst {ulp.max():.2f} ulp, {np.count_nonzero(ulp)} of {x.size} differ")
    assert T.log(np.array([1.0]))[0] == 0.0
    assert ulp.max() <= WORST_LOG_ULP


WORST_LOG_ULP = 2.0


def _species(rho, HI, HeI, HeII):
    nh, nhe = T.PSI * rho / T.MH, (1.0 - T.PSI) * rho / T.MHE
    heii, heiii = HeII.copy(), nhe - HeI - HeII
    heii[(heiii < 0) & (nhe - HeI < 0)] = 0.0
    heiii[heiii < 0] = 0.0
    return nh, nhe, (nh - HI) + heii + 2.0 * heiii


def compton_formula(case, tab, dt, sub, tmin=T.TMIN, tmax=T.TMAX):
    """backward Euler of edot = -comp1 (T - comp2) de in closed form, `sub` times"""
    n, level, box, rho, tgas, HI, HeI, HeII = case["head"]
    nh, nhe, de = _species(rho, HI, HeI, HeII)
    c = 1.3806503e-16 * (nh + nhe + de) / (float(np.float32(1.6667)) - 1.0)
    ah = tab["comp1"] * de / c * (dt / sub)
    T0 = np.minimum(np.maximum(tgas, tmin), tmax)
    Tn = T0.copy()
    for _ in range(sub):
        Tn = (Tn + ah * tab["comp2"]) / (1.0 + ah)
    return T0, Tn


@pytest.mark.parametrize("dt,sub", T.STEPS)
def test_compton_limit(cases, dt, sub):
    """all thirteen tables zero, no heating: T1 = (T0 + a h comp2)/(1 + a h), a = comp1 de / c, within 16 eps (T1 + T0 + comp2) (the
    computed F differs from the exact one by at most 8 eps of the sum of its three magnitudes, F' = 1 + a h >= 1, the bisection adds
    one ulp)"""
    case, tab = cases["wide"], dict(T.tables())
    tab["cool"] = np.zeros_like(tab["cool"])
    args = (None, False, None, None, np.zeros(3), 0.0, *case["grid"], tab["cool"], tab["comp1"], tab["comp2"])
    T1, lt, status, steps, change = T.advance(*case["head"], *args, dt, sub)
    assert status == 0
    T0, want = compton_formula(case, tab, dt, sub)
    err = np.abs(T1 - want) / (16 * EPS * (T1 + T0 + tab["comp2"]))
    print(f"Compton limit dt {dt:g} x{sub}: worst error / bound {err.max():.3f}")
    assert err.max() <= 1.0
    assert np.array_equal(lt, T.log(T1)) and np.array_equal(change, np.abs(T1 - T0) / T0)


@pytest.mark.parametrize("name", ["initial_refined", "chem_uniform_background", "wide_uniform"])
def test_stationarity(cases, name):
    """After thermalEquilibrium with a uniform background, an advance at the same rates with the stored hydroHeating leaves every cell
    with hydroHeating > 0 at exactly its temperature (the two evaluations of edot are the same statement: their sum is exactly 0),
    and every cell with hydroHeating == 0 and positive net heating ends strictly warmer."""
    case, tab = cases[name], T.tables()
    head, tmin = case["head"], 0.1       # (the wide medium's temperatures start at 10^-0.5: no clipping here)
    heating, cooling, hydro, status = T.equilibrium(*head, *T.rate_args(case, tab))
    assert status == 0 and np.any(hydro > 0)
    for dt, sub in T.STEPS:
        T1, lt, status, steps, change = T.advance(*head, *T.rate_args(case, tab), dt, sub, tmin=tmin, hydro=hydro)
        assert status == 0
        held = hydro > 0
        assert np.array_equal(T1[held], head[4][held]) and not steps[held].any()
        rising = (hydro == 0) & (heating - cooling > 0)
        print(f"{name} dt {dt:g} x{sub}: {held.sum()} cells held, {rising.sum()} heated")
        assert np.all(T1[rising] > head[4][rising])


# ---- ftte_cooling_coefficient_tables (host code of libftte.so; needs no device) -------------------------------------------

def cooling_numpy(nratec, temstart, temend, rtype, k, mellema=None, gnedin=None):
    """calc_rates.f:414-544 and :619 with the flags as compiled (:155); default-real literals widened from single precision"""
    w = lambda v: float(np.float32(v))      # noqa: E731
    exp = np.vectorize(math.exp, otypes=[np.float64])      # the C library's, as the library's host side takes it: the temperature nodes
    dlogtem = (math.log(temend) - math.log(temstart)) / w(nratec - 1)      # are then the same numbers on both sides
    t = exp(math.log(temstart) + np.arange(nratec).astype(np.float32).astype(np.float64) * dlogtem)
    lt = np.array([math.log10(v) for v in t])
    big = math.log(1.0e30)
    cut = lambda a: exp(-np.minimum(big, w(a) / t))      # noqa: E731
    soft = 1.0 + np.sqrt(t / 1.0e5)
    c = np.empty((13, nratec))
    c[0] = 7.5e-19 * cut(118348.) / soft                                                   # :423-428
    c[1] = 9.1e-27 * cut(13179.) * t ** w(-0.1687) / soft
    c[2] = 5.54e-17 * cut(473638.) * t ** w(-0.397) / soft
    c[3], c[4], c[6] = 2.18e-11 * k[0], 3.94e-11 * k[2], 8.72e-11 * k[4]                   # :451-453
    c[5] = 5.01e-27 * t ** w(-0.1687) / soft * cut(55338.)                                 # :446-447
    if rtype == 1:                                                                         # :467-469, :487-490
        c[7] = 8.70e-27 * np.sqrt(t) * (t / 1000.0) ** w(-0.2) / (1.0 + (t / 1.0e6) ** w(0.7))
        c[8] = 1.55e-26 * t ** w(0.3647)
        c[10] = 3.48e-26 * np.sqrt(t) * (t / 1000.0) ** w(-0.2) / (1.0 + (t / 1.0e6) ** w(0.7))
    else:                                                                                  # :470-483, :491-509
        def entry(x, v):
            j = np.clip(np.searchsorted(x, lt, side="left"), 1, x.size - 1)      # the first node that is not below log10 T
            val = 10.0 ** ((lt - x[j - 1]) / (x[j] - x[j - 1]) * (v[j] - v[j - 1]) + v[j - 1])
            return np.where((lt < x[0]) | (lt > x[-1]), 0.0, val)
        c[7] = entry(mellema[:, 0], mellema[:, 1])
        c[8] = entry(np.log10(gnedin[:, 0]), np.log10(gnedin[:, 1]))                       # :407-409
        c[10] = entry(np.log10(gnedin[:, 0]), np.log10(gnedin[:, 2]))
    c[9] = 1.24e-13 * t ** -1.5 * cut(470000.) * (1.0 + w(0.3) * cut(94000.))              # :513-515
    c[11] = 1.43e-27 * np.sqrt(t) * (w(1.1) + w(0.34) * exp(-(5.5 - lt) ** 2 / 3.0))    # :527-528
    tmp = float(np.float32(2.0) * np.float32(13.598)) * 1.60217646e-12 / (1.3806503e-16 * t)      # :543-544
    c[12] = w(7.5e-19) * exp(-0.75 * tmp / 2.0) / (1.0 + np.sqrt(t / 1.0e5))
    return c, 5.65e-36


def _synthetic_files():
    x = np.linspace(1.0, 7.0, 81)
    mellema = np.stack([x, -24.0 - 0.5 * (x - 1.0)], axis=1)                 # log10 T, log10 of the coefficient
    y = np.linspace(1.5, 7.5, 201)
    gnedin = np.stack([10 ** y, 10 ** (-25.0 - 0.3 * y), 10 ** (-24.5 - 0.4 * y)], axis=1)      # the values themselves
    return mellema, gnedin


@pytest.mark.parametrize("rtype", [1, 2])
def test_cooling_coefficient_tables(rtype):
    """against the numpy restatement: relative difference <= 8 eps (1 + x_max), x_max = log(dhuge) the largest argument the formulas
    pass to exp (an argument perturbed by one ulp moves exp by that many eps); case B on synthetic monotone arrays, with its zeros
    outside the arrays' temperatures"""
    import radiativetransfer_amd as rt
    nratec, temend = 5000, float(np.float32(1.0e8))
    mellema, gnedin = _synthetic_files() if rtype == 2 else (None, None)
    c, compa = rt.cooling_coefficient_tables(nratec, 1.0, temend, rtype, mellema, gnedin)
    k = rt.rate_coefficient_tables(nratec, 1.0, temend, rtype)[0]
    want, wcompa = cooling_numpy(nratec, 1.0, temend, rtype, k, mellema, gnedin)
    assert compa == wcompa == 5.65e-36
    bound = 8 * EPS * (1.0 + math.log(1.0e30))
    for r in range(13):
        rel = np.abs(c[r] - want[r]) / np.where(want[r] != 0, np.abs(want[r]), 1.0)
        print(f"case {'AB'[rtype - 1]} row {r}: worst relative difference / bound {rel.max() / bound:.3f}")
        assert np.all(rel <= bound), r
        assert np.array_equal(c[r] == 0, want[r] == 0)
    if rtype == 2:
        t = np.exp(np.linspace(0.0, math.log(temend), nratec))
        for r, lo, hi in ((7, 1.0, 7.0), (8, 1.5, 7.5), (10, 1.5, 7.5)):
            outside = (np.log10(t) < lo - 1e-6) | (np.log10(t) > hi + 1e-6)
            assert outside.any() and not c[r][outside].any() and np.all(c[r][~outside & (np.log10(t) > lo + 1e-6) & (np.log10(t) < hi - 1e-6)] > 0)


def test_cooling_coefficient_tables_refusals():
    from radiativetransfer_amd import _lib
    fn = _lib.load().ftte_cooling_coefficient_tables
    dp = C.POINTER(C.c_double)
    c, compa = np.empty((13, 8)), C.c_double()
    mellema, gnedin = _synthetic_files()
    cp, m, g = c.ctypes.data_as(dp), mellema.ctypes.data_as(dp), gnedin.ctypes.data_as(dp)
    status = lambda *a: _lib.STATUS[fn(*a)]      # noqa: E731
    assert status(8, 1.0, 1e8, 1, None, None, cp, C.byref(compa)) == "FTTE_OK"      # case A needs neither array
    assert status(8, 1.0, 1e8, 2, m, g, cp, C.byref(compa)) == "FTTE_OK"
    assert status(8, 1.0, 1e8, 2, None, g, cp, C.byref(compa)) == "FTTE_ERR_ARG"
    assert status(8, 1.0, 1e8, 2, m, None, cp, C.byref(compa)) == "FTTE_ERR_ARG"
    assert status(1, 1.0, 1e8, 1, None, None, cp, C.byref(compa)) == "FTTE_ERR_ARG"
    assert status(8, 0.0, 1e8, 1, None, None, cp, C.byref(compa)) == "FTTE_ERR_ARG"
    assert status(8, 10.0, 10.0, 1, None, None, cp, C.byref(compa)) == "FTTE_ERR_ARG"
    assert status(8, 1.0, 1e8, 3, None, None, cp, C.byref(compa)) == "FTTE_ERR_ARG"
    assert status(8, 1.0, 1e8, 1, None, None, None, C.byref(compa)) == "FTTE_ERR_ARG"
    assert status(8, 1.0, 1e8, 1, None, None, cp, None) == "FTTE_ERR_ARG"


# ---- the entry points exist everywhere a host reaches them (as tests/test_point_populations_abi.py) -------------------------

def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("name", SYMBOLS + ["ftte_cooling_coefficient_tables"])
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
    assert _lib.STATUS[lib.ftte_get_temperature(None, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_set_cooling_coefficients(None, 2, None, 0.0, 0.0)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_thermal_equilibrium(None, 0, None, None, None, 0.0, 0, None, None, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_advance_temperature(None, 1.0, 1, 1.0, 2.0, 0, 0, None, None, None, 0.0, 0, None)] == "FTTE_ERR_ARG"
