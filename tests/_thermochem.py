"""The coupled step (radiativetransfer_amd/csrc/ftte_thermochem_math.h) for the tests: the header itself, compiled by g++ from
tests/host/thermochem_check.cpp into a small shared library (no sanitizers) and looped over the cells -- the host evaluation the GPU
tests compare with bit for bit -- beside the existing pair at a given logarithm (pair()), and the inputs the CPU and the GPU tests
share.  Parity with the compiled reference is not established for this feature (the reference has no time step): the host statement
is the yardstick, as for the thermal step."""
from __future__ import annotations

import ctypes as C

import numpy as np

import _thermal as T
from _hostlib import HostLib, dp as _dp, f64 as _f64

CSRC, FLAGS, SANITIZE = T.CSRC, T.FLAGS, T.SANITIZE
TMIN, TMAX = T.TMIN, T.TMAX

# (dt, eta, max_subcycles) of the bitwise GPU tests
RUNS = [(1e9, 0.1, 64), (1e13, 0.1, 64), (1e13, 0.0, 3), (1e40, 0.5, 8)]


def _declare(L):
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
    head = [C.c_longlong, C.c_int, ip, C.c_double, dp, dp, dp, dp, dp, dp, dp, C.c_int, dp, dp, dp, dp, dp, C.c_double, C.c_int, C.c_double,
            C.c_double, C.c_double, dp, dp, C.c_double, C.c_double]
    L.tc_advance.argtypes = head + [dp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, dp, dp, dp, dp, dp, lp, ip, ip, dp, dp]
    L.tc_pair.argtypes = head + [C.c_double, C.c_double, C.c_double, dp, dp, dp, dp, dp]
    L.tc_advance.restype = L.tc_pair.restype = C.c_longlong


lib = HostLib("thermochem", "thermochem_check.cpp", ("ftte_thermochem_math.h", "ftte_thermal_math.h", "ftte_chem_math.h", "ftte_math.h"),
              "the coupled step", _declare, local=("fit_tables.h",))
SOURCE = lib.source


def _head(case, tab, chem, logtem=None, state=None):
    """the arguments tc_advance and tc_pair share, from a case of _thermal.golden_case / wide_medium (rates [6][ncell] or None), the
    tables of _thermal.tables() and the golden chem_uvb_refined (k; the case brings its ksi and uniform: cases()); state: (tgas, HI, HeI, HeII) in place of the case's"""
    n, level, box, rho, tgas, HI, HeI, HeII = case["head"]
    if state is not None:
        tgas, HI, HeI, HeII = state
    level = np.ascontiguousarray(level, dtype=np.int32)
    f = [_f64(a) for a in (rho, tgas, T.libm_log(tgas) if logtem is None else logtem, HI, HeI, HeII)]
    nc = f[0].size
    opt = [None if a is None else _f64(a) for a in (case["rates"], case["J"], case["ksi"], tab["gamma"], case["uniform"], tab["uniform_gamma"])]
    if opt[0] is not None:
        assert opt[0].shape == (6, nc)
    if case["run_uvb"]:
        assert opt[1].shape == (3, nc)
    k, cool = _f64(chem["k"]), _f64(tab["cool"])
    assert k.shape[0] == 6 and cool.shape[0] == 13 and k.shape[1] == cool.shape[1]
    args = [nc, int(n), level.ctypes.data_as(C.POINTER(C.c_int32)), float(box), *[_dp(a) for a in f], _dp(opt[0]), int(bool(case["run_uvb"])),
            *[_dp(a) for a in opt[1:]], float(case["threshold"]), k.shape[1], *[float(x) for x in case["grid"]], _dp(k), _dp(cool), float(tab["comp1"]),
            float(tab["comp2"])]
    return nc, args, [level, f, opt, k, cool]


def advance(case, tab, chem, dt, eta, max_subcycles, tmin=TMIN, tmax=TMAX, hydro=None, logtem=None, state=None):
    """thermochem_advance_cell over the cells of a case, from the stored logarithm `logtem` (default: the C library's log of tgas, as
    ftte_set_temperature takes it) -> dict of HI, HeI, HeII, T, logtem, status (0, or 1 + the first failing cell), steps, subcycles,
    capped, change, tchange (per cell)"""
    nc, args, keep = _head(case, tab, chem, logtem, state)
    hydro = None if hydro is None else _f64(hydro)
    out = [np.empty(nc) for _ in range(5)]
    steps, sub, cap = np.zeros(nc, dtype=np.int64), np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.int32)
    change, tchange = np.empty(nc), np.empty(nc)
    ip = C.POINTER(C.c_int32)
    status = lib().tc_advance(*args, _dp(hydro), float(dt), float(eta), int(max_subcycles), float(tmin), float(tmax), *[_dp(a) for a in out],
                              steps.ctypes.data_as(C.POINTER(C.c_longlong)), sub.ctypes.data_as(ip), cap.ctypes.data_as(ip), _dp(change), _dp(tchange))
    return dict(HI=out[0], HeI=out[1], HeII=out[2], T=out[3], logtem=out[4], status=int(status), steps=steps, subcycles=sub, capped=cap, change=change,
                tchange=tchange)


def pair(case, tab, chem, h, tmin=TMIN, tmax=TMAX, logtem=None, state=None):
    """the existing pair over h: chem_advance_cell(h, 1) at `logtem`, then thermal_advance_cell(h, 1) on the new species
    -> HI, HeI, HeII, T, ftte_log(T), status"""
    nc, args, keep = _head(case, tab, chem, logtem, state)
    out = [np.empty(nc) for _ in range(5)]
    status = lib().tc_pair(*args, float(h), float(tmin), float(tmax), *[_dp(a) for a in out])
    return (*out, int(status))


def schedule(dt, eta_tau, max_subcycles):
    """the subcycle lengths of the statement for a constant eta * tau (0: the uniform schedule), in its arithmetic"""
    out, remaining, s = [], float(dt), 0
    while remaining > 0.0:
        h = min(remaining, max(eta_tau, remaining / float(max_subcycles - s)))
        out.append(h)
        remaining = 0.0 if h >= remaining else remaining - h
        s += 1
    return out


# ---- the cases: those of tests/test_thermal_host.py with the chemistry's half of the rates ------------------------------------------

NAMES = ("initial_refined", "chem_uniform_background", "chem_uvb_refined", "wide", "wide_uniform")


def case(golden, name, grid):
    """a case of _thermal.golden_case / wide_medium with ksi[3][3] or uniform[3] (the ionisation integrals) beside it and, where it has
    point-source rates, krate24..26 in rows 0..2 of them: the golden's own for chem_uvb_refined, synthetic ones in the lit cells of
    the wide media"""
    chem = golden("chem_uvb_refined")
    if name.startswith("wide"):
        out = T.wide_medium(grid, uniform=name == "wide_uniform")
        rho = out["head"][3]
        rng = np.random.default_rng(23)
        vol = (out["head"][2] / out["head"][0]) ** 3
        lit = out["rates"][3] > 0
        for r in range(3):
            out["rates"][r] = np.where(lit, 10 ** rng.uniform(-16, -11, rho.size) * vol * T.PSI * rho / T.MH, 0.0)
        out["uniform"] = None if out["run_uvb"] else golden("initial_refined")["uniform"]
    else:
        g = golden(name)
        out = T.golden_case(g, name, grid)
        if out["rates"] is not None:
            out["rates"][:3] = g["krate"]
        out["uniform"] = None if out["run_uvb"] else g["uniform"]
    out["ksi"] = chem["ksi"] if out["run_uvb"] else None
    return out


def without_rates(c):
    out = dict(c)
    out["rates"] = None
    return out


def modes(c):
    """the case in every rate mode it has: as it is and, where it has point-source rates, without them"""
    return [c] if c["rates"] is None else [c, without_rates(c)]


# ---- the front cells of the issue: four densities, 100 K, neutral, lit at Gamma24 ~ 1e-12 /s -------------------------------------

def front_case(grid, ksi, nh=(1e-4, 1e-3, 1e-2, 1e-1)):
    nh = np.asarray(nh, dtype=np.float64)
    rho = nh * T.MH / T.PSI
    nc = rho.size
    nh_, nhe = T.PSI * rho / T.MH, (1.0 - T.PSI) * rho / T.MHE
    J = np.array([3.8e-22, 1.5e-22, 0.5e-22])[:, None] * np.ones((1, nc))
    head = (nc, np.zeros(nc, np.int32), 2.5e23, rho, np.full(nc, 100.0), nh_.copy(), nhe.copy(), np.zeros(nc))
    return dict(head=head, rates=None, run_uvb=True, J=J, threshold=0.0, grid=grid, uniform=None, ksi=ksi)


def existing_pair(case, tab, chem, dt, substeps=1):
    """what evolve does today: chemistry over dt at the stored logarithm, then the temperature over dt on the new species, through the
    two test libraries -> HI, T"""
    import _chem_advance as A
    n, level, box, rho, tgas, HI, HeI, HeII = case["head"]
    got = A.advance(n, level, box, rho, tgas, HI, HeI, HeII, None, True, case["J"], case["ksi"], None, 0.0, *case["grid"], chem["k"], dt, substeps)
    assert got[3] == 0
    th = T.advance(n, level, box, rho, tgas, got[0], got[1], got[2], *T.rate_args(case, tab), dt, substeps)
    assert th[2] == 0
    return got[0], th[0]
