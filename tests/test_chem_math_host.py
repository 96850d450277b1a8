"""The per-cell chemistry of the kernels (csrc/ftte_chem_math.h) evaluated on the host, without a GPU: the oracle library compiles
the same header with gcc and loops it over the cells (fo_device_solve_rate_equations, fo_device_initial_equilibrium,
fo_device_chem_tame), and the result is held against the two independent statements of the chemistry -- oracle/ftte_oracle_chem.c
and tests/_initial_equilibrium.py -- and against the vectors of the reference's own compiled code, bit for bit.

What this covers: on the host FTTE_DIV is `/` and FTTE_ANY is per element, so the header's control flow, operation order,
constants and branch logic (the clips, the self-shielding test, the interpolation, the four parameters of the one bisection, the
closing step and its test of the fractions, the `tame` predicate itself) are pinned here.  What it does not: the trimmed
division behind `tame` and the wavefront vote exist only on the device, and stay pinned by the bitwise GPU tests
(test_chem_gpu.py, test_initial_equilibrium_gpu.py), as do the kernels' loads, stores and the fold of their statistics."""
import numpy as np
import pytest

import _initial_equilibrium as R
import _oracle as O

PSI, MP, MN = R.PSI, R.MP, R.MN
BOX = 2.5e23
N = 16
NC = N ** 3


def _table(g):
    return float(g["logtem0"]), float(g["logtem9"]), float(g["dlogtem"]), g["k"]


def _chem_args(g, tab, uvb):
    """a chem_* golden as the argument list of O.solve_rate_equations (test_oracle_chem_golden.py: _run)"""
    return (int(g["n"]), g["level"], float(g["box"]), g["rho"], g["tgas"], g["HI"], g["HeI"], g["HeII"],
            g["krate"] if "krate" in g.files else None, uvb, g["J"] if "J" in g.files else None, g["ksi"] if "ksi" in g.files else None,
            g["uniform"] if "uniform" in g.files else None, float(g["threshold"]) if "threshold" in g.files else 0.0, *_table(tab))


def _same(mine, ref):
    """species, stopping cell and (where the oracle got through: it reports no steps when it stops) the steps"""
    return all(np.array_equal(a, b) for a, b in zip(mine[:3], ref[:3])) and mine[3] == ref[3] and (ref[3] != 0 or mine[4] == ref[4])


def _share(name, tame):
    print(f"{name}: {tame.sum()} of {tame.size} cells tame ({100.0 * tame.mean():.1f} %)")


@pytest.mark.parametrize("name,uvb", [("chem_uvb_refined", True), ("chem_uniform_background", False)])
def test_update_reproduces_the_reference(golden, name, uvb):
    g, tab = golden(name), golden("chem_uvb_refined")
    args = _chem_args(g, tab, uvb)
    HI, HeI, HeII, status, steps = O.device_solve_rate_equations(*args)
    assert status == 0
    assert np.array_equal(HI, g["HI_out"]) and np.array_equal(HeI, g["HeI_out"]) and np.array_equal(HeII, g["HeII_out"])
    assert steps == O.solve_rate_equations(*args)[4]
    tame = O.device_chem_tame(*args)
    _share(name, tame)
    assert tame.any()


@pytest.mark.parametrize("name", ["initial_refined", "initial_ingested"])
def test_start_up_reproduces_the_reference(golden, name):
    g, tab = golden(name), golden("chem_uvb_refined")
    args = (g["rho"], g["tgas"], g["HI"], g["HeI"], g["HeII"], g["uniform"], float(g["threshold"]), *_table(tab))
    HI, HeI, HeII, status, steps = O.device_initial_equilibrium(*args, passes=2)
    assert status == 0
    assert np.array_equal(HI, g["HI_out"]) and np.array_equal(HeI, g["HeI_out"]) and np.array_equal(HeII, g["HeII_out"])
    assert steps == int(R.initial_equilibrium(*args, passes=2)[3].sum())


def test_start_up_passes_compose(golden):
    g, tab = golden("initial_refined"), golden("chem_uvb_refined")
    rest = (g["uniform"], float(g["threshold"]), *_table(tab))
    one = O.device_initial_equilibrium(g["rho"], g["tgas"], g["HI"], g["HeI"], g["HeII"], *rest, passes=1)
    again = O.device_initial_equilibrium(g["rho"], g["tgas"], *one[:3], *rest, passes=1)
    two = O.device_initial_equilibrium(g["rho"], g["tgas"], g["HI"], g["HeI"], g["HeII"], *rest, passes=2)
    assert one[3] == again[3] == two[3] == 0
    assert all(np.array_equal(a, b) for a, b in zip(again[:3], two[:3])) and one[4] + again[4] == two[4]


def _wide_field(rho_range, j_range, seed):
    """the field of test_chem_gpu.py::test_equilibrium_over_wide_ranges_bitwise at 16^3: the same ranges, the same draws in the
    same order"""
    vol = (BOX / N) ** 3
    rng = np.random.default_rng(seed)
    rho = 10 ** rng.uniform(*rho_range, NC)
    nh, nhe = PSI * rho / MP, (1 - PSI) * rho / (2 * (MP + MN))
    tgas = 10 ** rng.uniform(1.0, 9.5, NC)
    J = 10 ** rng.uniform(*j_range, (3, NC))
    start = (nh * 10 ** rng.uniform(-8, 0, NC), nhe * 10 ** rng.uniform(-8, -0.5, NC), nhe * 10 ** rng.uniform(-8, -0.5, NC))
    krate = np.zeros((6, NC))
    lit = rng.random(NC) < 0.3
    krate[0] = np.where(lit, 10 ** rng.uniform(-16, -11, NC) * vol * start[0], 0.0)
    krate[1] = np.where(lit, 10 ** rng.uniform(-17, -12, NC) * vol * start[2], 0.0)
    krate[2] = np.where(lit, 10 ** rng.uniform(-16, -11, NC) * vol * start[1], 0.0)
    return rho, tgas, J, start, krate


def test_update_over_wide_ranges(golden):
    """densities over five decades, temperatures over the rate table's whole span, mean intensities over three decades, with and
    without point-source rates: species and steps equal the oracle's; over ten decades of density: the same first stopping cell"""
    g = golden("chem_uvb_refined")
    level = np.zeros(NC, np.int32)
    rho, tgas, J, start, krate = _wide_field((-27.5, -22.5), (-24.0, -21.0), seed=17)
    for rates in (None, krate[:3]):
        args = (N, level, BOX, rho, tgas, *start, rates, True, J, g["ksi"], None, 0.0, *_table(g))
        ref = O.solve_rate_equations(*args)
        assert ref[3] == 0
        assert _same(O.device_solve_rate_equations(*args), ref)
        _share("five decades, " + ("no point rates" if rates is None else "point rates"), O.device_chem_tame(*args))
    rho, tgas, J, start, krate = _wide_field((-31.0, -21.0), (-27.0, -19.0), seed=17)
    args = (N, level, BOX, rho, tgas, *start, None, True, J, g["ksi"], None, 0.0, *_table(g))
    ref = O.solve_rate_equations(*args)
    assert ref[3] > 0      # the 16^3 field holds a cell at which the reference stops
    assert O.device_solve_rate_equations(*args)[3] == ref[3]
    _share("ten decades", O.device_chem_tame(*args))


@pytest.fixture(scope="module", params=["k1", "k4"])
def vanishing(request, golden):
    """the fields of test_chem_gpu.py::test_vanishing_rate_coefficients_where_nothing_ionises_bitwise: a table whose k1 or k4 is
    below 1e-278 or exactly 0 at the lowest temperatures, in cells that nothing ionises"""
    g = golden("chem_uvb_refined")
    logtem0, logtem9, dlogtem = float(g["logtem0"]), float(g["logtem9"]), float(g["dlogtem"])
    uniform, threshold = np.array([3e-14, 1e-16, 2e-14]), 1e300      # mfp < threshold everywhere: shielded
    rows, zero_rows = 1000, 100
    rng = np.random.default_rng(3)
    k = np.array(g["k"], dtype=np.float64, copy=True)
    r = {"k1": 0, "k4": 3}[request.param]
    k[r, :rows] = 10 ** rng.uniform(-300, -279, rows)
    k[r, rows - zero_rows:rows] = 0.0
    if request.param == "k4":
        k[2, :rows] = 0.0

    def args(rho, tgas, start):
        return (1 if len(rho) == 1 else N, np.zeros(len(rho), np.int32), BOX, rho, tgas, *start, None, False, None, None, uniform, threshold,
                logtem0, logtem9, dlogtem, k)

    m = 3 * NC
    rho = 10 ** rng.uniform(-30, -16, m)
    nh, nhe = PSI * rho / MP, (1 - PSI) * rho / (2 * (MP + MN))
    tgas = np.exp(logtem0 + rng.uniform(0, (rows - zero_rows - 1) * dlogtem, m))
    start = (nh * 10 ** rng.uniform(-3, 0, m), nhe * 10 ** rng.uniform(-3, -0.5, m), nhe * 10 ** rng.uniform(-3, -0.5, m))
    converges = np.array([O.solve_rate_equations(*args(rho[i:i + 1], tgas[i:i + 1], [a[i:i + 1] for a in start]))[3] == 0 for i in range(m)])
    keep = np.flatnonzero(converges)[:NC]
    assert keep.size == NC
    rho, tgas, start = rho[keep], tgas[keep], tuple(a[keep] for a in start)
    hot = np.arange(1000, NC, 397)      # cells on the zero rows from cell 1000 on: the reference stops at the first of them
    tgas2 = tgas.copy()
    tgas2[hot] = np.exp(logtem0 + (rows - zero_rows / 2) * dlogtem)
    return request.param, args(rho, tgas, start), args(rho, tgas2, start), hot


def test_vanishing_rate_coefficients(vanishing):
    name, converging, stopping, hot = vanishing
    ref = O.solve_rate_equations(*converging)
    assert ref[3] == 0 and ref[4] > 0
    assert _same(O.device_solve_rate_equations(*converging), ref)
    ref = O.solve_rate_equations(*stopping)
    assert ref[3] == 1 + hot[0]
    assert O.device_solve_rate_equations(*stopping)[3] == ref[3]


def test_no_cell_of_the_vanishing_fields_is_tame(vanishing):
    """k1 de + kr24 or k4 de is subnormal or zero at de = 1e-30 there: the trimmed division would return NaN"""
    name, converging, stopping, _ = vanishing
    for label, args in (("converging", converging), ("stopping", stopping)):
        tame = O.device_chem_tame(*args)
        _share(f"vanishing {name}, {label}", tame)
        assert not tame.any()
