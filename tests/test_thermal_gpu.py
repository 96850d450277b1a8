"""The thermal balance on the GPU: ftte_thermal_equilibrium* and ftte_advance_temperature* (thermal_equilibrium_kernel,
thermal_advance_kernel) through the C ABI against the host evaluation of the same header (tests/_thermal.py:
ftte_thermal_math.h compiled by g++), bit for bit -- the statement consists of IEEE additions, multiplications, divisions and
explicit fused multiply-adds, its logarithm included -- and the driver radiativetransfer_amd.evolve(thermal=...) against the same
calls made by hand."""
import numpy as np
import pytest

import _oracle as O
import _thermal as T

pytestmark = pytest.mark.gpu

EPS = T.EPS


@pytest.fixture(scope="module")
def stellar():
    import radiativetransfer_amd as rt
    st = rt.StellarTransfer()
    yield st
    st.close()


@pytest.fixture(scope="module")
def chem(golden):
    return golden("chem_uvb_refined")


@pytest.fixture(scope="module")
def grid(chem):
    return float(chem["logtem0"]), float(chem["logtem9"]), float(chem["dlogtem"])


def _case(golden, grid, name):
    if name.startswith("wide"):
        return T.wide_medium(grid, uniform=name == "wide_uniform")
    return T.golden_case(golden(name), name, grid)


def _load(st, case, chem, tab=None):
    tab = T.tables() if tab is None else tab
    n, level, box, rho, tgas, HI, HeI, HeII = case["head"]
    st.set_grid(n, level, box)
    st.set_rate_coefficients(*case["grid"], chem["k"])
    st.set_cooling_coefficients(tab["cool"], tab["compa"], T.REDSHIFT)
    st.set_medium(HI, HeI, HeII, rho, None, 0)
    st.set_temperature(tgas)
    if case["rates"] is not None:
        st.set_rates(case["rates"])


def _rates(case, tab, J=None):
    """the rate arguments of thermal_equilibrium / advance_temperature for a case"""
    return dict(run_uvb=case["run_uvb"], J=case["J"] if J is None else J, gamma=tab["gamma"], uniform_gamma=tab["uniform_gamma"],
                threshold=case["threshold"], use_point_rates=case["rates"] is not None)


def _same_arrays(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} cells differ, first {bad[:5]}: {got[bad[:3]]} vs {want[bad[:3]]}"


@pytest.mark.parametrize("name,mode", [("initial_refined", "host"), ("chem_uniform_background", "host"), ("chem_uvb_refined", "host"),
                                       ("chem_uvb_refined", "device J")])
def test_equilibrium_bitwise(stellar, golden, chem, grid, name, mode):
    import torch
    case, tab = _case(golden, grid, name), T.tables()
    _load(stellar, case, chem)
    ref = T.equilibrium(*case["head"], *T.rate_args(case, tab))
    assert ref[3] == 0
    if mode == "device J":
        J = torch.from_numpy(np.ascontiguousarray(case["J"])).cuda()
        torch.cuda.synchronize()
        got = stellar.thermal_equilibrium(True, None, tab["gamma"], None, 0.0, True, j_device_ptr=J.data_ptr())
    else:
        got = stellar.thermal_equilibrium(**_rates(case, tab))
    for what, a, b in zip(("heating", "cooling", "hydroHeating"), got, ref[:3]):
        _same_arrays(a, b, what)
    assert np.any(got[0] > 0) and np.any(got[1] > 0)


@pytest.mark.parametrize("name", ["initial_refined", "chem_uniform_background", "chem_uvb_refined", "wide"])
def test_advance_bitwise(stellar, golden, chem, grid, name):
    """temperature(), rate_equation_steps() and max_change against the host evaluation, which settles every cell"""
    case, tab = _case(golden, grid, name), T.tables()
    _load(stellar, case, chem)
    for dt, sub in T.STEPS:
        stellar.set_temperature(case["head"][4])
        ref = T.advance(*case["head"], *T.rate_args(case, tab), dt, sub)
        assert ref[2] == 0
        change = stellar.advance_temperature(dt, substeps=sub, **_rates(case, tab))
        _same_arrays(stellar.temperature(), ref[0], f"temperature after {dt:g} x{sub}")
        assert stellar.rate_equation_steps() == int(ref[3].sum()) and ref[3].sum() > 0
        assert change == ref[4].max()


def test_node_major_table(golden, chem, grid, monkeypatch):
    """the alternative layout of the device's cooling table (FTTE_THERMAL_TABLE=nodes, kept for measurements): the same bits"""
    import radiativetransfer_amd as rt
    case, tab = _case(golden, grid, "wide"), T.tables()
    monkeypatch.setenv("FTTE_THERMAL_TABLE", "nodes")
    with rt.StellarTransfer() as st:
        _load(st, case, chem)
        dt, sub = T.STEPS[1]
        ref = T.advance(*case["head"], *T.rate_args(case, tab), dt, sub)
        assert ref[2] == 0
        st.advance_temperature(dt, substeps=sub, **_rates(case, tab))
        _same_arrays(st.temperature(), ref[0], "temperature")
        got = st.thermal_equilibrium(**_rates(case, tab))
    ref = T.equilibrium(*case["head"][:4], ref[0], *case["head"][5:], *T.rate_args(case, tab))
    assert ref[3] == 0 and all(np.array_equal(a, b) for a, b in zip(got, ref[:3]))


@pytest.mark.parametrize("name", ["initial_refined", "wide_uniform"])
def test_stationarity(stellar, golden, chem, grid, name):
    """with the stored hydroHeating every cell that has some stays exactly where it is; the others that are heated end warmer"""
    case, tab = _case(golden, grid, name), T.tables()
    _load(stellar, case, chem)
    tgas = case["head"][4]
    heating, cooling, hydro = stellar.thermal_equilibrium(**_rates(case, tab))
    held, rising = hydro > 0, (hydro == 0) & (heating - cooling > 0)
    assert held.any()
    for dt, sub in T.STEPS:
        stellar.set_temperature(tgas)
        stellar.advance_temperature(dt, substeps=sub, tmin=0.1, hydro_heating=True, **_rates(case, tab))
        T1 = stellar.temperature()
        ref = T.advance(*case["head"], *T.rate_args(case, tab), dt, sub, tmin=0.1, hydro=hydro)
        assert ref[2] == 0
        _same_arrays(T1, ref[0], "temperature")
        assert np.array_equal(T1[held], tgas[held]) and np.all(T1[rising] > tgas[rising])


@pytest.mark.parametrize("dt,sub", T.STEPS)
def test_compton_limit(stellar, golden, chem, grid, dt, sub):
    """zero tables, no heating: backward Euler in closed form, the bound of tests/test_thermal_host.py::test_compton_limit"""
    from test_thermal_host import compton_formula
    case, tab = _case(golden, grid, "wide"), dict(T.tables())
    tab["cool"] = np.zeros_like(tab["cool"])
    _load(stellar, case, chem, tab)
    stellar.advance_temperature(dt, False, None, None, np.zeros(3), 0.0, substeps=sub)
    T1 = stellar.temperature()
    T0, want = compton_formula(case, tab, dt, sub)
    err = np.abs(T1 - want) / (16 * EPS * (T1 + T0 + tab["comp2"]))
    print(f"Compton limit dt {dt:g} x{sub}: worst error / bound {err.max():.3f}")
    assert err.max() <= 1.0


def test_stride_loop(chem, grid):
    """164^3 = 4 410 944 leaves, more than the 16 384 x 256 threads of a launch: the first, the last and 10^4 random cells"""
    import radiativetransfer_amd as rt
    tab = T.tables()
    n, box = 164, 2.5e23
    nc = n ** 3
    assert nc > 16384 * 256
    rng = np.random.default_rng(3)
    rho = 3.0e-26 * np.exp(rng.normal(0.0, 0.8, nc))
    nh, nhe = T.PSI * rho / T.MH, (1 - T.PSI) * rho / T.MHE
    tgas = 10 ** rng.uniform(3.0, 5.0, nc)
    J = 10 ** rng.uniform(-23.5, -21.5, (3, nc))
    start = (0.5 * nh, 0.4 * nhe, 0.3 * nhe)
    dt, sub = 1e12, 2
    with rt.StellarTransfer() as st:
        st.set_uniform_grid(n, box)
        st.set_rate_coefficients(*grid, chem["k"])
        st.set_cooling_coefficients(tab["cool"], tab["compa"], T.REDSHIFT)
        st.set_medium(*start, rho, None, 0)
        st.set_temperature(tgas)
        st.advance_temperature(dt, True, J, tab["gamma"], substeps=sub)
        T1 = st.temperature()
        heating, cooling, hydro = st.thermal_equilibrium(True, J, tab["gamma"])
    pick = np.unique(np.concatenate(([0, nc - 1], rng.choice(nc, 10000, replace=False))))
    head = (n, np.zeros(pick.size, np.int32), box, rho[pick])
    species = [s[pick] for s in start]
    args = (None, True, J[:, pick], tab["gamma"], None, 0.0, *grid, tab["cool"], tab["comp1"], tab["comp2"])
    ref = T.advance(*head, tgas[pick], *species, *args, dt, sub)
    assert ref[2] == 0
    assert np.array_equal(T1[pick], ref[0])
    assert np.all((T1 >= T.TMIN) & (T1 <= T.TMAX))
    ref = T.equilibrium(*head, T1[pick], *species, *args)      # (the pass ran at the new temperature)
    assert ref[3] == 0
    assert np.array_equal(heating[pick], ref[0]) and np.array_equal(cooling[pick], ref[1]) and np.array_equal(hydro[pick], ref[2])


def test_hand_over_to_the_chemistry(stellar, golden, chem, grid):
    """before any advance the equilibrium update is today's (the host logarithm of set_temperature); after one it reads ftte_log(T1)"""
    case, tab = _case(golden, grid, "chem_uvb_refined"), T.tables()
    n, level, box, rho, tgas, HI, HeI, HeII = case["head"]
    _load(stellar, case, chem)
    stellar.solve_rate_equations(True, chem["J"], chem["ksi"])
    want = O.solve_rate_equations(n, level, box, rho, tgas, HI, HeI, HeII, None, True, chem["J"], chem["ksi"], None, 0.0, *grid, chem["k"])
    assert want[3] == 0 and all(np.array_equal(a, b) for a, b in zip(stellar.medium(), want[:3]))
    stellar.set_medium(HI, HeI, HeII, rho, None, 0)
    stellar.advance_temperature(1e13, substeps=3, **_rates(case, tab))
    ref = T.advance(*case["head"], *T.rate_args(case, tab), 1e13, 3)
    assert ref[2] == 0 and np.array_equal(stellar.temperature(), ref[0]) and np.any(ref[0] != tgas)
    stellar.solve_rate_equations(True, chem["J"], chem["ksi"])
    want = T.solve_at(n, level, box, rho, ref[1], HI, HeI, HeII, chem["J"], chem["ksi"], *grid, chem["k"])
    assert want[3] == 0
    for a, b in zip(stellar.medium(), want[:3]):
        _same_arrays(a, b, "species after the hand-over")
    today = O.solve_rate_equations(n, level, box, rho, tgas, HI, HeI, HeII, None, True, chem["J"], chem["ksi"], None, 0.0, *grid, chem["k"])
    assert not np.array_equal(today[0], want[0])      # (the new temperature was read)


def _expect(status, fn, *args, **kw):
    from radiativetransfer_amd import FtteError
    with pytest.raises(FtteError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)
    return str(e.value)


def test_refusals(stellar, golden, chem, grid):
    import radiativetransfer_amd as rt
    case, tab = _case(golden, grid, "chem_uvb_refined"), T.tables()
    n, level, box, rho, tgas, HI, HeI, HeII = case["head"]
    r = _rates(case, tab)
    with rt.StellarTransfer() as st:
        st.set_grid(n, level, box)
        assert "rate coefficients" in _expect("FTTE_ERR_STATE", st.set_cooling_coefficients, tab["cool"], tab["compa"], T.REDSHIFT)
        st.set_rate_coefficients(*grid, chem["k"])
        st.set_medium(HI, HeI, HeII, rho, None, 0)
        st.set_temperature(tgas)
        st.set_rates(case["rates"])
        assert "cooling coefficients" in _expect("FTTE_ERR_STATE", st.advance_temperature, 1e12, **r)
        assert "cooling coefficients" in _expect("FTTE_ERR_STATE", st.thermal_equilibrium, **r)
        _expect("FTTE_ERR_ARG", st.set_cooling_coefficients, tab["cool"][:, :100], tab["compa"], T.REDSHIFT)      # another nratec
        st.set_cooling_coefficients(tab["cool"], tab["compa"], T.REDSHIFT)
        assert "hydroHeating" in _expect("FTTE_ERR_STATE", st.advance_temperature, 1e12, hydro_heating=True, **r)
        for dt in (0.0, -1.0, float("inf"), float("nan")):
            _expect("FTTE_ERR_ARG", st.advance_temperature, dt, **r)
        for sub in (0, -1, 4097):
            _expect("FTTE_ERR_ARG", st.advance_temperature, 1e12, substeps=sub, **r)
        for tmin, tmax in ((0.0, 1e9), (-1.0, 1e9), (10.0, 10.0), (10.0, 1.0), (1.0, float("inf")), (float("nan"), 1e9)):
            _expect("FTTE_ERR_ARG", st.advance_temperature, 1e12, tmin=tmin, tmax=tmax, **r)
        _expect("FTTE_ERR_ARG", st.advance_temperature, 1e12, True, None, tab["gamma"])
        _expect("FTTE_ERR_ARG", st.advance_temperature, 1e12, False, None, None, None)
        st.thermal_equilibrium(**r)
        st.advance_temperature(1e12, hydro_heating=True, substeps=4096, **r)
        # one NaN temperature: the cell is named, and the temperature and its logarithm are left as they were
        bad = tgas.copy()
        bad[7] = np.nan
        st.set_temperature(bad)
        st.solve_rate_equations(True, chem["J"], chem["ksi"])
        before = st.medium()
        assert T.advance(*case["head"][:4], bad, HI, HeI, HeII, *T.rate_args(case, tab), 1e12, 1)[2] == 8
        text = _expect("FTTE_ERR_RATES", st.advance_temperature, 1e12, **r)
        assert "cell 7 " in text and "ftte_advance_temperature" in text
        assert "cell 7 " in _expect("FTTE_ERR_RATES", st.thermal_equilibrium, **r)
        now = st.temperature()
        assert np.isnan(now[7]) and np.array_equal(np.delete(now, 7), np.delete(tgas, 7))
        st.set_medium(HI, HeI, HeII, rho, None, 0)
        st.solve_rate_equations(True, chem["J"], chem["ksi"])      # logtem unchanged: the same update from the same state
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(st.medium(), before))
        # another grid: the temperature and hydroHeating belong to the old one
        st.set_grid(2, np.zeros(8, np.int32), 1e22)
        z = np.full(8, 1e-6)
        st.set_medium(z, z * 0.05, z * 0.01, np.full(8, 3e-24), None, 0)
        assert "temperature" in _expect("FTTE_ERR_STATE", st.advance_temperature, 1e12, False, None, None, np.zeros(3), 0.0)
        st.set_temperature(np.full(8, 1e4))
        assert "hydroHeating" in _expect("FTTE_ERR_STATE", st.advance_temperature, 1e12, False, None, None, np.zeros(3), 0.0, hydro_heating=True)
        st.advance_temperature(1e12, False, None, None, np.zeros(3), 0.0)


def test_device_objects_come_back(stellar, golden, chem, grid):
    import radiativetransfer_amd as rt
    case, tab = _case(golden, grid, "chem_uvb_refined"), T.tables()
    before = stellar.counter("device_objects")
    with rt.StellarTransfer() as st:
        _load(st, case, chem)
        st.thermal_equilibrium(**_rates(case, tab))
        st.advance_temperature(1e12, hydro_heating=True, **_rates(case, tab))
        assert st.counter("device_objects") > before
    assert stellar.counter("device_objects") == before


def test_multi_device_context_refuses(golden, chem, grid):
    import radiativetransfer_amd as rt
    case, tab = _case(golden, grid, "chem_uvb_refined"), T.tables()
    with rt.StellarTransfer(devices=[0, 0]) as st:
        st.set_grid(*[case["head"][i] for i in (0, 1, 2)])
        _expect("FTTE_ERR_UNSUPPORTED", st.set_cooling_coefficients, tab["cool"], tab["compa"], T.REDSHIFT)
        _expect("FTTE_ERR_UNSUPPORTED", st.temperature)
        _expect("FTTE_ERR_UNSUPPORTED", st.thermal_equilibrium, True, case["J"], tab["gamma"])
        _expect("FTTE_ERR_UNSUPPORTED", st.thermal_equilibrium, True, None, tab["gamma"], j_device_ptr=0)
        _expect("FTTE_ERR_UNSUPPORTED", st.advance_temperature, 1e12, True, case["J"], tab["gamma"])
        _expect("FTTE_ERR_UNSUPPORTED", st.advance_temperature_device, 1e12, 0, tab["gamma"])


def _evolve_setup(st, golden, chem, grid, rng):
    import radiativetransfer_amd as rt
    g, tab = golden("expansion_refined"), T.tables()      # a 12^3 base grid with refined cells
    n, level, box = int(g["n"]), g["level"], float(g["box"])
    tgas = 10 ** rng.uniform(3.5, 4.5, level.size)
    st.set_grid(n, level, box)
    st.set_rate_coefficients(*grid, chem["k"])
    st.set_cooling_coefficients(tab["cool"], tab["compa"], T.REDSHIFT)
    st.set_medium(g["HI"], g["HeI"], g["HeII"], g["rho"], None, 0)
    st.set_temperature(tgas)
    st.set_rate_tables(golden("point16_homogeneous")["tables"])
    beta = np.array([[6.3e-18, 1.2e-18, 2.0e-19], [0.0, 7.4e-18, 1.5e-18], [0.0, 0.0, 1.6e-18]])
    ang = np.array([rt.pix2ang_nest(1, i) for i in range(12)])
    return dict(sources=(np.array([int(g["src_cell"][0])]), np.array([50.0])), directions=(ang[:, 0].copy(), ang[:, 1].copy(), np.full(12, 1.0 / 12)),
                beta=beta, uvb=np.array([2e-22, 1e-22, 3e-23]), ksi=chem["ksi"], substeps=2)


def _by_hand(st, dt, nsteps, kw, thermal):
    """evolve's sequence of library calls, written out"""
    import torch
    J = torch.empty((3, st.ncell), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream()
    mass = st.hydrogen_mass()
    neutral = [mass[0] / mass[1]]
    for _ in range(nsteps):
        st.set_zero_rates()
        st.point_sources(*kw["sources"])
        st.compute_opacities_from_medium(kw["beta"])
        st.transport_device(*kw["directions"], kw["uvb"], J.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        st.advance_rate_equations_device(dt, J.data_ptr(), kw["ksi"], use_point_rates=True, substeps=kw["substeps"])
        if thermal is not None:
            st.advance_temperature_device(dt, J.data_ptr(), thermal["gamma"], use_point_rates=True, substeps=kw["substeps"], tmin=thermal["tmin"],
                                          tmax=thermal["tmax"], hydro_heating=thermal["hydro_heating"])
        mass = st.hydrogen_mass()
        neutral.append(mass[0] / mass[1])
    return np.array(neutral), st.medium(), st.temperature()


@pytest.mark.parametrize("with_thermal", [True, False])
def test_evolve(golden, chem, grid, with_thermal):
    """three steps with one source against the same calls made by hand, bit for bit: with thermal=..., the temperature step after
    each ionisation advance; with thermal=None, today's sequence and an untouched temperature"""
    import radiativetransfer_amd as rt
    thermal = dict(gamma=T.tables()["gamma"], tmin=10.0, tmax=1e8, hydro_heating=False) if with_thermal else None
    dt, out = 3e12, []
    for driver in ("evolve", "by hand"):
        with rt.StellarTransfer() as st:
            kw = _evolve_setup(st, golden, chem, grid, np.random.default_rng(11))
            start = st.temperature()
            if driver == "evolve":
                times, neutral = rt.evolve(st, dt, 3, thermal=thermal, **kw)
                assert np.array_equal(times, dt * np.arange(4))
                out.append((neutral, st.medium(), st.temperature()))
            else:
                out.append(_by_hand(st, dt, 3, kw, thermal))
    (n1, m1, t1), (n2, m2, t2) = out
    assert np.array_equal(n1, n2) and all(np.array_equal(a, b) for a, b in zip(m1, m2)) and np.array_equal(t1, t2)
    assert np.any(t1 != start) if with_thermal else np.array_equal(t1, start)
