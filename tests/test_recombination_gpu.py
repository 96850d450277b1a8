"""The diffuse recombination source on the GPU: ftte_recombination_source* (recombination_source_kernel) through the C ABI against
the host evaluation of the same header (tests/_recombination.py: ftte_recombination_math.h compiled by g++), bit for bit; the sweep
that carries it against the same values handed over by ftte_set_source_function; a closed thick box, where J must be S; the
on-the-spot limit reached through the library; the refusals; and radiativetransfer_amd.evolve(recombination=...) against the same
calls made by hand."""
import math

import numpy as np
import pytest

import _recombination as R

pytestmark = pytest.mark.gpu

EPS = R.EPS
UVB = np.array([2e-22, 1e-22, 3e-23])


@pytest.fixture(scope="module")
def tab():
    return R.tables()


@pytest.fixture(scope="module")
def dirs():
    import radiativetransfer_amd as rt
    return rt.healpix_directions(1)      # the 12 rotated level-1 directions, weights 1/12


def _load(st, m, tab, k=None, g=None):
    """grid, tables, medium, temperature and opacities in three groups: everything recombination_source needs"""
    st.set_grid(m["n"], m["level"], m["box"])
    st.set_rate_coefficients(*tab["grid"], tab["kb"] if k is None else k)
    st.set_ground_recombination(tab["g"] if g is None else g)
    st.set_medium(m["HI"], m["HeI"], m["HeII"], m["rho"], None, 0)
    st.set_temperature(m["tgas"])
    st.compute_opacities_from_medium(tab["beta"])


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first {bad[:5]}: {got.ravel()[bad[:3]]} vs {want.ravel()[bad[:3]]}"


def _expect(status, fn, *args, **kw):
    from radiativetransfer_amd import FtteError
    with pytest.raises(FtteError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)
    return str(e.value)


# ---- 1. the kernel against the host evaluation ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.MEDIA)
def test_kernel_bitwise(golden, tab, name):
    """S of the host-output and of the device-output form, and the lost counts, on two refined goldens and the wide medium (32^3:
    temperatures beyond both ends of the table, helium over its budget), for the identity and for shares that split the rows"""
    import torch
    import radiativetransfer_amd as rt
    m = R.medium(golden, name)
    logtem = R.libm_log(m["tgas"])
    with rt.StellarTransfer() as st:
        _load(st, m, tab)
        for share in (R.IDENTITY, R.SPLIT):
            want, _, wlost, status = R.source(m["rho"], logtem, m["HI"], m["HeI"], m["HeII"], tab["grid"], tab["g"], tab["ksi"], share)
            assert status == 0 and np.count_nonzero(want) > want.size // 2
            S, lost = st.recombination_source(tab["ksi"], share)
            _same(S, want, f"{name}: S (host output)")
            assert lost == wlost
            S_dev = torch.full((3, st.ncell), -1.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            assert st.recombination_source_device(tab["ksi"], share, S_dev.data_ptr()) == wlost
            _same(S_dev.cpu().numpy(), want, f"{name}: S (device output)")
            assert st.recombination_source(tab["ksi"], share, want_S=False) == (None, wlost)


# ---- 2. the sweep sees it -----------------------------------------------------------------------------------------------------

def _uniform16():
    import _thermal
    n, level, box, rho, tgas, HI, HeI, HeII = _thermal.wide_medium(None, n=16, seed=23)["head"]
    return dict(n=n, level=level, box=1.0e21, rho=rho, tgas=tgas, HI=HI, HeI=HeI, HeII=HeII)      # (a box a sweep partly sees through)


@pytest.mark.parametrize("case", ["uniform16", "refined (hybrid)", "uniform16, tile engine"])
def test_the_sweep_sees_it(golden, tab, dirs, case):
    """recombination_source then transport equals set_source_function(the S returned) then transport, bit for bit in J -- with no
    emission in force before the call (the kernel writes the field), and with one in force (computed beside it, copied in on success)"""
    import radiativetransfer_amd as rt
    m = R.medium(golden, "chem_uvb_refined") if case.startswith("refined") else _uniform16()
    with rt.StellarTransfer() as st:
        if case.endswith("tile engine"):
            st.set_option("engine", 1)
        _load(st, m, tab)
        plain = st.transport(*dirs, UVB)
        S, lost = st.recombination_source(tab["ksi"], R.SPLIT)
        J1 = st.transport(*dirs, UVB)
        S2, _ = st.recombination_source(tab["ksi"], R.IDENTITY)      # emission in force: computed beside it, then copied in
        J2 = st.transport(*dirs, UVB)
        S3, _ = st.recombination_source(tab["ksi"], R.SPLIT)         # and once more
        J3 = st.transport(*dirs, UVB)
        _same(S3, S, "S again")
        _same(J3, J1, "J with S again")
        st.set_source_function(None)
        _same(st.transport(*dirs, UVB), plain, "J without emission")
        st.set_source_function(S)
        _same(st.transport(*dirs, UVB), J1, "J after set_source_function(S)")
        st.set_source_function(S2)
        _same(st.transport(*dirs, UVB), J2, "J after set_source_function(S2)")
        assert np.any(J1 != plain) and np.any(J2 != J1)


# ---- 3, 4. a closed thick box ---------------------------------------------------------------------------------------------------

N, T_BOX, RHO = 16, 3.0e4, 1.0e-24
CENTRE = (8 * N + 8) * N + 8


@pytest.fixture(scope="module")
def box(tab):
    """A uniform 16^3 medium at 3e4 K in the case-B collisional equilibrium the library finds itself (no radiation), in a box sized so
    that HI beta[HI][group 0] per cell is 8 >= 5.  -> the medium, and the context's equilibrium HI of the centre cell."""
    import radiativetransfer_amd as rt
    nc = N ** 3
    nh, nhe = R.PSI * RHO / R.MH, (1 - R.PSI) * RHO / R.MHE
    m = dict(n=N, level=np.zeros(nc, np.int32), box=1.0e22, rho=np.full(nc, RHO), tgas=np.full(nc, T_BOX), HI=np.full(nc, 0.5 * nh),
             HeI=np.full(nc, 0.5 * nhe), HeII=np.full(nc, 0.3 * nhe))
    with rt.StellarTransfer() as st:
        _load(st, m, tab)
        st.solve_rate_equations(True, np.zeros((3, nc)), tab["ksi"])
        m["HI"], m["HeI"], m["HeII"] = st.medium()
    assert np.all(m["HI"] == m["HI"][0]) and 1e-3 < m["HI"][0] / nh < 1e-2
    m["box"] = N * 8.0 / (m["HI"][0] * tab["beta"][0, 0])
    return m


def test_closed_thick_box(box, tab, dirs):
    """uvb = 0, the H row only: J1 of the centre cell is S1 to 64 eps + exp(-35) relative -- every path from a boundary to the centre
    crosses at least 7 cells of tau >= 5 -- and J2, J3 are exactly 0 everywhere"""
    import radiativetransfer_amd as rt
    with rt.StellarTransfer() as st:
        _load(st, box, tab)
        S, lost = st.recombination_source(tab["ksi"], R.H_ONLY)
        J = st.transport(*dirs, np.zeros(3))
    assert lost == 0 and S[0, CENTRE] > 0 and not S[1:].any()
    assert box["HI"][0] * tab["beta"][0, 0] * box["box"] / N >= 5.0
    err = abs(J[0, CENTRE] - S[0, CENTRE]) / S[0, CENTRE]
    print(f"closed box: |J1 - S1| / S1 at the centre = {err:.3e} = {err / EPS:.2f} eps")
    assert err <= 64 * EPS + math.exp(-35.0)
    assert not J[1:].any()
    # a corner cell looks out of the box: a direction that enters it from outside with I = 0 leaves its mean short by at least
    # (1 - exp(-tau)) / tau, tau <= 8 sqrt(3), and weighs 1/12
    assert J[0, 0] < (1.0 - 0.005) * S[0, 0]


def test_on_the_spot_limit(box, tab, dirs):
    """The box at 3e4 K, collisional ionisation only: {opacities, recombination source, sweep, equilibrium update} with case-A k2 (k4,
    k6 case B) until max_change < 1e-12, at most 200 rounds (the map contracts with q = g/k2_A = 0.46 here).  The centre cell's HI
    equals the case-B equilibrium without emission to 1e-9 relative: the stop error 1e-12 of the fraction, over HI/nh = 2.4e-3 and
    times q/(1 - q), is 3.6e-10; the leak of the closed box is exp(-35)."""
    import torch
    import radiativetransfer_amd as rt
    k = tab["kb"].copy()
    k[1] = tab["ka"][1]
    assert np.array_equal(tab["ka"][[0, 2, 4]], tab["kb"][[0, 2, 4]])      # (the collisional rows are the same in both cases)
    J = torch.zeros((3, N ** 3), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream()
    with rt.StellarTransfer() as st:
        _load(st, box, tab, k=k)
        for rounds in range(1, 201):
            st.compute_opacities_from_medium(tab["beta"])
            st.recombination_source_device(tab["ksi"], R.H_ONLY)
            st.transport_device(*dirs, np.zeros(3), J.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            change = st.solve_rate_equations_device(J.data_ptr(), tab["ksi"])
            if change < 1e-12:
                break
        HI = st.medium()[0]
    want = box["HI"][CENTRE]
    err = abs(HI[CENTRE] - want) / want
    print(f"on-the-spot limit: {rounds} rounds, last change {change:.3e}, |HI - HI_B| / HI_B at the centre = {err:.3e}")
    assert rounds < 200 and change < 1e-12
    assert err <= 1e-9
    assert HI[0] > 1.001 * want      # (the corner loses some of its photons and stays more neutral: emission is what closes the gap)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals(golden, tab, dirs):
    import radiativetransfer_amd as rt
    m = R.medium(golden, "chem_uvb_refined")
    nc = m["level"].size
    ksi, g = tab["ksi"], tab["g"]
    with rt.StellarTransfer() as st:
        assert "ftte_set_grid" in _expect("FTTE_ERR_STATE", st.recombination_source, ksi, R.IDENTITY)
        st.set_grid(m["n"], m["level"], m["box"])
        assert "medium with density" in _expect("FTTE_ERR_STATE", st.recombination_source, ksi, R.IDENTITY)
        st.set_medium(m["HI"], m["HeI"], m["HeII"])
        assert "medium with density" in _expect("FTTE_ERR_STATE", st.recombination_source, ksi, R.IDENTITY)
        st.set_medium(m["HI"], m["HeI"], m["HeII"], m["rho"], None, 0)
        assert "ftte_set_temperature" in _expect("FTTE_ERR_STATE", st.recombination_source, ksi, R.IDENTITY)
        st.set_temperature(m["tgas"])
        assert "ftte_set_rate_coefficients" in _expect("FTTE_ERR_STATE", st.recombination_source, ksi, R.IDENTITY)
        assert "ftte_set_rate_coefficients" in _expect("FTTE_ERR_STATE", st.set_ground_recombination, g)
        st.set_rate_coefficients(*tab["grid"], tab["kb"])
        assert "ftte_set_ground_recombination" in _expect("FTTE_ERR_STATE", st.recombination_source_device, ksi, R.IDENTITY)
        _expect("FTTE_ERR_ARG", st.set_ground_recombination, g[:, :100])      # another nratec
        for value in (-1e-13, math.nan, math.inf):
            bad = g.copy()
            bad[1, 4321] = value
            assert "g[1][4321]" in _expect("FTTE_ERR_ARG", st.set_ground_recombination, bad)
        st.set_ground_recombination(g)
        assert "opacities" in _expect("FTTE_ERR_STATE", st.recombination_source, ksi, R.IDENTITY)
        st.set_opacity(np.full((8, nc), 1e-22))
        assert "8 frequency groups" in _expect("FTTE_ERR_STATE", st.recombination_source, ksi, R.IDENTITY)
        st.compute_opacities_from_medium(tab["beta"])
        for i, j, value in ((0, 0, 1.5), (1, 2, -0.1), (2, 1, math.nan)):
            share = R.IDENTITY.copy()
            share[i, j] = value
            assert f"share[{i}][{j}]" in _expect("FTTE_ERR_ARG", st.recombination_source, ksi, share)
        share = np.array([[0.5, 0.4, 0.2], [0, 1, 0], [0, 0, 1.0]])      # a row that adds up to 1.1
        assert "ion 0" in _expect("FTTE_ERR_ARG", st.recombination_source_device, ksi, share)
        S, lost = st.recombination_source(ksi, R.IDENTITY)
        # another nratec of the rate coefficients drops the table, as it drops the cooling coefficients
        st.set_rate_coefficients(tab["grid"][0], tab["grid"][1], (tab["grid"][1] - tab["grid"][0]) / 99, tab["kb"][:, ::50][:, :100])
        assert "ftte_set_ground_recombination" in _expect("FTTE_ERR_STATE", st.recombination_source, ksi, R.IDENTITY)


@pytest.mark.parametrize("in_force", [False, True])
def test_a_bad_leaf_leaves_the_emission_as_it_was(golden, tab, dirs, in_force):
    """rho = 0 in leaf 5: FTTE_ERR_RATES names it, and a sweep afterwards equals one before -- without emission, and with the caller's
    source function in force"""
    import radiativetransfer_amd as rt
    m = dict(R.medium(golden, "chem_uvb_refined"))
    rng = np.random.default_rng(2)
    mine = 10 ** rng.uniform(-24, -21, (3, m["level"].size))
    with rt.StellarTransfer() as st:
        _load(st, m, tab)
        if in_force:
            st.set_source_function(mine)
        before = st.transport(*dirs, UVB)
        rho = m["rho"].copy()
        rho[5] = 0.0
        st.set_medium(m["HI"], m["HeI"], m["HeII"], rho, None, 0)
        text = _expect("FTTE_ERR_RATES", st.recombination_source, tab["ksi"], R.IDENTITY)
        assert "cell 5 " in text and "ftte_recombination_source" in text
        _same(st.transport(*dirs, UVB), before, "J after the refusal")
        assert "cell 5 " in _expect("FTTE_ERR_RATES", st.recombination_source_device, tab["ksi"], R.IDENTITY)
        _same(st.transport(*dirs, UVB), before, "J after the second refusal")
        st.set_medium(m["HI"], m["HeI"], m["HeII"], m["rho"], None, 0)
        st.recombination_source(tab["ksi"], R.IDENTITY)
        assert np.any(st.transport(*dirs, UVB) != before)


def test_multi_device_context_refuses(golden, tab):
    import radiativetransfer_amd as rt
    m = R.medium(golden, "chem_uvb_refined")
    with rt.StellarTransfer(devices=[0, 0]) as st:
        st.set_grid(m["n"], m["level"], m["box"])
        _expect("FTTE_ERR_UNSUPPORTED", st.set_ground_recombination, tab["g"])
        _expect("FTTE_ERR_UNSUPPORTED", st.recombination_source, tab["ksi"], R.IDENTITY)
        _expect("FTTE_ERR_UNSUPPORTED", st.recombination_source_device, tab["ksi"], R.IDENTITY)


def test_device_objects_come_back(golden, tab, dirs):
    import radiativetransfer_amd as rt
    m = R.medium(golden, "initial_refined")
    with rt.StellarTransfer() as outer:
        before = outer.counter("device_objects")
        with rt.StellarTransfer() as st:
            _load(st, m, tab)
            st.recombination_source(tab["ksi"], R.SPLIT)
            st.recombination_source(tab["ksi"], R.SPLIT)      # (the buffer beside the field too)
            st.transport(*dirs, UVB)
            assert st.counter("device_objects") > before
        assert outer.counter("device_objects") == before


# ---- 6. evolve -------------------------------------------------------------------------------------------------------------------

def _evolve_setup(st, golden, tab):
    import _thermal
    g, th = golden("expansion_refined"), _thermal.tables()      # a 12^3 base grid with refined cells
    n, level, box = int(g["n"]), g["level"], float(g["box"])
    tgas = 10 ** np.random.default_rng(11).uniform(3.5, 4.5, level.size)
    st.set_grid(n, level, box)
    st.set_rate_coefficients(*tab["grid"], tab["ka"])
    st.set_cooling_coefficients(th["cool"], th["compa"], _thermal.REDSHIFT)
    st.set_ground_recombination(tab["g"])
    st.set_medium(g["HI"], g["HeI"], g["HeII"], g["rho"], None, 0)
    st.set_temperature(tgas)
    # no point sources: the tracer deposits its rates with fp64 atomics, the one order-dependent sum of the library, and two runs of
    # it differ in the last bits; the background and the recombination source drive these steps
    kw = dict(sources=None, directions=rt_dirs(), beta=tab["beta"], uvb=UVB, ksi=tab["ksi"], substeps=2)
    thermal = dict(gamma=th["gamma"], tmin=10.0, tmax=1e8, hydro_heating=False)
    return kw, thermal, dict(n=n, level=level, box=box, rho=g["rho"])


def rt_dirs():
    import radiativetransfer_amd as rt
    return rt.healpix_directions(1)


def _by_hand(st, dt, nsteps, kw, thermal, coupled, share):
    """evolve's sequence of library calls, written out; share None: the sequence as it was before there was a recombination source"""
    import torch
    J = torch.empty((3, st.ncell), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream()
    for _ in range(nsteps):
        st.set_zero_rates()
        st.compute_opacities_from_medium(kw["beta"])
        if share is not None:
            st.recombination_source_device(kw["ksi"], share)
        st.transport_device(*kw["directions"], kw["uvb"], J.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        if share is not None:
            st.set_source_function(None)
        if coupled is not None:
            st.advance_thermochemistry_device(dt, J.data_ptr(), kw["ksi"], thermal["gamma"], use_point_rates=True, eta=coupled["eta"],
                                              max_subcycles=coupled["max_subcycles"], tmin=thermal["tmin"], tmax=thermal["tmax"], hydro_heating=False)
        else:
            st.advance_rate_equations_device(dt, J.data_ptr(), kw["ksi"], use_point_rates=True, substeps=kw["substeps"])
        st.hydrogen_mass()
    if share is not None:
        st.set_source_function(None)
    return J.cpu().numpy()


@pytest.mark.parametrize("mode", ["plain advance", "coupled", "recombination=None"])
def test_evolve(golden, tab, mode):
    """three steps against the same calls made by hand, bit for bit in medium, temperature and the last J; afterwards a plain sweep
    equals one on a fresh context; recombination=None is the sequence as it was: the same results and as many launch records"""
    import radiativetransfer_amd as rt
    share = None if mode == "recombination=None" else R.SPLIT
    coupled = dict(eta=0.1, max_subcycles=16) if mode == "coupled" else None
    dt, out = 3e12, []
    for driver in ("evolve", "by hand"):
        with rt.StellarTransfer() as st:
            kw, thermal, grid = _evolve_setup(st, golden, tab)
            if driver == "evolve":
                last = {}
                th = None if coupled is None else dict(thermal, coupled=coupled)
                rec = None if share is None else dict(share=share)
                rt.evolve(st, dt, 3, thermal=th, recombination=rec, on_step=lambda step, s, J: last.update(J=J.cpu().numpy()), **kw)
                J = last["J"]
            else:
                J = _by_hand(st, dt, 3, kw, thermal, coupled, share)
            records = len(st.launch_records())
            medium, tgas = st.medium(), st.temperature()
            st.compute_opacities_from_medium(kw["beta"])
            after = st.transport(*kw["directions"], kw["uvb"])
            out.append((J, medium, tgas, records, after))
            if driver == "evolve":
                with rt.StellarTransfer() as fresh:
                    fresh.set_grid(grid["n"], grid["level"], grid["box"])
                    fresh.set_medium(*medium, grid["rho"], None, 0)
                    fresh.compute_opacities_from_medium(kw["beta"])
                    _same(after, fresh.transport(*kw["directions"], kw["uvb"]), "a plain sweep after evolve")
    (J1, m1, t1, r1, a1), (J2, m2, t2, r2, a2) = out
    _same(J1, J2, "the last J")
    for a, b in zip(m1, m2):
        _same(a, b, "medium")
    _same(t1, t2, "temperature")
    _same(a1, a2, "the sweep afterwards")
    assert r1 == r2 and r1 > 0


def test_evolve_switches_emission_off_on_an_exception(golden, tab):
    import radiativetransfer_amd as rt
    with rt.StellarTransfer() as st:
        kw, thermal, grid = _evolve_setup(st, golden, tab)
        st.compute_opacities_from_medium(kw["beta"])
        plain = st.transport(*kw["directions"], kw["uvb"])

        def stop(step, s, J):
            raise RuntimeError("stop here")
        with pytest.raises(RuntimeError, match="stop here"):
            rt.evolve(st, 3e12, 2, recombination=dict(share=R.SPLIT), on_step=stop, **kw)
        medium = st.medium()
        st.set_medium(golden("expansion_refined")["HI"], golden("expansion_refined")["HeI"], golden("expansion_refined")["HeII"], grid["rho"], None, 0)
        st.compute_opacities_from_medium(kw["beta"])
        _same(st.transport(*kw["directions"], kw["uvb"]), plain, "a plain sweep after the exception")
        assert np.any(medium[0] != golden("expansion_refined")["HI"])
