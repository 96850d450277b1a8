"""Time-dependent ionisation on the GPU: ftte_advance_rate_equations* (advance_equations_kernel) through the C ABI against the host
evaluation of the same header (tests/_chem_advance.py: chem_advance_cell compiled by g++), bit for bit -- the step consists of IEEE
additions, multiplications and divisions, and the logarithm of the temperature is taken on the host -- and the driver
radiativetransfer_amd.evolve against the same loop through the oracle."""
import numpy as np
import pytest

import _chem_advance as A
import _oracle as O

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
STEPS = [(1e9, 1), (1e9, 3), (1e13, 1), (1e13, 3), (1e40, 1), (1e40, 3)]


@pytest.fixture(scope="module")
def stellar():
    import radiativetransfer_amd as rt
    st = rt.StellarTransfer()
    yield st
    st.close()


def _table(g):
    return float(g["logtem0"]), float(g["logtem9"]), float(g["dlogtem"]), g["k"]


def _load(st, g, tab):
    st.set_grid(int(g["n"]), g["level"], float(g["box"]))
    st.set_rate_coefficients(*_table(tab))
    st.set_medium(g["HI"], g["HeI"], g["HeII"], g["rho"], None, 0)
    st.set_temperature(g["tgas"])


def _same(st, change, ref):
    """the medium, the steps and the change of the last call against the host evaluation's"""
    HI, HeI, HeII = st.medium()
    assert ref[3] == 0
    bad = np.flatnonzero((HI != ref[0]) | (HeI != ref[1]) | (HeII != ref[2]))
    assert bad.size == 0, f"{bad.size} of {HI.size} cells differ, first {bad[:5]}: HI {HI[bad[:3]]} vs {ref[0][bad[:3]]}"
    assert st.rate_equation_steps() == int(ref[4].sum())
    assert change == ref[5].max()


@pytest.mark.parametrize("name,mode", [("chem_uvb_refined", "host J"), ("chem_uvb_refined", "device J + point rates"),
                                       ("chem_uniform_background", "uniform"), ("initial_refined", "uniform")])
def test_goldens_bitwise(stellar, golden, name, mode):
    import torch
    g, tab = golden(name), golden("chem_uvb_refined")
    st = stellar
    _load(st, g, tab)
    head = (int(g["n"]), g["level"], float(g["box"]), g["rho"], g["tgas"], g["HI"], g["HeI"], g["HeII"])
    if mode == "device J + point rates":
        rates = np.zeros((6, g["level"].size))
        rates[:3] = g["krate"]
        st.set_rates(rates)
        J = torch.from_numpy(np.ascontiguousarray(g["J"])).cuda()
        torch.cuda.synchronize()
    for dt, sub in STEPS:
        st.set_medium(g["HI"], g["HeI"], g["HeII"], g["rho"], None, 0)
        if mode == "host J":
            change = st.advance_rate_equations(dt, True, g["J"], g["ksi"], substeps=sub)
            ref = A.advance(*head, None, True, g["J"], g["ksi"], None, 0.0, *_table(tab), dt, sub)
        elif mode == "device J + point rates":
            change = st.advance_rate_equations_device(dt, J.data_ptr(), g["ksi"], use_point_rates=True, substeps=sub)
            ref = A.advance(*head, g["krate"], True, g["J"], g["ksi"], None, 0.0, *_table(tab), dt, sub)
        else:
            change = st.advance_rate_equations(dt, False, None, None, g["uniform"], float(g["threshold"]), substeps=sub)
            ref = A.advance(*head, None, False, None, None, g["uniform"], float(g["threshold"]), *_table(tab), dt, sub)
        _same(st, change, ref)


def test_wide_ranges_bitwise(golden):
    """a 32^3 random medium: densities over five decades, temperatures over the rate table's whole span, mean intensities over three
    decades, point-source rates in three cells of ten"""
    import radiativetransfer_amd as rt
    g = golden("chem_uvb_refined")
    n, box = 32, 2.5e23
    nc = n ** 3
    vol = (box / n) ** 3
    rng = np.random.default_rng(17)
    rho = 10 ** rng.uniform(-27.5, -22.5, nc)
    nh, nhe = A.PSI * rho / A.MH, (1 - A.PSI) * rho / A.MHE
    tgas = 10 ** rng.uniform(-0.5, 9.5, nc)
    J = 10 ** rng.uniform(-24.0, -21.0, (3, nc))
    start = (nh * 10 ** rng.uniform(-8, 0.1, nc), nhe * 10 ** rng.uniform(-8, 0.0, nc), nhe * 10 ** rng.uniform(-8, 0.0, nc))
    krate = np.zeros((6, nc))
    lit = rng.random(nc) < 0.3
    krate[0] = np.where(lit, 10 ** rng.uniform(-16, -11, nc) * vol * start[0], 0.0)
    krate[1] = np.where(lit, 10 ** rng.uniform(-17, -12, nc) * vol * start[2], 0.0)
    krate[2] = np.where(lit, 10 ** rng.uniform(-16, -11, nc) * vol * start[1], 0.0)
    level = np.zeros(nc, np.int32)
    with rt.StellarTransfer() as st:
        st.set_uniform_grid(n, box)
        st.set_rate_coefficients(*_table(g))
        st.set_medium(*start, rho, None, 0)
        st.set_temperature(tgas)
        st.set_rates(krate)
        for dt, sub in [(1e9, 1), (1e13, 3), (1e40, 1)]:
            st.set_medium(*start, rho, None, 0)
            change = st.advance_rate_equations(dt, True, J, g["ksi"], use_point_rates=True, substeps=sub)
            _same(st, change, A.advance(n, level, box, rho, tgas, *start, krate[:3], True, J, g["ksi"], None, 0.0, *_table(g), dt, sub))


def test_stride_loop(golden):
    """164^3 = 4 410 944 leaves, more than the 16 384 x 256 threads of a launch: the first, the last and 10^4 random cells"""
    import radiativetransfer_amd as rt
    g = golden("chem_uvb_refined")
    n, box = 164, 2.5e23
    nc = n ** 3
    assert nc > 16384 * 256
    rng = np.random.default_rng(3)
    rho = 3.0e-26 * np.exp(rng.normal(0.0, 0.8, nc))
    nh, nhe = A.PSI * rho / A.MH, (1 - A.PSI) * rho / A.MHE
    tgas = 10 ** rng.uniform(3.5, 5.0, nc)
    J = 10 ** rng.uniform(-23.5, -21.5, (3, nc))
    start = (0.5 * nh, 0.4 * nhe, 0.3 * nhe)
    dt, sub = 1e12, 2
    with rt.StellarTransfer() as st:
        st.set_uniform_grid(n, box)
        st.set_rate_coefficients(*_table(g))
        st.set_medium(*start, rho, None, 0)
        st.set_temperature(tgas)
        st.advance_rate_equations(dt, True, J, g["ksi"], substeps=sub)
        HI, HeI, HeII = st.medium()
    pick = np.unique(np.concatenate(([0, nc - 1], rng.choice(nc, 10000, replace=False))))
    ref = A.advance(n, np.zeros(pick.size, np.int32), box, rho[pick], tgas[pick], *[s[pick] for s in start], None, True, J[:, pick], g["ksi"], None,
                    0.0, *_table(g), dt, sub)
    assert ref[3] == 0
    assert np.array_equal(HI[pick], ref[0]) and np.array_equal(HeI[pick], ref[1]) and np.array_equal(HeII[pick], ref[2])
    assert np.all((HI >= 0) & (HI <= nh * (1 + A.SLACK)) & (HeI >= 0) & (HeII >= 0) & (HeI + HeII <= nhe * (1 + A.SLACK)))


def test_equilibrium_limit_on_the_device(stellar, golden):
    """a step of 1e40 s, twice, lands on the reference's start-up equilibrium in every one of the 405 cells (the bound:
    test_chem_advance_host.py (a))"""
    g, tab = golden("initial_refined"), golden("chem_uvb_refined")
    _load(stellar, g, tab)
    for _ in range(2):
        stellar.advance_rate_equations(1e40, False, None, None, g["uniform"], float(g["threshold"]))
    HI, HeI, HeII = stellar.medium()
    nh, nhe = A.PSI * g["rho"] / A.MH, (1 - A.PSI) * g["rho"] / A.MHE
    worst = max((np.abs(HI - g["HI_out"]) / nh).max(), (np.abs(HeI - g["HeI_out"]) / nhe).max(), (np.abs(HeII - g["HeII_out"]) / nhe).max())
    print(f"worst difference / element density {worst:.3e}")
    assert 16 * A.WORST_A <= A.CEILING and worst <= 16 * A.WORST_A


def test_closed_loop(stellar, golden):
    """Three steps of evolve() on the grid, sources, tables and directions of test_chem_gpu.py::test_closed_loop_on_the_device,
    against the same loop through the oracle's tracer, opacities and sweep and the host evaluation of the step fed the device's
    rates: J and the species bit for bit."""
    import radiativetransfer_amd as rt
    g = golden("chem_uvb_refined")
    tabs = golden("point16_homogeneous")["tables"]
    n, level, box = int(g["n"]), g["level"], float(g["box"])
    nc = level.size
    st = stellar
    _load(st, g, g)
    st.set_rate_tables(tabs)
    beta = np.array([[6.3e-18, 1.2e-18, 2.0e-19], [0.0, 7.4e-18, 1.5e-18], [0.0, 0.0, 1.6e-18]])  # [species][group]
    ang = np.array([rt.pix2ang_nest(1, i) for i in range(12)])
    phi, theta, w = ang[:, 0].copy(), ang[:, 1].copy(), np.full(12, 1.0 / 12)
    uvb = np.array([2e-22, 1e-22, 3e-23])
    src, ndot = np.array([5, nc // 2]), np.array([50.0, 20.0])
    dt, sub = 3e12, 2
    state = [g["HI"].copy(), g["HeI"].copy(), g["HeII"].copy()]
    seen = []

    def check(it, st, Jd):
        HI, HeI, HeII = state
        rates, _ = O.point_sources(n, level, HI, HeI, HeII, g["rho"], np.zeros(nc), box, 0, src, ndot, tabs.reshape(6, -1))
        kappa = O.compute_opacities(HI, HeI, HeII, beta)
        J = O.sweep_tree(n, level, kappa, box, phi, theta, w, uvb, arith=1)
        J = J[0] if isinstance(J, tuple) else J
        assert np.array_equal(Jd.cpu().numpy(), J), it
        dev_rates = st.rates()
        ref = A.advance(n, level, box, g["rho"], g["tgas"], HI, HeI, HeII, dev_rates[:3], True, J, g["ksi"], None, 0.0, *_table(g), dt, sub)
        assert ref[3] == 0
        m = st.medium()
        assert np.array_equal(m[0], ref[0]) and np.array_equal(m[1], ref[1]) and np.array_equal(m[2], ref[2]), it
        scale = np.abs(rates).max(axis=1, keepdims=True)
        assert np.all(np.abs(dev_rates - rates) <= 1e-9 * np.abs(rates) + 1e-13 * scale)
        state[:] = ref[:3]
        seen.append(it)

    times, neutral = rt.evolve(st, dt, 3, sources=(src, ndot), directions=(phi, theta, w), beta=beta, uvb=uvb, ksi=g["ksi"], substeps=sub,
                               on_step=check)
    assert seen == [0, 1, 2]
    assert np.array_equal(times, dt * np.arange(4))
    assert neutral.shape == (4,) and np.all((neutral > 0) & (neutral <= 1))
    mass = st.hydrogen_mass()
    assert neutral[-1] == mass[0] / mass[1]


def test_photon_budget(golden):
    """One star in the middle of a homogeneous 16^3 grid, no background, no collisional ionisation (k1 = 0): a step turns
    HI' = (HI + h k2 de nh) / (1 + h (G + k2 de)) >= HI / (1 + h G) with G = krate24 / (vol HI), so a cell loses no more neutral
    atoms than ionising photons were absorbed in it, vol (HI - HI') <= h krate24 -- in every cell and step; and HI stays in
    [0, nh]."""
    import radiativetransfer_amd as rt
    tabs = golden("point16_homogeneous")["tables"]
    ksi = golden("chem_uvb_refined")["ksi"]
    n, box = 16, 16e20
    nc = n ** 3
    vol = (box / n) ** 3
    rho = np.full(nc, 1e-3 * A.MH / A.PSI)
    nh, nhe = A.PSI * rho / A.MH, (1 - A.PSI) * rho / A.MHE
    k = np.zeros((6, 2))
    k[1] = 2.59e-13
    beta = np.array([[6.3e-18, 1.2e-18, 2.0e-19], [0.0, 7.4e-18, 1.5e-18], [0.0, 0.0, 1.6e-18]])
    ang = np.array([rt.pix2ang_nest(1, i) for i in range(12)])
    directions = (ang[:, 0].copy(), ang[:, 1].copy(), np.full(12, 1.0 / 12))
    centre = (n // 2) * (n * n + n + 1)
    dt = 1e10
    before = [nh.copy()]
    spent = []

    def check(it, st, Jd):
        assert not Jd.cpu().numpy().any()      # no background, no emission: the point source alone
        HI = st.medium()[0]
        krate24 = st.rates()[0]
        assert np.all((HI >= 0) & (HI <= nh))
        assert np.all(vol * (before[0] - HI) <= dt * krate24 * (1 + 8 * EPS))
        spent.append(float((vol * (before[0] - HI)).sum() / (dt * krate24.sum())))
        before[0] = HI

    with rt.StellarTransfer() as st:
        st.set_uniform_grid(n, box)
        st.set_rate_coefficients(0.0, 20.0, 20.0, k)
        st.set_medium(nh, nhe, np.zeros(nc), rho, None, 0)
        st.set_temperature(np.full(nc, 1e4))
        st.set_rate_tables(tabs)
        times, neutral = rt.evolve(st, dt, 5, sources=(np.array([centre]), np.array([1.0])), directions=directions, beta=beta, uvb=np.zeros(3),
                                   ksi=ksi, on_step=check)
    print("share of the absorbed photons that left an ion behind, per step:", spent, "neutral fraction:", neutral)
    assert len(spent) == 5 and all(0 < s <= 1 + 8 * EPS for s in spent)
    assert np.all(np.diff(neutral) < 0)      # the region grows


def _expect(status, fn, *args, **kw):
    from radiativetransfer_amd import FtteError
    with pytest.raises(FtteError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)
    return str(e.value)


def test_errors(stellar, golden):
    import radiativetransfer_amd as rt
    g = golden("chem_uvb_refined")
    st = stellar
    _load(st, g, g)
    # dt and substeps
    for dt in (0.0, -1.0, float("inf"), float("nan")):
        _expect("FTTE_ERR_ARG", st.advance_rate_equations, dt, True, g["J"], g["ksi"])
    for sub in (0, -1, 4097):
        _expect("FTTE_ERR_ARG", st.advance_rate_equations, 1e12, True, g["J"], g["ksi"], substeps=sub)
    _expect("FTTE_ERR_ARG", st.advance_rate_equations, 1e12, True, None, g["ksi"])
    _expect("FTTE_ERR_ARG", st.advance_rate_equations, 1e12, False, None, None, None)
    st.set_zero_rates()
    st.advance_rate_equations(1e12, True, g["J"], g["ksi"], use_point_rates=True, substeps=4096)
    # an empty cell: named, and the medium left as it was
    rho = g["rho"].copy()
    rho[7] = 0.0
    st.set_medium(g["HI"], g["HeI"], g["HeII"], rho, None, 0)
    assert A.advance(int(g["n"]), g["level"], float(g["box"]), rho, g["tgas"], g["HI"], g["HeI"], g["HeII"], None, True, g["J"], g["ksi"], None, 0.0,
                     *_table(g), 1e12, 1)[3] == 8
    text = _expect("FTTE_ERR_RATES", st.advance_rate_equations, 1e12, True, g["J"], g["ksi"])
    assert "cell 7 " in text and "ftte_advance_rate_equations" in text
    m = st.medium()
    assert np.array_equal(m[0], g["HI"]) and np.array_equal(m[1], g["HeI"]) and np.array_equal(m[2], g["HeII"])
    # call order, as for the equilibrium update
    with rt.StellarTransfer() as fresh:
        fresh.set_grid(2, np.zeros(8, np.int32), 1e22)
        z = np.full(8, 1e-6)
        fresh.set_medium(z, z, z, None, None, 0)
        for need in ("rate coefficients", "temperature", "density"):
            assert need in _expect("FTTE_ERR_STATE", fresh.advance_rate_equations, 1e12, False, None, None, np.zeros(3), 0.0)
            if need == "rate coefficients":
                fresh.set_rate_coefficients(*_table(g))
            elif need == "temperature":
                fresh.set_temperature(np.full(8, 1e4))
        fresh.set_medium(z, z * 0.05, z * 0.01, np.full(8, 3e-24), None, 0)
        assert "point-source rates" in _expect("FTTE_ERR_STATE", fresh.advance_rate_equations, 1e12, False, None, None, np.zeros(3), 0.0,
                                               use_point_rates=True)
        fresh.advance_rate_equations(1e12, False, None, None, np.zeros(3), 0.0)


def test_multi_device_context_refuses(golden):
    import radiativetransfer_amd as rt
    g = golden("chem_uvb_refined")
    with rt.StellarTransfer(devices=[0, 0]) as st:
        st.set_grid(int(g["n"]), g["level"], float(g["box"]))
        _expect("FTTE_ERR_UNSUPPORTED", st.advance_rate_equations, 1e12, True, g["J"], g["ksi"])
        _expect("FTTE_ERR_UNSUPPORTED", st.advance_rate_equations_device, 1e12, 0, g["ksi"])


def test_fortran_host_evolves(golden, tmp_path):
    """fortran/ftte_demo_evolve: three steps of the loop with the advance in place of the equilibrium, from a Fortran host, against
    evolve() on the same case: the same calls in the same order, so the same species, times and neutral fractions"""
    import os
    import subprocess
    import radiativetransfer_amd as rt
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "fortran", "ftte_demo_evolve")
    if not os.path.exists(exe):
        pytest.skip("fortran/ftte_demo_evolve not built (no Fortran compiler at build time)")
    g = golden("chem_uvb_refined")
    tabs = golden("point16_homogeneous")["tables"]
    n, level, box = int(g["n"]), g["level"], float(g["box"])
    nc = level.size
    alpha = np.array([1.8, 1.5, 1.2])
    uvb = np.array([2e-22, 1e-22, 3e-23])
    src, ndot = np.array([5, nc // 2], np.int64), np.array([50.0, 20.0])
    nsteps, L, dt, sub = 3, 2, 3e12, 2
    case, out = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(case, "wb") as f:      # the case file of fortran/ftte_demo_loop
        f.write(np.array([n, nc, src.size, nsteps, L, g["k"].shape[1]], "<i4").tobytes())
        f.write(np.concatenate([[box], alpha, uvb]).astype("<f8").tobytes())
        f.write(level.astype("<i4").tobytes())
        for name in ("rho", "tgas", "HI", "HeI", "HeII"):
            f.write(g[name].astype("<f8").tobytes())
        f.write(src.astype("<i8").tobytes())
        f.write(ndot.astype("<f8").tobytes())
        f.write(tabs.astype("<f8").tobytes())
        f.write(np.array([float(g["logtem0"]), float(g["logtem9"]), float(g["dlogtem"])], "<f8").tobytes())
        f.write(np.ascontiguousarray(g["k"], "<f8").tobytes())      # k(nratec,6) in Fortran order == [6][nratec]
    res = subprocess.run([exe, str(case), str(out), repr(dt), str(sub)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "ftte_demo_evolve OK" in res.stdout, res.stdout + res.stderr
    raw = np.fromfile(out, "<f8")
    species, rest = raw[:3 * nc].reshape(3, nc), raw[6 * nc:]
    times, neutral = rest[:nsteps + 1], rest[nsteps + 1:]
    beta, ksi, _ = rt.uvb_beta_table(alpha)
    phi, theta, _ = rt.healpix_directions(L)
    w = np.full(phi.size, float(np.float32(1.0) / np.float32(phi.size)))
    with rt.StellarTransfer() as st:
        _load(st, g, g)
        st.set_medium(g["HI"], g["HeI"], g["HeII"], g["rho"], g["rho"], 0)
        st.set_rate_tables(tabs)
        t, frac = rt.evolve(st, dt, nsteps, sources=(src, ndot), directions=(phi, theta, w), beta=beta, uvb=uvb, ksi=ksi, substeps=sub)
        mine = st.medium()
    assert np.array_equal(times, t)
    assert np.all(np.abs(neutral - frac) <= 1e-12 * frac)
    for a, b in zip(species, mine):
        assert np.all(np.abs(a - b) <= 1e-8 * np.abs(b) + 1e-30)
