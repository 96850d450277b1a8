"""The coupled step on the GPU: ftte_advance_thermochemistry* and ftte_get_subcycles (thermochem_advance_kernel) through the C ABI
against the host evaluation of the same header (tests/_thermochem.py: ftte_thermochem_math.h compiled by g++), bit for bit -- the
statement consists of IEEE additions, multiplications, divisions, fmin, fmax, fabs and explicit fused multiply-adds, its logarithm
included -- its refusals, the hand-over of the new logarithm to the chemistry, and radiativetransfer_amd.evolve(thermal=dict(...,
coupled=...)) against the same loop through the oracle and the host statement."""
import numpy as np
import pytest

import _chem_advance as A
import _oracle as O
import _thermal as T
import _thermochem as TC

pytestmark = pytest.mark.gpu


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


def _rates(case, tab):
    """the rate arguments of advance_thermochemistry for a case"""
    return dict(run_uvb=case["run_uvb"], J=case["J"], ksi=case["ksi"], gamma=tab["gamma"], uniform=case["uniform"], uniform_gamma=tab["uniform_gamma"],
                threshold=case["threshold"], use_point_rates=case["rates"] is not None)


def _same_arrays(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} cells differ, first {bad[:5]}: {got[bad[:3]]} vs {want[bad[:3]]}"


def _same(st, out, ref, what):
    """everything a call reports against the host evaluation `ref`"""
    assert ref["status"] == 0, what
    for got, s in zip(st.medium(), ("HI", "HeI", "HeII")):
        _same_arrays(got, ref[s], f"{what}: {s}")
    _same_arrays(st.temperature(), ref["T"], f"{what}: T")
    _same_arrays(st.subcycles(), ref["subcycles"], f"{what}: subcycles per leaf")
    sub = ref["subcycles"].astype(np.int64)
    assert (out["subcycles"], out["largest"], out["capped"]) == (int(sub.sum()), int(sub.max()), int(ref["capped"].sum())), what
    assert out["species_change"] == ref["change"].max() and out["temperature_change"] == ref["tchange"].max(), what
    assert st.rate_equation_steps() == int(ref["steps"].sum()) and ref["steps"].sum() > 0, what


def _same_logtem(st, case, chem, tab, ref, what):
    """the logarithm the call left on the device, read the only way a host can: the existing pair over h after it, against the host's
    pair at ref's logarithm"""
    h = 1e12
    state = (ref["T"], ref["HI"], ref["HeI"], ref["HeII"])
    want = TC.pair(case, tab, chem, h, logtem=ref["logtem"], state=state)
    assert want[5] == 0
    r = _rates(case, tab)
    st.advance_rate_equations(h, r["run_uvb"], r["J"], r["ksi"], r["uniform"], r["threshold"], r["use_point_rates"])
    st.advance_temperature(h, r["run_uvb"], r["J"], r["gamma"], r["uniform_gamma"], r["threshold"], r["use_point_rates"])
    for got, w, s in zip((*st.medium(), st.temperature()), want[:4], ("HI", "HeI", "HeII", "T")):
        _same_arrays(got, w, f"{what}: {s} after the pair that read the new logarithm")
    # (and it was the new one: at the stored logarithm of the start the chemistry comes out differently)
    old = TC.pair(case, tab, chem, h, logtem=T.libm_log(case["head"][4]), state=state)
    assert not np.array_equal(old[0], want[0])


@pytest.mark.parametrize("name", ["initial_refined", "chem_uniform_background", "chem_uvb_refined"])
def test_bitwise_on_the_goldens(stellar, golden, chem, grid, name):
    """the goldens (405 leaves on two levels, 512 for the uniform background: no multiple of 64 among the refined ones) in every rate mode
    they have, over a short, a front-crossing, a uniform and an equilibrium-length schedule"""
    tab = T.tables()
    for case in TC.modes(TC.case(golden, name, grid)):
        _load(stellar, case, chem)
        HI, HeI, HeII, rho = *case["head"][5:], case["head"][3]
        for dt, eta, cap in TC.RUNS:
            stellar.set_medium(HI, HeI, HeII, rho, None, 0)
            stellar.set_temperature(case["head"][4])
            if case["rates"] is not None:
                stellar.set_rates(case["rates"])
            ref = TC.advance(case, tab, chem, dt, eta, cap)
            out = stellar.advance_thermochemistry(dt, eta=eta, max_subcycles=cap, **_rates(case, tab))
            _same(stellar, out, ref, f"{name} rates {case['rates'] is not None} dt {dt:g} eta {eta} cap {cap}")
        _same_logtem(stellar, case, chem, tab, ref, name)


@pytest.mark.parametrize("name", ["wide", "wide_uniform"])
def test_bitwise_where_lanes_diverge(stellar, golden, chem, grid, name):
    """the 32^3 wide media: leaves of 1 and of `cap` subcycles share wavefronts (checked: both occur within one aligned group of 64
    consecutive leaves)"""
    tab, case = T.tables(), TC.case(golden, name, grid)
    dt, eta, cap = 1e11, 0.1, 8
    ref = TC.advance(case, tab, chem, dt, eta, cap)
    groups = ref["subcycles"].reshape(-1, 64)
    both = (groups == 1).any(axis=1) & (groups == cap).any(axis=1)
    print(f"{name}: {both.sum()} of {both.size} groups of 64 hold leaves of 1 and of {cap} subcycles; subcycles {np.bincount(ref['subcycles'])}")
    assert both.any()
    _load(stellar, case, chem)
    out = stellar.advance_thermochemistry(dt, eta=eta, max_subcycles=cap, **_rates(case, tab))
    _same(stellar, out, ref, name)


def test_stride_loop(chem, grid):
    """164^3 = 4 410 944 leaves, more than the 16 384 x 256 threads of a launch, cap = 4: the first, the last and 10^4 random cells, and
    the counters over all of them against the per-leaf map"""
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
    dt, eta, cap = 1e12, 0.1, 4
    with rt.StellarTransfer() as st:
        st.set_uniform_grid(n, box)
        st.set_rate_coefficients(*grid, chem["k"])
        st.set_cooling_coefficients(tab["cool"], tab["compa"], T.REDSHIFT)
        st.set_medium(*start, rho, None, 0)
        st.set_temperature(tgas)
        out = st.advance_thermochemistry(dt, True, J, chem["ksi"], tab["gamma"], eta=eta, max_subcycles=cap)
        m, T1, sub = st.medium(), st.temperature(), st.subcycles()
    pick = np.unique(np.concatenate(([0, nc - 1], rng.choice(nc, 10000, replace=False))))
    case = dict(head=(n, np.zeros(pick.size, np.int32), box, rho[pick], tgas[pick], *[s[pick] for s in start]), rates=None, run_uvb=True, J=J[:, pick],
                threshold=0.0, grid=grid, ksi=chem["ksi"], uniform=None)
    ref = TC.advance(case, tab, chem, dt, eta, cap)
    assert ref["status"] == 0
    for got, s in zip((*m, T1, sub), ("HI", "HeI", "HeII", "T", "subcycles")):
        assert np.array_equal(got[pick], ref[s]), s
    assert sub.min() >= 1 and sub.max() <= cap
    assert (out["subcycles"], out["largest"]) == (int(sub.astype(np.int64).sum()), int(sub.max()))
    # (a leaf may take `cap` subcycles of its own choosing, the last being what remained: the flag counts only those the even split bounded)
    assert np.count_nonzero(ref["capped"]) * (nc // pick.size) // 2 <= out["capped"] <= nc
    assert np.all((T1 >= T.TMIN) & (T1 <= T.TMAX)) and np.all((m[0] >= 0) & (m[0] <= nh * (1 + A.SLACK)))


def test_hand_over_to_the_chemistry(stellar, golden, chem, grid):
    """after the coupled call ftte_advance_rate_equations_device reads the new logarithm"""
    import torch
    tab, case = T.tables(), TC.without_rates(TC.case(golden, "chem_uvb_refined", grid))
    _load(stellar, case, chem)
    ref = TC.advance(case, tab, chem, 1e13, 0.1, 32)
    stellar.advance_thermochemistry(1e13, eta=0.1, max_subcycles=32, **_rates(case, tab))
    assert np.array_equal(stellar.temperature(), ref["T"]) and np.any(ref["T"] != case["head"][4])
    J = torch.from_numpy(np.ascontiguousarray(case["J"])).cuda()
    torch.cuda.synchronize()
    stellar.advance_rate_equations_device(1e12, J.data_ptr(), case["ksi"])
    n, level, box, rho = case["head"][:4]
    args = (None, True, case["J"], case["ksi"], None, 0.0, *grid, chem["k"], 1e12, 1)
    want = TC.pair(case, tab, chem, 1e12, logtem=ref["logtem"], state=(ref["T"], ref["HI"], ref["HeI"], ref["HeII"]))
    for got, w in zip(stellar.medium(), want[:3]):
        _same_arrays(got, w, "species after the hand-over")
    today = A.advance(n, level, box, rho, ref["T"], ref["HI"], ref["HeI"], ref["HeII"], *args)      # (at libm's logarithm of the new T)
    stale = A.advance(n, level, box, rho, case["head"][4], ref["HI"], ref["HeI"], ref["HeII"], *args)      # (at the old temperature)
    assert today[3] == 0 and not np.array_equal(stale[0], want[0])


def _expect(status, fn, *args, **kw):
    from radiativetransfer_amd import FtteError
    with pytest.raises(FtteError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)
    return str(e.value)


def test_refusals(golden, chem, grid):
    import radiativetransfer_amd as rt
    tab, case = T.tables(), TC.case(golden, "chem_uvb_refined", grid)
    n, level, box, rho, tgas, HI, HeI, HeII = case["head"]
    r = _rates(case, tab)
    call = lambda st, **kw: st.advance_thermochemistry(kw.pop("dt", 1e12), **{**r, **kw})      # noqa: E731
    with rt.StellarTransfer() as st:
        st.set_grid(n, level, box)
        st.set_medium(HI, HeI, HeII, rho, None, 0)
        assert "rate coefficients" in _expect("FTTE_ERR_STATE", call, st)
        st.set_rate_coefficients(*grid, chem["k"])
        assert "cooling coefficients" in _expect("FTTE_ERR_STATE", call, st)
        st.set_cooling_coefficients(tab["cool"], tab["compa"], T.REDSHIFT)
        assert "temperature" in _expect("FTTE_ERR_STATE", call, st)
        st.set_temperature(tgas)
        assert "point-source rates" in _expect("FTTE_ERR_STATE", call, st)
        st.set_rates(case["rates"])
        assert "ftte_advance_thermochemistry" in _expect("FTTE_ERR_STATE", st.subcycles)      # before any coupled call on this grid
        assert "hydroHeating" in _expect("FTTE_ERR_STATE", call, st, hydro_heating=True)
        for dt in (0.0, -1.0, float("inf"), float("nan")):
            _expect("FTTE_ERR_ARG", call, st, dt=dt)
        for eta in (-0.1, float("inf"), float("nan")):
            _expect("FTTE_ERR_ARG", call, st, eta=eta)
        for cap in (0, -1, 4097):
            _expect("FTTE_ERR_ARG", call, st, max_subcycles=cap)
        for tmin, tmax in ((0.0, 1e9), (-1.0, 1e9), (10.0, 10.0), (10.0, 1.0), (1.0, float("inf")), (float("nan"), 1e9)):
            _expect("FTTE_ERR_ARG", call, st, tmin=tmin, tmax=tmax)
        for missing in ("J", "ksi", "gamma"):
            _expect("FTTE_ERR_ARG", call, st, **{missing: None})
        _expect("FTTE_ERR_ARG", call, st, run_uvb=False, uniform=None, uniform_gamma=np.zeros(3))
        _expect("FTTE_ERR_ARG", call, st, run_uvb=False, uniform=np.zeros(3), uniform_gamma=None)
        assert "ftte_advance_thermochemistry" in _expect("FTTE_ERR_STATE", st.subcycles)      # no refused call has made a map
        st.thermal_equilibrium(r["run_uvb"], r["J"], r["gamma"], None, 0.0, True)
        call(st, hydro_heating=True, eta=0.0, max_subcycles=2)
        assert np.all(st.subcycles() == 2)
        # one NaN temperature: the leaf is named, and medium, temperature, logarithm and the subcycle map are left as they were
        st.set_medium(HI, HeI, HeII, rho, None, 0)
        bad = tgas.copy()
        bad[7] = np.nan
        st.set_temperature(bad)
        assert TC.advance(dict(case, head=(n, level, box, rho, bad, HI, HeI, HeII)), tab, chem, 1e12, 0.1, 16, logtem=T.libm_log(tgas))["status"] == 8
        text = _expect("FTTE_ERR_RATES", call, st, max_subcycles=16)
        assert "cell 7 " in text and "ftte_advance_thermochemistry" in text
        now = st.temperature()
        assert np.isnan(now[7]) and np.array_equal(np.delete(now, 7), np.delete(tgas, 7))
        assert all(np.array_equal(a, b) for a, b in zip(st.medium(), (HI, HeI, HeII))) and np.all(st.subcycles() == 2)
        st.solve_rate_equations(True, case["J"], case["ksi"])      # the logarithm too: the equilibrium update from the same state
        with rt.StellarTransfer() as other:
            _load(other, dict(case, head=(n, level, box, rho, bad, HI, HeI, HeII)), chem)
            other.solve_rate_equations(True, case["J"], case["ksi"])
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(st.medium(), other.medium()))
        # an empty leaf
        st.set_temperature(tgas)
        empty = rho.copy()
        empty[3] = 0.0
        st.set_medium(HI, HeI, HeII, empty, None, 0)
        assert "cell 3 " in _expect("FTTE_ERR_RATES", call, st)
        assert np.array_equal(st.temperature(), tgas) and np.all(st.subcycles() == 2)
        # another grid: the map belongs to the old one
        st.set_grid(2, np.zeros(8, np.int32), 1e22)
        z = np.full(8, 1e-6)
        st.set_medium(z, z * 0.05, z * 0.01, np.full(8, 3e-24), None, 0)
        st.set_temperature(np.full(8, 1e4))
        _expect("FTTE_ERR_STATE", st.subcycles)
        out = st.advance_thermochemistry(1e12, False, None, None, None, np.zeros(3), np.zeros(3), 0.0)
        assert st.subcycles().shape == (8,) and out["subcycles"] == int(st.subcycles().sum())


def test_two_bad_leaves_the_lower_one_is_named(golden, chem, grid):
    """The fold's minimum across wavefronts and workgroups, for each of the six per-leaf kernels through its entry point: on the 405
    leaves of chem_uvb_refined (two workgroups, the last wavefront partly filled) leaf 300, in the second workgroup, and leaf 130, in
    the third wavefront of the first, are bad at once -- a NaN temperature for the thermal kernels and the coupled one; for the
    chemistry's an empty leaf, as in their own refusal tests: their statements clip a NaN species into range and do not refuse it.
    The refusal names leaf 130, and medium, temperature and subcycle map are left as they were."""
    import radiativetransfer_amd as rt
    tab, case = T.tables(), TC.case(golden, "chem_uvb_refined", grid)
    n, level, box, rho, tgas, HI, HeI, HeII = case["head"]
    assert level.size == 405
    r = _rates(case, tab)
    both = [300, 130]
    nan_t, empty = tgas.copy(), rho.copy()
    nan_t[both], empty[both] = np.nan, 0.0
    chemistry = (r["run_uvb"], r["J"], r["ksi"], None, r["threshold"], True)
    heating = (r["run_uvb"], r["J"], r["gamma"], None, r["threshold"], True)
    calls = [("rate_equations_kernel", empty, tgas, lambda st: st.solve_rate_equations(*chemistry)),
             ("advance_equations_kernel", empty, tgas, lambda st: st.advance_rate_equations(1e12, *chemistry)),
             ("initial_equilibrium_kernel", empty, tgas, lambda st: st.initial_ionization_equilibrium(golden("initial_refined")["uniform"], 0.0)),
             ("thermal_equilibrium_kernel", rho, nan_t, lambda st: st.thermal_equilibrium(*heating)),
             ("thermal_advance_kernel", rho, nan_t, lambda st: st.advance_temperature(1e12, *heating)),
             ("thermochem_advance_kernel", rho, nan_t, lambda st: st.advance_thermochemistry(1e12, **r))]
    with rt.StellarTransfer() as st:
        _load(st, case, chem)
        st.advance_thermochemistry(1e12, eta=0.0, max_subcycles=2, **r)      # a subcycle map to leave alone
        for kernel, rho_, tgas_, call in calls:
            st.set_medium(HI, HeI, HeII, rho_, None, 0)
            st.set_temperature(tgas_)
            text = _expect("FTTE_ERR_RATES", call, st)
            assert "cell 130 " in text, (kernel, text)
            assert all(np.array_equal(a, b) for a, b in zip(st.medium(), (HI, HeI, HeII))), kernel
            assert np.array_equal(st.temperature(), tgas_, equal_nan=True) and np.all(st.subcycles() == 2), kernel


def test_device_objects_come_back(stellar, golden, chem, grid):
    import radiativetransfer_amd as rt
    tab, case = T.tables(), TC.case(golden, "chem_uvb_refined", grid)
    before = stellar.counter("device_objects")
    with rt.StellarTransfer() as st:
        _load(st, case, chem)
        st.advance_thermochemistry(1e12, **_rates(case, tab))
        st.subcycles()
        assert st.counter("device_objects") > before
    assert stellar.counter("device_objects") == before


def test_multi_device_context_refuses(golden, chem, grid):
    import radiativetransfer_amd as rt
    tab, case = T.tables(), TC.case(golden, "chem_uvb_refined", grid)
    with rt.StellarTransfer(devices=[0, 0]) as st:
        st.set_grid(*[case["head"][i] for i in (0, 1, 2)])
        _expect("FTTE_ERR_UNSUPPORTED", st.advance_thermochemistry, 1e12, True, case["J"], case["ksi"], tab["gamma"])
        _expect("FTTE_ERR_UNSUPPORTED", st.advance_thermochemistry_device, 1e12, 0, case["ksi"], tab["gamma"])
        _expect("FTTE_ERR_UNSUPPORTED", st.subcycles)


def test_evolve_coupled(golden, chem, grid):
    """Three steps of evolve(thermal=dict(..., coupled=dict(eta=0.1, max_subcycles=32))) against the same loop through the oracle's
    tracer, opacities and sweep and the host statement fed the device's rates (as test_chem_advance_gpu.py::test_closed_loop does for
    the chemistry alone): J, the species and T bit for bit, the logarithm handed from step to step."""
    import radiativetransfer_amd as rt
    g, tab = chem, T.tables()
    tabs = golden("point16_homogeneous")["tables"]
    n, level, box = int(g["n"]), g["level"], float(g["box"])
    nc = level.size
    beta = np.array([[6.3e-18, 1.2e-18, 2.0e-19], [0.0, 7.4e-18, 1.5e-18], [0.0, 0.0, 1.6e-18]])      # [species][group]
    ang = np.array([rt.pix2ang_nest(1, i) for i in range(12)])
    phi, theta, w = ang[:, 0].copy(), ang[:, 1].copy(), np.full(12, 1.0 / 12)
    uvb = np.array([2e-22, 1e-22, 3e-23])
    src, ndot = np.array([5, nc // 2]), np.array([50.0, 20.0])
    dt, eta, cap = 3e12, 0.1, 32
    thermal = dict(gamma=tab["gamma"], tmin=10.0, tmax=1e8, hydro_heating=False, coupled=dict(eta=eta, max_subcycles=cap))
    state = dict(HI=g["HI"].copy(), HeI=g["HeI"].copy(), HeII=g["HeII"].copy(), T=g["tgas"].copy(), logtem=T.libm_log(g["tgas"]))
    seen = []

    def check(it, st, Jd):
        HI, HeI, HeII = state["HI"], state["HeI"], state["HeII"]
        kappa = O.compute_opacities(HI, HeI, HeII, beta)
        J = O.sweep_tree(n, level, kappa, box, phi, theta, w, uvb, arith=1)
        J = J[0] if isinstance(J, tuple) else J
        assert np.array_equal(Jd.cpu().numpy(), J), it
        case = dict(head=(n, level, box, g["rho"], state["T"], HI, HeI, HeII), rates=st.rates(), run_uvb=True, J=J, threshold=0.0, grid=grid,
                    ksi=g["ksi"], uniform=None)
        ref = TC.advance(case, tab, chem, dt, eta, cap, tmin=10.0, tmax=1e8, logtem=state["logtem"])
        assert ref["status"] == 0
        for got, s in zip((*st.medium(), st.temperature(), st.subcycles()), ("HI", "HeI", "HeII", "T", "subcycles")):
            _same_arrays(got, ref[s], f"step {it}: {s}")
        for s in state:
            state[s] = ref[s]
        seen.append((it, int(ref["subcycles"].max())))

    with rt.StellarTransfer() as st:
        st.set_grid(n, level, box)
        st.set_rate_coefficients(*grid, g["k"])
        st.set_cooling_coefficients(tab["cool"], tab["compa"], T.REDSHIFT)
        st.set_medium(g["HI"], g["HeI"], g["HeII"], g["rho"], None, 0)
        st.set_temperature(g["tgas"])
        st.set_rate_tables(tabs)
        times, neutral = rt.evolve(st, dt, 3, sources=(src, ndot), directions=(phi, theta, w), beta=beta, uvb=uvb, ksi=g["ksi"], thermal=thermal,
                                   on_step=check)
    print(f"steps and their largest subcycle counts: {seen}")
    assert [s[0] for s in seen] == [0, 1, 2] and max(s[1] for s in seen) > 1
    assert np.array_equal(times, dt * np.arange(4)) and np.all((neutral > 0) & (neutral <= 1))
