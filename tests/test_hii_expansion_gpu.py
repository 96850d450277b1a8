"""The start-up expansion of HII regions on the GPU (equiSources.f90:1035-1069: findExpansion for every star and leaf, then
applyExpansion): ftte_expand_hii_regions against the reference's own compiled routines (tests/golden/expansion_*.npz,
make_golden_expansion.py) and against the numpy restatement of tests/_hii_expansion.py, rho, HI, HeI, HeII and rhoCoef bit for
bit; the workgroup cull counted; the tracer's packed copy and the opacities after an expansion; the refusals; the Fortran host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _hii_expansion as X
import radiativetransfer_amd as rt

pytestmark = pytest.mark.gpu

GOLDENS = ["expansion_refined", "expansion_uniform16", "expansion_ingested"]
FIELDS = ("rho", "HI", "HeI", "HeII")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stellar():
    st = rt.StellarTransfer()
    yield st
    st.close()


@pytest.fixture(scope="module")
def host_parameters(golden):
    """per golden: ftte_expansion_parameters' own [nsrc][3] and where it equals the reference's bit for bit"""
    out = {}
    for name in GOLDENS:
        g = golden(name)
        own = X.parameters_of(g["rho"], g["src_cell"], rt.expansion_parameters)
        out[name] = (own, bool(np.array_equal(own, g["params"])))
    return out


def _load(st, g, rho=None, abun2=None, dust=0):
    st.set_grid(int(g["n"]), g["level"], float(g["box"]))
    st.set_medium(g["HI"], g["HeI"], g["HeII"], g["rho"] if rho is None else rho, abun2, dust)


def _state(st):
    return [st.density(), *st.medium()]


def _same(got, want):
    """bit for bit (a NaN equals itself)"""
    return all(np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))
               for a, b in zip(got, want))


def _restated(g, src, params, rho=None):
    rho = g["rho"] if rho is None else rho
    coef = X.rho_coef(int(g["n"]), g["level"], float(g["box"]), rho, src, params)
    return coef, X.apply_expansion(coef, rho, g["HI"], g["HeI"], g["HeII"])


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_bitwise_with_the_reference_parameters(stellar, golden, name):
    g = golden(name)
    runs = []
    for _ in range(2):
        _load(stellar, g)
        coef, changed = stellar.expand_hii_regions(g["src_cell"], g["params"])
        state = _state(stellar)
        assert np.array_equal(coef, g["rho_coef"])
        for got, key in zip(state, FIELDS):
            assert np.array_equal(got, g[key + "_out"]), key
        assert changed == int((g["rho_coef"] < 1).sum())
        assert 0 < stellar.counter("expansion_exact_tests") <= g["src_cell"].size * g["level"].size
        runs.append([coef, *state, stellar.counter("expansion_exact_tests")])
    assert _same(runs[0][:5], runs[1][:5]) and runs[0][5] == runs[1][5]     # the same bits, run after run


@pytest.mark.parametrize("name", GOLDENS)
def test_parameters_from_the_host_leaves(stellar, golden, host_parameters, name):
    """params = NULL: the densities gathered on the device, the parameters and the centres made on the host"""
    g = golden(name)
    own, identical = host_parameters[name]
    _load(stellar, g)
    coef, changed = stellar.expand_hii_regions(g["src_cell"])
    state = _state(stellar)
    _load(stellar, g)
    coef2, changed2 = stellar.expand_hii_regions(g["src_cell"], own)
    assert np.array_equal(coef, coef2) and changed == changed2 and _same(state, _state(stellar))
    if identical:
        assert np.array_equal(coef, g["rho_coef"]) and _same(state, [g[k + "_out"] for k in FIELDS])
    else:
        want_coef, want = _restated(g, g["src_cell"], own)
        assert np.array_equal(coef, want_coef) and _same(state, want)


def test_temperature_and_abundance_are_not_touched(stellar, golden):
    """abun2 through the tracer's dust term (dust approximation 2 reads rho and abun2), tgas through an equilibrium update: after
    the expansion both calls give what a fresh context gives that was handed the expanded fields and the same abun2 and tgas"""
    g, chem = golden("expansion_refined"), golden("chem_uvb_refined")
    tables = golden("point16_homogeneous")["tables"]
    rng = np.random.default_rng(3)
    abun2 = rng.uniform(0.005, 0.05, g["level"].size)
    tgas = 10 ** rng.uniform(3.5, 4.5, g["level"].size)
    uniform = np.array([3e-14, 1e-16, 2e-14])
    src, ndot = g["src_cell"][:2], np.array([50.0, 20.0])

    def prepare(st):
        st.set_rate_coefficients(float(chem["logtem0"]), float(chem["logtem9"]), float(chem["dlogtem"]), chem["k"])
        st.set_temperature(tgas)
        st.set_rate_tables(tables)

    def finish(st):
        st.set_zero_rates()
        st.point_sources(src, ndot)
        rates = st.rates()
        st.solve_rate_equations(False, uniform=uniform, threshold=0.0)
        return rates, st.medium()

    with rt.StellarTransfer() as A:
        _load(A, g, abun2=abun2, dust=2)
        prepare(A)
        A.expand_hii_regions(g["src_cell"], g["params"])
        rates_a, species_a = finish(A)
    with rt.StellarTransfer() as B:
        B.set_grid(int(g["n"]), g["level"], float(g["box"]))
        B.set_medium(g["HI_out"], g["HeI_out"], g["HeII_out"], g["rho_out"], abun2, 2)
        prepare(B)
        rates_b, species_b = finish(B)
    assert _same(species_a, species_b)
    scale = np.abs(rates_b).max(axis=1, keepdims=True)
    assert np.all(np.abs(rates_a - rates_b) <= 1e-9 * np.abs(rates_b) + 1e-13 * scale)


def test_no_stars(stellar, golden):
    g = golden("expansion_uniform16")
    _load(stellar, g)
    coef, changed = stellar.expand_hii_regions(np.zeros(0, np.int64))
    assert changed == 0 and np.array_equal(coef, np.ones(g["level"].size))
    assert _same(_state(stellar), [g[k] for k in FIELDS]) and stellar.counter("expansion_exact_tests") == 0


def test_a_sphere_that_holds_the_whole_box(stellar, golden):
    g = golden("expansion_refined")
    nh = X.PSI * g["rho"] / X.MH
    nh_src = float(np.median(nh))
    params = np.array([[10.0 * float(g["box"]), 0.25, nh_src]])
    _load(stellar, g)
    coef, changed = stellar.expand_hii_regions(g["src_cell"][:1], params)
    lower = nh <= X.MARGIN * nh_src
    assert lower.any() and not lower.all()
    assert np.array_equal(coef, np.where(lower, 0.25, 1.0)) and changed == int(lower.sum())
    assert _same(_state(stellar), X.apply_expansion(coef, *[g[k] for k in FIELDS]))
    assert stellar.counter("expansion_exact_tests") == g["level"].size      # nothing can be ruled out


def test_a_star_in_very_thin_gas_changes_nothing(stellar, golden):
    """nh < 1e-6: the density coefficient comes out above 1, and min(rhoCoef, coefficient) stays 1 inside a radius of megaparsecs"""
    g = golden("expansion_uniform16")
    cell = 1234
    rho = g["rho"].copy()
    rho[cell] = 1e-7 * X.MH / X.PSI
    radius, dcoef = rt.expansion_parameters(X.PSI * rho[cell] / X.MH)
    assert dcoef > 1.0 and radius > float(g["box"])
    _load(stellar, g, rho=rho)
    coef, changed = stellar.expand_hii_regions([cell])
    assert changed == 0 and np.array_equal(coef, np.ones(rho.size))
    assert _same(_state(stellar), [rho, g["HI"], g["HeI"], g["HeII"]])


def test_workgroups_rule_out_far_stars(stellar, golden):
    """16^3 uniform, 40 stars whose spheres are under one cell wide.  The centres of up to 1024 consecutive leaves lie in at most
    four i-planes and such a sphere reaches one plane, so whatever the group size up to 1024, a star survives the cull in at most
    a quarter of the groups: exact tests <= nsrc ncell / 4.  The results stay the restatement's bit for bit."""
    g = golden("expansion_uniform16")
    n, box, src = int(g["n"]), float(g["box"]), g["src_cell"]
    nh = X.PSI * g["rho"] / X.MH
    params = np.column_stack([np.full(src.size, 0.45 * box / n), np.linspace(0.1, 0.9, src.size), 2.0 * nh[src]])
    want_coef, want = _restated(g, src, params)
    assert (want_coef < 1).sum() == np.unique(src).size                       # each star its own cell and nothing else
    _load(stellar, g)
    coef, changed = stellar.expand_hii_regions(src, params)
    assert np.array_equal(coef, want_coef) and changed == int((want_coef < 1).sum()) and _same(_state(stellar), want)
    tests = stellar.counter("expansion_exact_tests")
    print(f"exact tests {tests} of {src.size * n ** 3} star-leaf pairs")
    assert 0 < tests <= src.size * n ** 3 // 4


def _rates_close(a, b):
    scale = np.abs(b).max(axis=1, keepdims=True)
    return bool(np.all(np.abs(a - b) <= 1e-9 * np.abs(b) + 1e-13 * scale))


def test_tracer_and_opacities_see_the_expanded_medium(golden):
    """After an expansion the tracer's packed copy is rebuilt and ftte_compute_opacities reads the scaled species: both give what a
    fresh context gives that was handed the expanded arrays through set_medium.  The opacities compare bit for bit.  The traced
    rates are sums of fp64 atomic additions whose last bits depend on the run (include/ftte.h, ftte_point_sources), on one context
    as much as between two, so they compare at the bound the suite uses for traced rates everywhere (test_gas_state_gpu.py:
    1e-9 |ref| + 1e-13 max|ref| per plane), after the assertion that the trace before the expansion lies far outside it."""
    g = golden("expansion_uniform16")
    tables = golden("point16_homogeneous")["tables"]
    beta = np.array([[6.3e-18, 1.2e-18, 2.0e-19], [0.0, 7.4e-18, 1.5e-18], [0.0, 0.0, 1.6e-18]])
    src, ndot = g["src_cell"][:3], np.array([50.0, 20.0, 5.0])

    def trace(st):
        st.set_zero_rates()
        st.point_sources(src, ndot)
        return st.rates()

    with rt.StellarTransfer() as A:
        _load(A, g)
        A.set_rate_tables(tables)
        before = trace(A)                       # the packed copy now holds the medium before the expansion
        A.compute_opacities_from_medium(beta)
        A.expand_hii_regions(g["src_cell"], g["params"])
        after = trace(A)
        A.compute_opacities_from_medium(beta)
        J_a = A.transport(*rt.healpix_directions(1), np.array([2e-22, 1e-22, 3e-23]))
    with rt.StellarTransfer() as B:
        B.set_grid(int(g["n"]), g["level"], float(g["box"]))
        B.set_medium(g["HI_out"], g["HeI_out"], g["HeII_out"], g["rho_out"], None, 0)
        B.set_rate_tables(tables)
        fresh = trace(B)
        B.compute_opacities_from_medium(beta)
        J_b = B.transport(*rt.healpix_directions(1), np.array([2e-22, 1e-22, 3e-23]))
    assert not _rates_close(before, fresh)
    assert np.any(np.abs(before - fresh) > 1e-3 * np.abs(fresh))
    assert _rates_close(after, fresh)
    assert np.array_equal(J_a, J_b) and J_a.max() > 0      # the same opacities: the sweep is deterministic


def _expect(code, fn, *args, **kw):
    with pytest.raises(rt.FtteError) as err:
        fn(*args, **kw)
    assert err.value.status == code, str(err.value)
    return str(err.value)


def test_refusals_leave_the_medium_alone(golden):
    g = golden("expansion_refined")
    src, nc = g["src_cell"][:5], g["level"].size
    before = [g[k] for k in FIELDS]
    with rt.StellarTransfer() as st:
        assert "ftte_set_grid" in _expect("FTTE_ERR_STATE", st.expand_hii_regions, src)           # no grid
        st.set_grid(int(g["n"]), g["level"], float(g["box"]))
        assert "density" in _expect("FTTE_ERR_STATE", st.expand_hii_regions, src)                 # no medium
        _expect("FTTE_ERR_STATE", st.density)
        st.set_medium(g["HI"], g["HeI"], g["HeII"], None, None, 0)
        assert "density" in _expect("FTTE_ERR_STATE", st.expand_hii_regions, src)                 # a medium without rho
        _expect("FTTE_ERR_STATE", st.density)
        _load(st, g)
        cells = np.ascontiguousarray(src, np.int64)
        coef = np.empty(nc)
        rc = st._lib.ftte_expand_hii_regions(st._ctx, -1, cells.ctypes.data_as(C.POINTER(C.c_int64)), None,
                                             coef.ctypes.data_as(C.POINTER(C.c_double)), None)
        assert rc == -1                                                                            # nsrc < 0
        for bad in (-1, nc):
            msg = _expect("FTTE_ERR_ARG", st.expand_hii_regions, [int(src[0]), bad, int(src[1])], g["params"][:3])
            assert "source 1 " in msg
            _expect("FTTE_ERR_ARG", st.expand_hii_regions, [int(src[0]), bad, int(src[1])])
        assert _same(_state(st), before)
        for value in (0.0, -1e-24, np.nan, np.inf):
            rho = g["rho"].copy()
            rho[src[2]] = value
            _load(st, g, rho=rho)
            msg = _expect("FTTE_ERR_ARG", st.expand_hii_regions, src)
            assert "source 2 " in msg and "not positive and finite" in msg
            assert _same(_state(st), [rho, g["HI"], g["HeI"], g["HeII"]])
            st.expand_hii_regions(src, g["params"][:5])                   # given parameters do not read the host leaf's density
        _load(st, g)
        coef, changed = st.expand_hii_regions(src)                        # and the context is still good
        assert changed > 0 and (coef < 1).sum() == changed


def test_multi_device_context_refuses(golden):
    g = golden("expansion_uniform16")
    with rt.StellarTransfer(devices=[0, 0]) as st:
        st.set_grid(int(g["n"]), g["level"], float(g["box"]))
        _expect("FTTE_ERR_UNSUPPORTED", st.expand_hii_regions, g["src_cell"], g["params"])
        _expect("FTTE_ERR_UNSUPPORTED", st.density)


def test_fortran_host(golden, tmp_path):
    """fortran/ftte_demo_expansion on the refined golden: stars as call sequences, ftte_locate_cell, params = NULL; the five arrays
    it writes are the reference's bit for bit"""
    exe = os.path.join(ROOT, "fortran", "ftte_demo_expansion")
    if not os.path.exists(exe):
        pytest.skip("fortran/ftte_demo_expansion not built (no Fortran compiler at build time)")
    g = golden("expansion_refined")
    nc, ns = g["level"].size, g["src_cell"].size
    case, out = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(case, "wb") as f:
        f.write(np.array([int(g["n"]), nc, ns, g["star_position"].shape[1]], "<i4").tobytes())
        f.write(np.array([float(g["box"])], "<f8").tobytes())
        f.write(g["level"].astype("<i4").tobytes())
        for k in FIELDS:
            f.write(g[k].astype("<f8").tobytes())
        f.write(g["star_level"].astype("<i4").tobytes())
        f.write(np.ascontiguousarray(g["star_position"], "<i4").tobytes())      # [star][maxpos] == Fortran (maxpos, nstars)
    res = subprocess.run([exe, str(case), str(out)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "ftte_demo_expansion OK" in res.stdout, res.stdout + res.stderr
    got = np.fromfile(out, "<f8").reshape(5, nc)
    for a, key in zip(got, ("rho_coef", "rho_out", "HI_out", "HeI_out", "HeII_out")):
        assert np.array_equal(a, g[key]), key
