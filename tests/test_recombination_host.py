"""The diffuse recombination source on the host (no GPU): radiativetransfer_amd/csrc/ftte_recombination_math.h compiled by g++ --
under the sanitizers as a program (tests/host/recombination_check.cpp), and as the small library of tests/_recombination.py against a
numpy restatement, for photon conservation, at its edges, and in the on-the-spot limit as algebra -- the helper
ground_recombination_tables, and the entry points' names where hosts look for them.  The reference has nothing to compare with: its
emissivity is hard-wired to zero (transportRoutinesModule.f90:673-675)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _recombination as R

ROOT = R.ROOT
EPS = R.EPS
SYMBOLS = ["ftte_set_ground_recombination", "ftte_recombination_source", "ftte_recombination_source_device"]


@pytest.fixture(scope="module")
def tab():
    return R.tables()


@pytest.fixture(scope="module")
def media(golden):
    out = {}
    for name in R.MEDIA:
        m = R.medium(golden, name)
        m["logtem"] = R.libm_log(m["tgas"])
        out[name] = m
    return out


def _state(m):
    return m["rho"], m["logtem"], m["HI"], m["HeI"], m["HeII"]


def test_statement_under_the_sanitizers(tmp_path):
    """tests/host/recombination_check.cpp's main(): S finite and not negative, 4 pi S D = E, the lost pairs, bad densities named -- with
    AddressSanitizer and UBSan, as a program of its own"""
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "recombination_check")
    subprocess.check_call([gxx, *R.SANITIZE, "-I" + R.CSRC, R.SOURCE, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:])
    assert res.returncode == 0 and "recombination source under the sanitizers: ok" in res.stdout, res.stdout[-4000:] + res.stderr[-4000:]


@pytest.mark.parametrize("share", ["identity", "split"])
@pytest.mark.parametrize("name", R.MEDIA)
def test_restatement(media, tab, name, share):
    """S of the header against the numpy restatement: |difference| <= 32 eps S_scale per leaf and group.  The derivation: every term
    of E and of D is a product of non-negative numbers and every sum adds non-negative terms, so relative errors add and nothing
    cancels but three differences.  nh - HI and nhe - HeI - HeII are formed from the same operands by the same operations on both
    sides, hence equal; the interpolation's is covered by measuring against S_scale, S with the larger of the two table nodes
    (both forms of the interpolation are within 4 eps of max(a, b) of the exact value).  Roundings of one side: the coefficient 4,
    de 2, R 2, a share's product 1, E's sum 2, D's products and sum 3, 4 pi D 1, the division 1: 16.  Two sides: 32.  Where D is 0
    both sides give exactly 0."""
    m = media[name]
    sh = R.IDENTITY if share == "identity" else R.SPLIT
    S, E, lost, status = R.source(*_state(m), tab["grid"], tab["g"], tab["ksi"], sh)
    assert status == 0
    wS, wE, D, wlost, scale = R.source_numpy(*_state(m), tab["grid"], tab["g"], tab["ksi"], sh)
    assert lost == wlost
    dark = D == 0
    assert np.array_equal(S[dark], np.zeros(dark.sum())) and np.array_equal(wS[dark], S[dark])
    bound = 32 * EPS * scale
    worst = np.max(np.abs(S - wS)[~dark] / np.where(bound[~dark] > 0, bound[~dark], 1.0))
    print(f"{name} {share}: worst difference / bound {worst:.3f}; {lost} lost pairs, {np.count_nonzero(S)} of {S.size} S > 0")
    assert np.all(np.abs(S - wS) <= bound)
    assert np.count_nonzero(S) > S.size // 2


@pytest.mark.parametrize("share", ["identity", "split"])
@pytest.mark.parametrize("name", R.MEDIA)
def test_photon_conservation(media, tab, name, share):
    """a leaf bathed in J = S re-absorbs what it emits: 4 pi S[j] D[j] == E[j] to 4 eps relative wherever D[j] > 0 (S carries the
    roundings of 4 pi D and of the division, the product here two more)"""
    m = media[name]
    sh = R.IDENTITY if share == "identity" else R.SPLIT
    S, E, lost, status = R.source(*_state(m), tab["grid"], tab["g"], tab["ksi"], sh)
    assert status == 0
    nh, nhe, hi, hei, heii = R.clipped(m["rho"], m["HI"], m["HeI"], m["HeII"])
    D = R.capture(hi, hei, heii, tab["ksi"])
    lit = D > 0
    back = 4.0 * R.PI * S * D
    err = np.abs(back - E)[lit] / np.where(E[lit] > 0, E[lit], 1.0)
    print(f"{name} {share}: worst |4 pi S D - E| / E = {err.max() / EPS:.2f} eps over {lit.sum()} pairs")
    assert err.max() <= 4 * EPS
    assert np.all(back[lit][E[lit] == 0] == 0)


def _one(tab, rho, T, HI, HeI, HeII, share=R.IDENTITY, ksi=None):
    a = [np.array([float(v)]) for v in (rho, math.log(T), HI, HeI, HeII)]
    S, E, lost, status = R.source(*a, tab["grid"], tab["g"], tab["ksi"] if ksi is None else ksi, share)
    return S[:, 0], E[:, 0], lost, status


def _g_at(tab, T):
    """the three coefficients at T by hand: linear in log T between the two nodes around it"""
    a, b, c = tab["grid"]
    x = (min(max(math.log(T), a), b) - a) / c
    i = min(int(x), tab["g"].shape[1] - 2)
    return tab["g"][:, i] + (x - i) * (tab["g"][:, i + 1] - tab["g"][:, i])


def test_edges_by_hand(tab):
    rho, T = 2.0e-24, 2.0e4
    nh, nhe = R.PSI * rho / R.MH, (1 - R.PSI) * rho / R.MHE
    ksi, g = tab["ksi"], _g_at(tab, T)
    # HI = 0: hydrogen recombines, nothing absorbs group 0 -- lost, and S[0] = 0; groups 1 and 2 find helium
    S, E, lost, status = _one(tab, rho, T, 0.0, 0.5 * nhe, 0.3 * nhe)
    de = nh + 0.3 * nhe + 2 * 0.2 * nhe
    assert status == 0 and lost == 1 and S[0] == 0.0 and E[0] == pytest.approx(g[0] * de * nh, rel=1e-12)
    assert S[1] == pytest.approx(g[1] * de * 0.3 * nhe / (4 * R.PI * 0.5 * nhe * ksi[1, 2]), rel=1e-12)
    assert S[2] == pytest.approx(g[2] * de * 0.2 * nhe / (4 * R.PI * (0.3 * nhe * ksi[2, 1] + 0.5 * nhe * ksi[2, 2])), rel=1e-12)
    # a species above its element's budget is clipped: HI = 3 nh is nh, HeI = 2 nhe is nhe and leaves HeII no room
    assert all(np.array_equal(a, b) for a, b in zip(_one(tab, rho, T, 3 * nh, 2 * nhe, 0.5 * nhe)[:2], _one(tab, rho, T, nh, nhe, 0.0)[:2]))
    S, E, lost, status = _one(tab, rho, T, 0.5 * nh, 0.8 * nhe, 0.7 * nhe)      # HeII clipped to 0.2 nhe: no HeIII
    want = _one(tab, rho, T, 0.5 * nh, 0.8 * nhe, nhe - 0.8 * nhe)
    assert np.array_equal(S, want[0]) and np.array_equal(E, want[1]) and E[2] == 0.0
    S, E, lost, status = _one(tab, rho, T, -1.0, -1.0, -1.0)                     # negative species count as none: HII and HeIII
    assert np.array_equal(E, _one(tab, rho, T, 0.0, 0.0, 0.0)[1]) and lost == 2 and not S.any() and E[1] == 0.0      # emit, no HeII does
    # T below and above the table's ends: clamped like the chemistry, to the end nodes' coefficients
    lo, hi = math.exp(tab["grid"][0]), math.exp(tab["grid"][1])
    state = (0.3 * nh, 0.4 * nhe, 0.4 * nhe)
    for end, beyond, node in ((lo, lo * 1e-3, 0), (hi, hi * 1e3, -1)):
        at, out = _one(tab, rho, end, *state), _one(tab, rho, beyond, *state)
        assert np.array_equal(at[0], out[0]) and np.array_equal(at[1], out[1])
        de = 0.7 * nh + 0.4 * nhe + 2 * (nhe - 0.4 * nhe - 0.4 * nhe)
        assert out[1][0] == pytest.approx(tab["g"][0, node] * de * 0.7 * nh, rel=1e-12)
    # fully neutral gas: no recombination, S = 0, nothing lost
    S, E, lost, status = _one(tab, rho, T, nh, nhe, 0.0)
    assert status == 0 and lost == 0 and not S.any() and not E.any()
    # a density that is zero, negative, infinite or NaN stops the leaf
    for bad in (0.0, -rho, math.inf, math.nan):
        assert _one(tab, bad, T, 0.1 * nh, 0.1 * nhe, 0.1 * nhe)[3] == 1


def test_on_the_spot_limit_as_algebra(tab):
    """share = the H row only, J := S, hydrogen alone with case-A k2: the balance k2_A de HII = (k1 de + 4 pi S ksi24) HI iterated to
    its fixed point equals the case-B balance with k2_B' = k2_A - g[0], k2_B' de HII = k1 de HI, because 4 pi S ksi24 HI is g[0] de HII
    by construction.  The map contracts with q = g[0]/k2_A < 0.6 below 1e5 K, so a last change of delta leaves an error of at most
    delta q/(1 - q) < 1.5 delta; 64 eps for the roundings of the two closed forms."""
    a, b, c = tab["grid"]
    T = np.array([8.0e3, 1.5e4, 3.0e4, 6.0e4])
    i = np.rint((np.log(T) - a) / c).astype(int)
    T = np.exp(a + i * c)                                     # on the nodes: the coefficients are the tables' entries
    k1, k2A, g0 = tab["ka"][0, i], tab["ka"][1, i], tab["g"][0, i]
    assert np.all(g0 / k2A < 0.6)
    rho = np.array([1e-26, 1e-25, 1e-24, 1e-23])
    nh, nhe = R.PSI * rho / R.MH, (1 - R.PSI) * rho / R.MHE
    ksi = np.zeros((3, 3))
    ksi[0, 0] = tab["ksi"][0, 0]

    def balance(k2, gamma):
        """HI of k2 (nh - HI)^2 = (k1 (nh - HI) + gamma) HI, hydrogen alone (de = HII): with y = HI/nh,
        (k1 + k2) nh y^2 - ((k1 + 2 k2) nh + gamma) y + k2 nh = 0, the smaller root, in the form that subtracts nothing"""
        A, B, Cq = (k1 + k2) * nh, (k1 + 2.0 * k2) * nh + gamma, k2 * nh
        disc = (k1 * nh) ** 2 + 2.0 * gamma * (k1 + 2.0 * k2) * nh + gamma * gamma      # B^2 - 4 A C multiplied out: positive terms only
        return nh * (2.0 * Cq / (B + np.sqrt(disc)))

    HI, delta = balance(k2A, 0.0), 1e-14
    for rounds in range(200):
        S, E, lost, status = R.source(rho, np.log(T), HI, nhe, np.zeros(4), tab["grid"], tab["g"], ksi, R.H_ONLY)
        assert status == 0 and lost == 0
        new = balance(k2A, 4.0 * R.PI * S[0] * ksi[0, 0])
        change = np.max(np.abs(new - HI) / HI)
        HI = new
        if change < delta:
            break
    want = balance(k2A - g0, 0.0)
    err = np.abs(HI - want) / want
    print(f"on-the-spot limit: {rounds + 1} rounds, worst relative difference {err.max():.3e}")
    assert rounds < 100 and err.max() <= 1.5 * delta + 64 * EPS
    assert np.any(HI < 0.9 * balance(k2A, 0.0))      # (the diffuse photons matter: case A alone leaves the hot cells more neutral)


def test_ground_recombination_tables(tab):
    """non-negative and finite; rows 0 and 2 the difference of the two cases' k2 and k6; row 1 the radiative fit of coll_rates' case-A
    k4 less case B, restated here -- without the dielectronic term, so it falls monotonically above 1e3 K.  Between 1e4 and
    1e7 K its ratio to row 0 stays in [1, 16]: the two fits give 1.07 at 1e4 K, where helium's and hydrogen's ground states recombine
    alike, and 11.8 at 1e7 K, helium's radiative power law T^-0.6353 falling more slowly than hydrogen's difference; with the
    dielectronic term left in the ratio would pass 100 near 1e6 K."""
    import radiativetransfer_amd as rt
    g, ka, kb = tab["g"], tab["ka"], tab["kb"]
    a, b, c = tab["grid"]
    assert g.shape == (3, 5000) and np.all(g >= 0) and np.all(np.isfinite(g))
    assert np.array_equal(g[0], np.maximum(ka[1] - kb[1], 0)) and np.array_equal(g[2], np.maximum(ka[5] - kb[5], 0))
    T = np.exp(a + np.arange(5000).astype(np.float32).astype(np.float64) * c)
    w = lambda v: float(np.float32(v))      # noqa: E731
    radiative = w(3.92e-13) / (T / w(11605.0)) ** w(0.6353)
    tmp = float(np.float32(2.0) * np.float32(24.587)) * 1.60217646e-12 / (1.3806503e-16 * T)
    want = np.maximum(radiative - w(1.26e-14) * tmp ** 0.75, 0.0)
    rel = np.abs(g[1] - want) / np.where(want > 0, radiative, 1.0)
    print(f"row 1 against its restatement: worst {rel.max() / EPS:.1f} eps of the radiative fit")
    assert rel.max() <= 64 * EPS and np.array_equal(g[1] == 0, want == 0)
    pos = g[1] > 0
    assert not pos[T < 100].any() and pos[T > 200].all()      # the radiative fit falls below case B's near 130 K
    # no dielectronic bump: the difference of the two power laws, T^-0.6353 and T^-0.75, peaks at (0.75/0.6353)^(1/0.1147) = 4.3 times
    # the temperature it vanishes at and falls from there on; k4_A - k4_B itself rises again near 1e5 K
    assert np.all(np.diff(g[1][T > 1e3]) < 0) and np.any(np.diff((ka[3] - kb[3])[T > 1e3]) > 0)
    band = (T >= 1e4) & (T <= 1e7)
    ratio = g[1][band] / g[0][band]
    print(f"row 1 / row 0 over 1e4 .. 1e7 K: {ratio.min():.3f} .. {ratio.max():.3f}")
    assert ratio.min() >= 1.0 and ratio.max() <= 16.0
    assert np.max((ka[3] - kb[3])[band] / g[0][band]) > 100.0
    small = rt.ground_recombination_tables(64, 10.0, 1e6)
    k64 = rt.rate_coefficient_tables(64, 10.0, 1e6, 1)[0]
    assert small.shape == (3, 64) and np.array_equal(small[0], np.maximum(k64[1] - rt.rate_coefficient_tables(64, 10.0, 1e6, 2)[0][1], 0))


# ---- the entry points exist everywhere a host reaches them (as tests/test_thermal_host.py) ----------------------------------

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
    assert _lib.STATUS[lib.ftte_set_ground_recombination(None, 2, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_recombination_source(None, None, None, None, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_recombination_source_device(None, None, None, None, None)] == "FTTE_ERR_ARG"


def test_python_surface():
    import inspect
    import radiativetransfer_amd as rt
    assert "recombination" in inspect.signature(rt.evolve).parameters
    for name in ("set_ground_recombination", "recombination_source", "recombination_source_device"):
        assert callable(getattr(rt.StellarTransfer, name))
