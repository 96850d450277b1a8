"""Population slots on the GPU: many rate-table sets held at once, every star of a batch naming the slot it reads
(ftte_stellar_beta_tables, ftte_set_population_tables, ftte_get_population_tables, ftte_point_sources_populations).

Tolerances are those of tests/test_point_gpu.py, for its reasons.  Tables against the reference's: 1e-13 relative (exp/log of two
math libraries).  Tracer against the oracle: 1e-9 of the rate plus 1e-13 of the largest rate of that reaction (a ray deposits a
difference of nearly equal numbers; rays are summed with atomics).  Tracer against the tracer (the same deposits in another order
of the atomics): 1e-11 / 1e-14.  Escape sums: 1e-9 relative.  Tables against the single call's and levels: equal.
"""
import functools
import os
import sys

import numpy as np
import pytest

import _oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_point as M  # noqa: E402  (synthetic_population() only)

pytestmark = pytest.mark.gpu

# (iSpectrum, coefSpectrum, iMetal, coefMetal): every iMetal bracket of the library, coefMetal on both ends and inside, two spectra
POPULATIONS = [(3, 0.25, 1, 0.0), (3, 0.25, 2, 0.3), (20, 0.6, 3, 1.0), (20, 0.6, 4, 0.3)]


@pytest.fixture(scope="module")
def pop():
    return M.synthetic_population()


@pytest.fixture(scope="module")
def stellar():
    import radiativetransfer_amd as rt
    st = rt.StellarTransfer()
    yield st
    st.close()


def _close(mine, ref, rel=1e-9, floor=1e-13):
    scale = np.abs(ref).max(axis=-1, keepdims=True)
    err = np.abs(mine - ref) - (rel * np.abs(ref) + floor * scale)
    assert np.all(err <= 0), f"worst excess {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"


def _build(st, pop, populations):
    p = np.array(populations)
    return st.stellar_beta_tables(pop[0], pop[1], pop[2], p[:, 0].astype(int), p[:, 1], p[:, 2].astype(int), p[:, 3])


@pytest.fixture(scope="module")
def three(stellar, pop):
    """The tables of the first three populations as the slots hold them (what the oracle is given for that slot)."""
    _build(stellar, pop, POPULATIONS[:3])
    return np.stack([stellar.population_tables(k) for k in range(3)])


def test_tables(stellar, golden, pop):
    totals = _build(stellar, pop, POPULATIONS)
    assert stellar.counter("population_slots") == len(POPULATIONS)
    slots = [stellar.population_tables(k) for k in range(len(POPULATIONS))]
    for k, (isp, cs, im, cm) in enumerate(POPULATIONS):
        total = stellar.stellar_beta_table(pop[0], pop[1], pop[2], isp, cs, im, cm)
        assert total == totals[k]
        assert np.array_equal(slots[k], stellar.rate_tables()), k
        assert np.array_equal(stellar.population_tables(k), slots[k])  # the single call leaves the slots alone
    assert not np.array_equal(slots[0], slots[1]) and not np.array_equal(slots[2], slots[3])
    # the two populations of the reference's own vectors, side by side
    names = ("point16_homogeneous", "point10_refined_dust")
    gs = [golden(n) for n in names]
    totals = _build(stellar, pop, [(int(g["iSpectrum"]), float(g["coefSpectrum"]), int(g["iMetal"]), float(g["coefMetal"])) for g in gs])
    assert stellar.counter("population_slots") == 2
    for k, g in enumerate(gs):
        if "totalIntegral" in g.files:
            assert totals[k] == float(g["totalIntegral"])
        mine, ref = stellar.population_tables(k).reshape(6, -1), g["tables"].reshape(6, -1)
        assert np.all(np.abs(mine - ref) <= 1e-13 * np.abs(ref)), names[k]
    # tables handed over come back as they went in
    given = np.stack([gs[1]["tables"].reshape(6, -1), gs[0]["tables"].reshape(6, -1), 3.0 * gs[0]["tables"].reshape(6, -1)])
    stellar.set_population_tables(given)
    assert stellar.counter("population_slots") == 3
    for k in range(3):
        assert np.array_equal(stellar.population_tables(k).reshape(6, -1), given[k])


def _random_tree(rng, n, p1, p2):
    level = []
    for _ in range(n ** 3):
        if rng.random() < p1:
            for _ in range(8):
                if rng.random() < p2:
                    level += [2] * 8
                else:
                    level.append(1)
        else:
            level.append(0)
    return np.array(level, np.int32)


SLOT_OF_STAR = np.array([2, 0, 1, 2, 0, 1, 1, 0, 2], np.int32)  # not monotonic; every slot used by stars that are apart


@functools.lru_cache(maxsize=None)
def _refined_case(dust):
    """12^3 random three-level tree and media as test_tracer_against_oracle_refined, nine stars."""
    rng = np.random.default_rng(100 + dust)
    n = 12
    level = _random_tree(rng, n, 0.15, 0.2)
    nc = level.size
    HI = 10 ** rng.uniform(-5.5, -3.2, nc)
    HeI, HeII = 0.08 * HI, 10 ** rng.uniform(-7, -5, nc)
    rho, abun2 = 1.7e-24 * 10 ** rng.uniform(-4, -2, nc), 10 ** rng.uniform(-3, -0.5, nc)
    src = rng.choice(nc, 9, replace=False)
    ndot = rng.integers(1, 50, 9).astype(float)
    return dict(n=n, level=level, box=3.0e22, HI=HI, HeI=HeI, HeII=HeII, rho=rho, abun2=abun2, src=src, ndot=ndot, dust=dust)


def _set_case(st, c):
    st.set_grid(c["n"], c["level"], c["box"])
    st.set_medium(c["HI"], c["HeI"], c["HeII"], c["rho"], c["abun2"], c["dust"])
    st.set_zero_rates()


def _oracle(c, stars, tables):
    return O.point_sources(c["n"], c["level"], c["HI"], c["HeI"], c["HeII"], c["rho"], c["abun2"], c["box"], c["dust"],
                           c["src"][stars], c["ndot"][stars], tables.reshape(6, -1))


@pytest.mark.parametrize("dust", [0, 2])
def test_tracer_against_oracle_per_population(stellar, pop, three, dust):
    c = _refined_case(dust)
    ref = sum(_oracle(c, np.flatnonzero(SLOT_OF_STAR == k), three[k])[0] for k in range(3))
    hp_ref = [_oracle(c, [s], three[SLOT_OF_STAR[s]])[1] for s in range(9)]
    _build(stellar, pop, POPULATIONS[:3])
    _set_case(stellar, c)
    hp = stellar.point_sources_populations(c["src"], c["ndot"], SLOT_OF_STAR)
    mine = stellar.rates()
    print("highest pixel levels", hp.tolist(), hp_ref)
    assert hp.tolist() == hp_ref
    _close(mine, ref)
    assert np.array_equal(mine == 0, ref == 0)


@pytest.mark.parametrize("dust", [0, 2])
def test_against_the_single_population_path(stellar, pop, dust):
    c = _refined_case(dust)
    _set_case(stellar, c)
    one_by_one = []
    for s in range(9):
        stellar.stellar_beta_table(pop[0], pop[1], pop[2], *POPULATIONS[SLOT_OF_STAR[s]])
        hp = stellar.point_sources(c["src"][s:s + 1], c["ndot"][s:s + 1])
        one_by_one.append((hp, stellar.escape(1)))
    ref = stellar.rates()
    _build(stellar, pop, POPULATIONS[:3])
    stellar.set_zero_rates()
    hp = stellar.point_sources_populations(c["src"], c["ndot"], SLOT_OF_STAR)
    _close(stellar.rates(), ref, rel=1e-11, floor=1e-14)
    esc = stellar.escape(9)
    # this box is 9.7 kpc wide: rays cross the inner output radii only, and the spectrum, taken at 100 kpc, stays zero
    # (test_escape_spectrum_through_slots has a box that reaches it)
    assert esc["remaining"].any() and esc["boundary"].any()
    for s in range(9):
        assert hp[s] == one_by_one[s][0]
        for key in ("remaining", "boundary", "dust", "spectrum", "fraction"):
            want = one_by_one[s][1][key][0]
            assert np.all(np.abs(esc[key][s] - want) <= 1e-9 * np.abs(want) + 1e-300), (s, key)


def test_escape_spectrum_through_slots(stellar, golden, pop):
    """The reference's escape vector: from one of its stars rays reach the last output radius, where the spectrum is taken (which
    rays do is geometry, the same for any population).  Each star's escape record through a slot equals the record of the same star traced alone with that population current."""
    g = golden("point12_escape")
    lit = g["ndotSpectrum"].any(axis=-1)
    assert lit.any()
    stellar.set_grid(int(g["n"]), g["level"], float(g["box"]))
    stellar.set_medium(g["HI"], g["HeI"], g["HeII"], g["rho"], g["abun2"], int(g["dust"]))
    src, ndot, slot = g["src_leaf"], g["src_weight"].astype(float), np.array([1, 0, 1], np.int32)
    alone = []
    for s in range(3):
        stellar.stellar_beta_table(pop[0], pop[1], pop[2], *POPULATIONS[slot[s]])
        stellar.point_sources(src[s:s + 1], ndot[s:s + 1])
        alone.append(stellar.escape(1))
    _build(stellar, pop, POPULATIONS[:2])
    stellar.point_sources_populations(src, ndot, slot)
    esc = stellar.escape(3)
    assert np.array_equal(esc["spectrum"].any(axis=-1), lit)
    for s in range(3):
        for key in ("remaining", "boundary", "dust", "spectrum", "fraction"):
            want = alone[s][key][0]
            assert np.all(np.abs(esc[key][s] - want) <= 1e-9 * np.abs(want) + 1e-300), (s, key)


def test_batch_seam(stellar, golden):
    """More stars than one batch of the split queues (1024): star s and star s - 1024 read different slots, and a ray knows its
    star only by its number within the batch."""
    g = golden("point16_homogeneous")
    n = 16
    rng = np.random.default_rng(7)
    stellar.set_grid(n, np.zeros(n ** 3, np.int32), float(g["box"]))
    HI = g["HI"] * 10 ** rng.uniform(-0.5, 0.5, n ** 3)
    stellar.set_medium(HI, g["HeI"], g["HeII"], None, None, 0)
    base = g["tables"].reshape(6, -1)
    # three table sets that differ in every entry and by a different factor per reaction
    tables = np.stack([base, base * np.array([2.0, 0.5, 3.0, 2.0, 0.5, 3.0])[:, None], base ** 1.01])
    nstar = 1100
    src = rng.choice(n ** 3, nstar, replace=False)
    ndot = rng.uniform(1, 3, nstar)
    slot = (np.arange(nstar) % 3).astype(np.int32)
    assert np.all(slot[1024:] != slot[:nstar - 1024])
    stellar.set_zero_rates()
    for k in range(3):
        stellar.set_rate_tables(tables[k])
        stellar.point_sources(src[slot == k], ndot[slot == k])
    ref = stellar.rates()
    stellar.set_population_tables(tables)
    stellar.set_zero_rates()
    hp = stellar.point_sources_populations(src, ndot, slot)
    _close(stellar.rates(), ref, rel=1e-11, floor=1e-14)
    esc = stellar.escape(nstar)
    print("highest pixel levels beyond the seam", sorted(set(hp[1024:].tolist())), "before it", sorted(set(hp[:1024].tolist())))
    for s in np.linspace(1024, nstar - 1, 10).astype(int):
        stellar.set_rate_tables(tables[slot[s]])
        assert hp[s] == stellar.point_sources(src[s:s + 1], ndot[s:s + 1]), s
        alone = stellar.escape(1)
        for key in ("remaining", "boundary"):
            assert np.all(np.abs(esc[key][s] - alone[key][0]) <= 1e-9 * np.abs(alone[key][0]) + 1e-300), (s, key)


def test_one_slot_for_all(stellar, golden):
    g = golden("point10_refined_dust")
    stellar.set_grid(int(g["n"]), g["level"], float(g["box"]))
    stellar.set_medium(g["HI"], g["HeI"], g["HeII"], g["rho"], g["abun2"], int(g["dust"]))
    other = golden("point16_homogeneous")["tables"]
    rng = np.random.default_rng(3)
    src = rng.choice(g["level"].size, 40, replace=False)
    ndot = rng.uniform(1, 3, 40)
    stellar.set_rate_tables(g["tables"])
    stellar.set_zero_rates()
    hp_ref = stellar.point_sources(src, ndot)
    ref = stellar.rates()
    # the current tables are another population's from here on: the slot variant neither reads nor changes them
    stellar.set_rate_tables(other)
    before = stellar.rate_tables()
    stellar.set_population_tables(g["tables"].reshape(1, 6, -1))
    stellar.set_zero_rates()
    hp = stellar.point_sources_populations(src, ndot, np.zeros(40, np.int32))
    _close(stellar.rates(), ref, rel=1e-11, floor=1e-14)
    assert hp.max() == hp_ref
    assert np.array_equal(stellar.rate_tables(), before) and np.array_equal(before.reshape(-1), other.reshape(-1))
    assert stellar.point_sources_populations([], [], []).size == 0


def test_errors_and_lifetime(stellar, golden):
    import radiativetransfer_amd as rt
    from radiativetransfer_amd import FtteError

    def expect(status, call, *args):
        with pytest.raises(FtteError) as e:
            call(*args)
        assert e.value.status == status, e.value
        return str(e.value)

    tables = golden("point16_homogeneous")["tables"].reshape(6, -1)
    objects = stellar.counter("device_objects")
    z = np.full(64, 1e-6)
    with rt.StellarTransfer() as st:
        assert st.counter("population_slots") == 0
        expect("FTTE_ERR_STATE", st.population_tables, 0)
        st.set_grid(4, np.zeros(64, np.int32), 1.0e22)
        st.set_medium(z, z, z, None, None, 0)
        st.set_rate_tables(tables)      # current tables alone are not slots
        expect("FTTE_ERR_STATE", st.point_sources_populations, [21], [1.0], [0])
        npop = 3
        st.set_population_tables(np.stack([tables] * npop))
        assert st.counter("population_slots") == npop
        st.set_zero_rates()
        st.point_sources_populations([21, 5], [1.0, 2.0], [2, 0])
        before = st.rates()
        assert before[0].sum() > 0
        assert "star 1" in expect("FTTE_ERR_ARG", st.point_sources_populations, [21, 5, 7], [1.0, 1.0, 1.0], [0, -1, npop])
        assert "star 2" in expect("FTTE_ERR_ARG", st.point_sources_populations, [21, 5, 7], [1.0, 1.0, 1.0], [0, 1, npop])
        expect("FTTE_ERR_ARG", st.point_sources_populations, [64], [1.0], [0])   # the preconditions of point_sources
        expect("FTTE_ERR_ARG", st.population_tables, npop)
        expect("FTTE_ERR_ARG", st.population_tables, -1)
        assert np.array_equal(st.rates(), before)
        with pytest.raises(ValueError):
            st.set_population_tables(np.zeros(10))
        with pytest.raises(ValueError):
            st.point_sources_populations([1, 2], [1.0, 1.0], [0])
        st.set_population_tables(tables[None])                                   # fewer slots replace more
        assert st.counter("population_slots") == 1
        expect("FTTE_ERR_ARG", st.point_sources_populations, [21], [1.0], [1])
        assert st.counter("device_objects") > objects
    assert stellar.counter("device_objects") == objects
    with rt.StellarTransfer(devices=[0, 0]) as multi:
        expect("FTTE_ERR_UNSUPPORTED", multi.point_sources_populations, [0], [1.0], [0])
        expect("FTTE_ERR_UNSUPPORTED", multi.set_population_tables, tables[None])
        expect("FTTE_ERR_UNSUPPORTED", multi.population_tables, 0)
