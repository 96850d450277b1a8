"""The absorption line of csrc/ftte_spectra_math.h on the host (g++ through tests/_spectra.py; no GPU): the profile against an
independent Voigt function (tests/golden/voigt_table.npz: scipy's Faddeeva function, make_golden_voigt.py), the line against plain
numpy, known answers, the geometry of the sightlines against the numpy restatement of the projected map, the helpers of the GPU tests (the
segments of a uniform grid, trees with sightlines of a wanted length), the host's batch rule (csrc/ftte_spectra.h, against a stub of
the HIP runtime) with the tests' restatement of it, and the whole under the sanitizers as programs of their own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _analysis as A
import _spectra as S

DOPPLER = (S.LYMAN_ALPHA[0], 0.0, S.LYMAN_ALPHA[2], 0.0)


@pytest.fixture(scope="module")
def voigt(golden):
    return golden("voigt_table")


@pytest.fixture(scope="module")
def refined(golden):
    g = golden("analysis_refined6")
    return g, A.Tree(int(g["n"]), g["level"])


def thermal_b(tgas, line=DOPPLER):
    return float(np.sqrt(2.0 * S.KB * tgas / line[2] + line[3] ** 2))


# ---- 1. the profile

# relative error of Tepper-Garcia's form, a property of the formula: |x| <= 2, 2..8, >= 8 (the largest sit near |x| = 3..4, where H < 1e-4)
BOUNDS = {1.0e-5: (3e-5, 0.02, 1.1e-3), 4.7e-4: (1.2e-3, 0.03, 1.1e-3), 4.7e-3: (1.1e-2, 0.06, 1.1e-3)}


@pytest.mark.parametrize("k", [0, 1, 2])
def test_profile_against_the_faddeeva_function(voigt, k):
    a = float(voigt["a"][k])
    for name, bound in zip(("core", "mid", "wing"), BOUNDS[a]):
        x, want = voigt["x_" + name], voigt["H_" + name][k]
        got = S.profile(x, a)
        rel = np.abs(got - want) / want
        print(f"a = {a:g}, {name}: largest relative error {rel.max():.3e} at x = {x[rel.argmax()]:.4g} (bound {bound:g})")
        assert rel.max() <= bound
        assert np.array_equal(S.profile(-x, a), got)  # H is even


@pytest.mark.parametrize("k, bound", [(1, 4e-7), (2, 3e-5)])
def test_profile_across_the_small_x_switch(voigt, k, bound):
    a, x, want = float(voigt["a"][k]), voigt["x_switch"], voigt["H_switch"][k]
    assert (x * x < 1e-4).sum() > 100 and (x * x >= 1e-4).sum() > 100
    rel = np.abs(S.profile(x, a) - want) / want
    print(f"a = {a:g}: largest relative error across x^2 = 1e-4 {rel.max():.3e} at x = {x[rel.argmax()]:.4g} (bound {bound:g})")
    assert rel.max() <= bound


def test_doppler_profile():
    x = np.concatenate([np.linspace(0.0, 8.0, 40001), -np.linspace(0.0, 8.0, 4001)])
    x = x[x * x <= 64.0]
    got, want = S.profile(x, 0.0), np.exp(-x * x)
    ulp = np.abs(got - want) / np.spacing(want)
    print(f"a = 0: largest distance from np.exp(-x*x) {ulp.max():.2f} ulp")
    assert ulp.max() <= 4.0
    beyond = np.array([np.nextafter(8.0, 9.0), 8.5, 30.0, 1e3, 1e200, -9.0])
    assert np.array_equal(S.profile(beyond, 0.0), np.zeros(beyond.size))


def test_the_wing_alone_is_the_whole_form_beyond_the_core():
    """what a wavefront without a core evaluates has the bits of the whole form with H0 = 0, up to the cap of x^2"""
    x2 = np.concatenate([np.nextafter(64.0, 65.0) * np.ones(1), np.geomspace(64.0, 1e12, 20001)[1:], np.geomspace(1e12, 2.0 ** 200, 2001)])
    for a in (1e-5, 4.7e-4, 4.7e-3, 0.3):
        w, whole = S.wing(x2, a)
        assert S.same_bits(w, whole) and np.all(w > 0)


# ---- 2. the line against plain numpy

def _random_line(rng, nseg):
    size = 3.0e22 * np.ldexp(1.0, -rng.integers(0, 4, nseg))
    s = np.cumsum(size) - 0.5 * size
    return 10.0 ** rng.uniform(-9, -3, nseg), size, 10.0 ** rng.uniform(3, 5.5, nseg), s, rng.uniform(-2e7, 2e7, nseg)


@pytest.mark.parametrize("nseg, hubble, period", [(1, 0.0, 0.0), (37, 2.3e-18, 0.0), (1000, 2.3e-18, 0.0), (200, 0.0, 6.0e7)])
def test_line_against_numpy(nseg, hubble, period):
    """a = 0: the same formula in the same order with np.exp.  Every term is positive, the header's exponential is within a few ulp of
    np.exp's, and a sequential sum of nseg positive terms loses at most nseg 2^-53: 1e-12 relative per pixel for up to 1000 segments"""
    rng = np.random.default_rng(1000 + nseg)
    dens, size, tgas, s, u = _random_line(rng, nseg)
    nvel, v0, dv = 300, -3.0e7, 2.0e5
    status, tau, summary = S.lines([0, nseg], dens, size, tgas, s, u, nvel, v0, dv, DOPPLER, hubble, period)
    assert status == 0
    want = S.numpy_tau(dens, size, tgas, s, u, nvel, v0, dv, DOPPLER, hubble, period)
    assert (want > 0).sum() > 30 and np.array_equal(tau[0] == 0.0, want == 0.0)
    nz = want > 0
    rel = np.abs(tau[0][nz] - want[nz]) / want[nz]
    print(f"{nseg} segments: largest relative difference {rel.max():.2e}")
    assert rel.max() <= 1e-12
    # the summaries from the header's own tau, recomputed with numpy
    cum = np.cumsum(tau[0])
    p_lo, p_hi = int(np.argmax(cum >= 0.05 * cum[-1])), int(np.argmax(cum >= 0.95 * cum[-1]))
    assert summary[0, 2] == (p_hi - p_lo) * dv
    w = float(np.sum(-np.expm1(-tau[0]) * dv))
    assert abs(summary[0, 1] - w) <= 1e-12 * w
    n = 0.0
    for q in range(nseg):
        n = n + dens[q] * size[q]
    assert summary[0, 0] == n
    assert (summary[0, 1], summary[0, 2]) == S.summarise(tau[0], dv)


# ---- 3. known answers

@pytest.mark.parametrize("ratio", [2.0, 3.0])
def test_the_integral_of_tau_is_n_sigma(ratio):
    """one static segment resolved by b = 2 dv or 3 dv inside a window of at least +-9 b: sum tau dv = N sigma_line (the midpoint rule
    of a Gaussian at this spacing is exact to 1e-16; b = dv would be 3e-5 off, which is why it is not here)"""
    tgas = 1.0e4
    b = thermal_b(tgas)
    dv = b / ratio
    nvel = int(2 * 10 * ratio) + 1
    dens, size = 3.0e-6, 2.0e22
    status, tau, summary = S.lines([0, 1], [dens], [size], [tgas], [0.5 * size], [0.0], nvel, -0.5 * nvel * dv, dv, DOPPLER)
    assert status == 0 and nvel * dv >= 18 * b
    total, want = float(np.sum(tau[0]) * dv), dens * size * DOPPLER[0]
    print(f"b = {ratio:g} dv: sum tau dv / (N sigma) - 1 = {total / want - 1:.2e}")
    assert abs(total - want) <= 1e-12 * want


def test_dv90_of_two_components():
    """two equal components at +-V, V = 40 dv, b = 3 dv: 90 % of the optical depth lies between their outer flanks"""
    tgas = 1.0e4
    dv = thermal_b(tgas) / 3.0
    V, nvel = 40 * dv, 200
    status, tau, summary = S.lines([0, 2], [1e-6, 1e-6], [1e22, 1e22], [tgas, tgas], [0.5e22, 1.5e22], [-V, V], nvel, -0.5 * nvel * dv, dv, DOPPLER)
    assert status == 0
    print(f"dv90 / dv = {summary[0, 2] / dv:g}")
    assert 80.0 <= summary[0, 2] / dv <= 92.0


def test_period_wraps_a_segment():
    tgas, nvel = 2.0e4, 64
    dv = thermal_b(tgas) / 2.5
    v0 = 1.0e6
    args = ([0, 1], [1e-6], [1e22], [tgas], [0.5e22])
    for line in (DOPPLER, S.LYMAN_ALPHA):
        _, wrapped, _ = S.lines(*args, [v0 - 3 * dv], nvel, v0, dv, line, period=nvel * dv)
        _, inside, _ = S.lines(*args, [v0 + (nvel - 3) * dv], nvel, v0, dv, line, period=nvel * dv)
        _, cut, _ = S.lines(*args, [v0 - 3 * dv], nvel, v0, dv, line)
        assert np.all(np.abs(wrapped - inside) <= 1e-13 * inside) and inside[0, -4:].min() > 10 * cut[0, -4:].max()


def test_a_leaf_without_a_line_width_is_refused():
    for tgas, line in ((-1.0, DOPPLER), (float("nan"), DOPPLER), (float("inf"), DOPPLER), (0.0, DOPPLER)):
        status, tau, summary = S.lines([0, 2], [1e-6, 1e-6], [1e22, 1e22], [1e4, tgas], [0.5e22, 1.5e22], [0.0, 0.0], 8, -1e6, 2.5e5, line)
        assert status == 2 and np.all(tau == -7.0) and np.all(summary == -7.0)
    status, _, _ = S.lines([0, 1], [1e-6], [1e22], [0.0], [0.5e22], [0.0], 8, -1e6, 2.5e5, (DOPPLER[0], 0.0, DOPPLER[2], 1e5))
    assert status == 0  # b_turb alone is a width


# ---- 4. geometry

def test_sightlines_are_the_projected_map_columns(refined):
    """for every izone the segment list of each sightline holds the leaves and sizes of the path integral of _analysis.project_map in
    its order: the sequential sums agree bit for bit for two value arrays, and consecutive segments abut along the depth"""
    g, T = refined
    box, shape = float(g["box"]), (13, 11)
    other = np.random.default_rng(7).uniform(0.5, 2.0, g["HI"].size)
    for izone in range(1, 25):
        for centre, zoom in (((0.5, 0.5, 0.5), 1.0), ((0.3, 0.7, 0.9), 2.5)):
            seg = S.Segments(T, box, izone, shape, centre, zoom)
            assert seg.off[-1] == seg.leaf.size and np.all(np.diff(seg.off) >= 1)
            for value in (g["HI"], other):
                out = S.map_lines(seg, value, np.full(value.size, 1e4), None, 1, 0.0, 1e5, DOPPLER)
                want = A.project_map(T, value, g["rho"], box, izone, shape, centre, zoom, mode=1)
                assert np.array_equal(out["N"].astype(np.float32).view(np.uint32), want.view(np.uint32)), izone
            first = np.zeros(seg.leaf.size, dtype=bool)
            first[seg.off[:-1]] = True
            assert np.array_equal(seg.s[first], 0.5 * seg.size[first])
            step = seg.s[1:] - seg.s[:-1]
            gap = np.abs(step - 0.5 * (seg.size[1:] + seg.size[:-1]))  # (s is a rounded product: a few ulp of s)
            assert np.all(gap[~first[1:]] <= 4 * np.spacing(seg.s[1:][~first[1:]]))
            assert np.array_equal(seg.size, box / T.n / 2.0 ** T.level[seg.leaf])


def test_velocity_component_and_sign():
    for izone in range(1, 25):
        src, mirror = A.zone(izone)
        a, mirrored = S.depth_axis(izone)
        assert src[a] == 2 and mirrored == mirror[a]
    assert S.depth_axis(1) == (2, False) and S.depth_axis(3) == (0, False) and S.depth_axis(15) == (0, True)


def test_mirrored_depth_reverses_the_spectrum(refined):
    g, T = refined
    box, shape, nvel, dv = float(g["box"]), (7, 5), 128, 4.0e5
    rng = np.random.default_rng(11)
    vel = [rng.uniform(-1.5e7, 1.5e7, g["HI"].size) for _ in range(3)]
    tgas = 10.0 ** rng.uniform(3.5, 4.5, g["HI"].size)
    pairs = []
    for z1 in range(1, 25):
        for z2 in range(z1 + 1, 25):
            (s1, m1), (s2, m2) = A.zone(z1), A.zone(z2)
            a = s1.index(2)
            if s1 == s2 and m1[a] != m2[a] and all(m1[q] == m2[q] for q in range(3) if q != a):
                pairs.append((z1, z2))
    assert len(pairs) >= 4
    for z1, z2 in pairs:
        for line in (DOPPLER, S.LYMAN_ALPHA):
            one = S.map_lines(S.Segments(T, box, z1, shape), g["HI"], tgas, vel, nvel, -0.5 * nvel * dv, dv, line)
            two = S.map_lines(S.Segments(T, box, z2, shape), g["HI"], tgas, vel, nvel, -0.5 * nvel * dv, dv, line)
            assert one["tau"].max() > 0 and not np.array_equal(one["tau"], one["tau"][:, :, ::-1])
            assert np.all(np.abs(two["tau"] - one["tau"][:, :, ::-1]) <= 1e-13 * one["tau"][:, :, ::-1])


def test_uniform_segments_are_the_walk_of_a_uniform_tree():
    """what the GPU test of a 257^3 grid takes for its segments, at a size the Tree can be built at"""
    n, box = 16, 2.5e24
    T = A.Tree(n, np.zeros(n ** 3, dtype=np.int64))
    vel = [np.random.default_rng(q).uniform(-1e7, 1e7, n ** 3) for q in range(3)]
    for izone in (1, 5, 8, 15, 24):
        for shape, centre, zoom in (((3, 2), (0.5, 0.5, 0.5), 1.0), ((7, 5), (0.5, 0.5, 0.5), 1.0), ((13, 11), (0.3, 0.7, 0.9), 2.5)):
            want, got = S.Segments(T, box, izone, shape, centre, zoom), S.uniform_segments(n, box, izone, shape, centre, zoom)
            assert got.shape == want.shape and got.npix == want.npix and got.izone == want.izone
            for key in ("off", "leaf", "size", "s"):
                a, b = getattr(got, key), getattr(want, key)
                assert a.dtype == b.dtype and np.array_equal(a, b), (izone, shape, key)
            assert np.array_equal(got.velocity(vel), want.velocity(vel)) and np.array_equal(got.velocity(None), want.velocity(None))
            assert np.array_equal(S.line_counts(got), S.line_counts(want))
    assert np.diff(S.uniform_segments(n, box, 3, (13, 11), (0.3, 0.7, 0.9), 2.5).off).max() < n  # (the zoomed window is shallower)


def test_deep_levels_give_the_wanted_counts():
    """the trees of the GPU tests' chunk edges: the counts asked for, at the columns asked for, under the two izones they are for"""
    columns = {(1, 2): 512, (2, 1): 513, (0, 3): 1027, (3, 3): 4, (0, 0): 9}
    level = S.deep_levels(4, columns)
    T = A.Tree(4, level)
    for izone in (1, 5):
        counts = np.diff(S.Segments(T, 3.0e24, izone, (4, 4)).off).reshape(4, 4)
        for i in range(4):
            for j in range(4):
                at = (i, j) if izone == 1 else (j, i)  # (izone 5: map axis i is storage j)
                assert counts[i, j] == columns.get(at, 4), (izone, i, j)
    assert S.line_counts(S.Segments(T, 3.0e24, 1, (4, 4)))[1 + 4 * 2] == 512


# ---- 5. the batch rule

BATCH_CASES = [((4096, 70, False, 1027), 2040), ((4096, 70, True, 1027), 2006), ((65536, 1024, True, 512), 8168), ((100, 1024, True, 4), 100),
               ((5, 1 << 24, True, 4), 1), ((0, 1024, True, 4), 1), ((4608, 4096, True, 4), 2046), ((1280, 16384, True, 4), 511)]


def _batch_check(tmp_path, flags, name):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / name)
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    subprocess.check_call([gxx, *flags, "-I" + os.path.join(S.ROOT, "tests", "host", "stub"), "-I" + S.CSRC,
                           os.path.join(S.ROOT, "tests", "host", "spectra_batch_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitized", [False, True])
def test_batch_rule(tmp_path, sanitized):
    """ftte::spectra_batch_lines as a program of its own (tests/host/spectra_batch_check.cpp): its known values and its property;
    and the restatement the GPU tests place their seams by, against the same values and against the function over random arguments"""
    exe = _batch_check(tmp_path, S.SANITIZE if sanitized else ["-std=c++17", "-O2", "-Wall", "-Werror"], "batch")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "spectra batch rule: ok" in res.stdout and "ERROR" not in res.stderr, res.stdout[-2000:] + res.stderr[-4000:]
    for args, want in BATCH_CASES:
        assert S.batch_lines(*args) == want, args
    assert [b[1] for b in S.batches(4096, 70, False, 1027)] == [2040, 2040, 16] and [b[1] for b in S.batches(4096, 70, True, 1027)] == [2006, 2006, 84]
    assert S.batches(4608, 4096, True, 4) == [(0, 2046), (2046, 2046), (4092, 516)]
    rng = np.random.default_rng(26)
    rows = [(int(rng.integers(0, 100000)), int(rng.integers(0, 40000)), int(rng.integers(0, 2)), int(rng.integers(0, 3000))) for _ in range(300)]
    rows += [(int(rng.integers(0, 40)), int(rng.integers(0, 1 << 25)), 1, int(rng.integers(0, 4000000))) for _ in range(60)]
    rows += [(n, v, t, m) for n in (1, 7, 65536) for v in (1, 1024) for t in (0, 1) for m in (511, 512, 513)]
    case = tmp_path / "rows.txt"
    case.write_text("".join("%d %d %d %d\n" % r for r in rows))
    res = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "ERROR" not in res.stderr, res.stderr[-4000:]
    got = [int(v) for v in res.stdout.split()]
    assert got == [S.batch_lines(n, v, bool(t), m) for n, v, t, m in rows]
    assert len({g == r[0] for g, r in zip(got, rows)}) == 2 and 1 in got  # whole maps, cut maps and single lines among them


# ---- 6. under the sanitizers

def test_statement_under_the_sanitizers(refined, golden, tmp_path):
    """tests/host/spectra_check.cpp's main() over the goldens' segment lists, with AddressSanitizer and UBSan, as a program of its own"""
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    g, T = refined
    ing = golden("ingest6_three_levels_metals_velocities")
    Ti = A.Tree(int(ing["out_n"]), ing["out_level"])
    off, cols = [np.zeros(1, dtype=np.int64)], [[] for _ in range(5)]
    rng = np.random.default_rng(3)
    for tree, box, dens, tgas, vel, izones in (
            (T, float(g["box"]), g["HI"], 10.0 ** rng.uniform(3.5, 5.0, g["HI"].size), [rng.uniform(-1e7, 1e7, g["HI"].size)] * 3, (1, 8, 15, 24)),
            (Ti, float(ing["out_box"]), ing["out_HI"], ing["out_tgas"], [1e5 * ing["out_vel" + c] for c in "xyz"], (2, 13, 21))):
        for izone in izones:
            seg = S.Segments(tree, box, izone, (13, 11))
            off.append(off[-1][-1] + seg.off[1:])
            for col, a in zip(cols, (dens[seg.leaf], seg.size, tgas[seg.leaf], seg.s, seg.velocity(vel))):
                col.append(np.asarray(a, dtype=np.float64))
    off = np.concatenate(off)
    case = tmp_path / "segments.bin"
    with open(case, "wb") as f:
        f.write(np.array([off.size - 1], "<i8").tobytes())
        f.write(off.astype("<i8").tobytes())
        for col in cols:
            f.write(np.concatenate(col).astype("<f8").tobytes())
    exe = str(tmp_path / "spectra_check")
    subprocess.check_call([gxx, *S.SANITIZE, "-DSPECTRA_CHECK_MAIN", "-I" + S.CSRC, S.SOURCE, "-o", exe])
    for args in ([exe, str(case)], [exe]):
        res = subprocess.run(args, capture_output=True, text=True, timeout=600)
        print(res.stdout[-2000:])
        assert res.returncode == 0 and "sightline spectra under the sanitizers: ok" in res.stdout, res.stdout[-4000:] + res.stderr[-4000:]
