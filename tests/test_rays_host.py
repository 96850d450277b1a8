"""The ray walk of csrc/ftte_ray_math.h on the host (g++ through tests/_rays.py; no GPU): against the brute-force intersection of a
ray with every leaf's box, on the named rays and on fixed-seed random ones over a uniform grid, a grid with a corner refined two
levels and the three-level ingest golden; axis-aligned rays against the segments of the sightline spectra bit for bit under all 24
izones; the host's batch rule (csrc/ftte_rays.h, against a stub of the HIP runtime) with the tests' restatement of it; the walk
under the sanitizers as a program of its own; and the entry points where hosts look for them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _analysis as A
import _rays as R
import _spectra as S

SYMBOLS = ["ftte_ray_spectra", "ftte_ray_spectra_device", "ftte_ray_segments"]


def corner_levels(n=4):
    """base cell 0 refined, its first child refined again"""
    return np.array([2] * 8 + [1] * 7 + [0] * (n ** 3 - 1), dtype=np.int32)


@pytest.fixture(scope="module")
def trees(golden):
    g = golden("ingest6_three_levels_metals_velocities")
    out = {"uniform": A.Tree(4, np.zeros(64, dtype=np.int32)), "corner": A.Tree(4, corner_levels()), "ingest": A.Tree(int(g["out_n"]), g["out_level"])}
    return {k: (t, R.leaf_boxes(t)) for k, t in out.items()}


def test_leaf_boxes_fill_the_box(trees):
    for name, (tree, (lo, h)) in trees.items():
        assert abs((h ** 3).sum() - tree.n ** 3) < 1e-9 and np.array_equal(h, np.ldexp(1.0, -tree.level)), name
        assert lo.min() == 0.0 and (lo + h[:, None]).max() == tree.n


@pytest.mark.parametrize("name", ["uniform", "corner", "ingest"])
def test_named_rays_against_the_brute_force(trees, name):
    tree, boxes = trees[name]
    cases = R.named_rays(tree.n)
    walk = R.Walk(tree, [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
    segments = tiny = 0
    worst = 0.0
    for r, case in enumerate(cases):
        assert R.arguments_ok(case[1], case[2], case[3]), case[0]
        s, t, w = R.compare(walk, boxes, r)
        segments, tiny, worst = segments + s, tiny + t, max(worst, w)
    print(f"{name}: {segments} segments, {tiny} tiny, largest difference {worst:.3e} cells")
    assert tiny <= 0.01 * segments
    count = dict(zip([c[0] for c in cases], np.diff(walk.off)))
    for what in ("a miss", "pointing away", "a miss on an axis without direction", "a tmax before the box", "on the far face, outwards"):
        assert count[what] == 0, what
    for what in ("the body diagonal", "in a face plane", "along an edge", "a tmax inside a leaf", "an origin inside a deepest leaf", "negative zeros"):
        assert count[what] > 0, what
    assert all(count[f"{s}e_{a}"] >= tree.n for s in "+-" for a in range(3))


def test_the_body_diagonal_crosses_the_diagonal_leaves_only(trees):
    """every crossing is a three-way tie: the two cells between get chords of exactly 0 and give nothing"""
    n = 4
    for name, want in (("uniform", [(i * n + i) * n + i for i in range(n)]), ("corner", None)):
        tree, (lo, h) = trees[name]
        r3 = 1.0 / np.sqrt(3.0)
        walk = R.Walk(tree, [(0, 0, 0), (n, n, n)], [(r3, r3, r3), (-r3, -r3, -r3)])
        on_diagonal = np.nonzero((lo[:, 0] == lo[:, 1]) & (lo[:, 1] == lo[:, 2]))[0]
        forth, back = walk.of(0)[0], walk.of(1)[0]
        assert sorted(forth.tolist()) == sorted(on_diagonal.tolist()) and np.array_equal(forth, back[::-1]), name
        assert np.array_equal(lo[forth, 0], np.sort(lo[forth, 0]))
        if want is not None:
            assert forth.tolist() == [tree.leaf[v] for v in want]
    assert R.lib().ry_step_bound(4, 0) == 15 and R.lib().ry_step_bound(6, 2) == 75 and R.lib().ry_step_bound(4, 41) == 0


def test_ties_go_to_the_lowest_axis(trees):
    """the tied axes' t's are the same expression, so the tie is exact; the segments do not show which axis took it (the cells
    between give chords of 0), the exit axis does"""
    r3, r2 = 1.0 / np.sqrt(3.0), 1.0 / np.sqrt(2.0)
    for name in ("uniform", "corner"):
        tree = trees[name][0]
        for o, d, want in (((0, 0, 0), (r3, r3, r3), 0), ((4, 4, 4), (-r3, -r3, -r3), 0), ((0.5, 0, 0), (0.0, r2, r2), 1), ((0, 0.5, 0), (r2, 0.0, r2), 0),
                           ((0, 0, 0.5), (r2, r2, -0.0), 0), ((3.0, 3.5, 3.0), (-r2, 0.0, -r2), 0), ((0.2, 0.1, 0.1), (r3, r3, r3), 0),
                           ((0.1, 0.2, 0.1), (r3, r3, r3), 1), ((0.1, 0.1, 0.2), (r3, r3, r3), 2), ((0.5, 0.5, 0.5), (0.0, 0.0, -1.0), 2)):
            axis, t = R.first_exit(tree, o, d)
            assert axis == want and t > 0, (name, o, d, axis)
    assert R.first_exit(trees["uniform"][0], (-1.0, 5.0, 0.5), (1.0, 0.0, 0.0))[0] == -1


@pytest.mark.parametrize("name", ["uniform", "corner", "ingest"])
def test_random_rays_against_the_brute_force(trees, name):
    """2 000 rays with origins inside and outside the box; none of them has a leaf below the threshold in either list"""
    tree, boxes = trees[name]
    o, d, tmax = R.random_rays(tree.n, 2000, seed=tree.ncell)
    walk = R.Walk(tree, o, d, tmax)
    segments = tiny = hits = 0
    worst = 0.0
    for r in range(o.shape[0]):
        s, t, w = R.compare(walk, boxes, r)
        segments, tiny, worst, hits = segments + s, tiny + t, max(worst, w), hits + (s > 0)
    print(f"{name}: {segments} segments on {hits} rays, {tiny} tiny, largest difference {worst:.3e} cells")
    assert tiny == 0 and 500 < hits < 2000 and segments > 2 * hits  # (a mean of some three leaves a ray across four cells)


def test_the_refusals():
    good = (0.0, 0.0, 1.0)
    assert R.arguments_ok((1, 2, 3), good) and R.arguments_ok((1, 2, 3), (-0.0, 0.0, -1.0), -5.0)
    assert R.arguments_ok((1, 2, 3), (0.0, 0.0, 1.0 + 4e-10)) and not R.arguments_ok((1, 2, 3), (0.0, 0.0, 1.0 + 6e-10))
    for bad in (np.nan, np.inf, -np.inf):
        assert not R.arguments_ok((bad, 2, 3), good) and not R.arguments_ok((1, 2, 3), (0.0, bad, 1.0)) and not R.arguments_ok((1, 2, 3), good, bad)
    assert not R.arguments_ok((1, 2, 3), (0, 0, 0)) and not R.arguments_ok((1, 2, 3), (1, 1, 1))


# ---- axis-aligned rays are the sightline spectra's pixel columns

@pytest.mark.parametrize("window", [((0.5, 0.5, 0.5), 1.0), ((0.1, 0.93, 0.95), 3.0)])
def test_axis_aligned_rays_equal_the_sightlines(trees, golden, window):
    """all 24 izones, a 13 x 11 map (its middle column lies on a face between base cells): the leaves, and size and s with equal bits"""
    tree, _ = trees["ingest"]
    box = float(golden("ingest6_three_levels_metals_velocities")["out_box"])
    rng = np.random.default_rng(24)
    vel = [rng.uniform(-2e7, 2e7, tree.ncell) for _ in range(3)]
    centre, zoom = window
    for izone in range(1, 25):
        seg = S.Segments(tree, box, izone, (13, 11), centre, zoom)
        walk = R.Walk(tree, *R.axis_rays(tree, izone, (13, 11), centre, zoom))
        assert np.array_equal(walk.off, seg.off) and np.array_equal(walk.leaf, seg.leaf), izone
        size, s, u = walk.line_inputs(box, vel)
        assert S.same_bits(size, seg.size) and S.same_bits(s, seg.s) and S.same_bits(u, seg.velocity(vel)), izone
        size, s, u = walk.line_inputs(box, None)
        assert S.same_bits(u, seg.velocity(None))


# ---- the batch rule

def _batch_check(tmp_path, flags, name):
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / name)
    # the stub's directory comes first: <hip/hip_runtime_api.h> is the stub even where ROCm is installed
    subprocess.check_call([gxx, *flags, "-I" + os.path.join(R.ROOT, "tests", "host", "stub"), "-I" + R.CSRC,
                           os.path.join(R.ROOT, "tests", "host", "ray_batch_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitized", [False, True])
def test_batch_rule(tmp_path, sanitized):
    """ftte::ray_batch_rays as a program of its own (tests/host/ray_batch_check.cpp): its known values and its property; and the
    restatement the GPU tests place their seams by, against the same values and against the function over random counts"""
    exe = _batch_check(tmp_path, R.SANITIZE if sanitized else ["-std=c++17", "-O2", "-Wall", "-Werror"], "batch")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "ray batch rule: ok" in res.stdout and "ERROR" not in res.stderr, res.stdout[-2000:] + res.stderr[-4000:]
    prefix = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)  # noqa: E731
    assert [b[1] for b in R.batches(prefix([4] * 4608), 4096, True)] == [2038, 2038, 532]
    assert [b[1] for b in R.batches(prefix([4] * 4608), 4096, False)] == [4608]
    assert [b[1] for b in R.batches(prefix([10, 3000000, 10, 10]), 64, True)] == [1, 1, 2]
    assert [b[1] for b in R.batches(prefix([1000000] * 3), 0, False, R.LIST_BYTES)] == [2, 1]
    rng = np.random.default_rng(5)
    rows = []
    for q in range(60):
        nray = int(rng.integers(1, 3000))
        counts = rng.integers(0, 40000 if q % 4 else 2000000, nray)
        rows.append((int(rng.integers(0, 30000)), int(q % 2), (R.RECORD_BYTES, R.LIST_BYTES)[q % 3 == 0], counts))
    case = tmp_path / "rows.txt"
    case.write_text("".join(f"{nvel} {stage} {per} {c.size} {' '.join(map(str, c))}\n" for nvel, stage, per, c in rows))
    res = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    answers = [[int(v) for v in line.split()] for line in res.stdout.splitlines()]
    assert len(answers) == len(rows)
    for (nvel, stage, per, counts), got in zip(rows, answers):
        assert [b[1] for b in R.batches(prefix(counts), nvel, bool(stage), per)] == got
    assert max(len(a) for a in answers) > 2 and min(len(a) for a in answers) == 1


def test_walk_under_the_sanitizers(tmp_path):
    """tests/host/ray_check.cpp as a program with -fsanitize=address,undefined: the named rays and random ones over a uniform and a
    refined grid"""
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "ray_check")
    subprocess.check_call([gxx, *R.SANITIZE, "-DRAY_CHECK_MAIN", "-I" + R.CSRC, R.SOURCE, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:])
    assert res.returncode == 0 and "ray walk under the sanitizers: ok" in res.stdout, res.stdout[-4000:] + res.stderr[-4000:]


# ---- the entry points exist everywhere a host reaches them

def _read(*parts):
    with open(os.path.join(R.ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_named_where_hosts_look(name):
    lib = C.CDLL(os.path.join(R.ROOT, "radiativetransfer_amd", "libftte.so"))
    assert getattr(lib, name) is not None
    assert re.search(r"^\s*%s;" % name, _read("radiativetransfer_amd", "csrc", "ftte.map"), re.M)
    assert re.search(r"^int %s\(" % name, _read("include", "ftte.h"), re.M)
    assert "bind(C, name='%s')" % name in _read("fortran", "ftte_binding.f90")
    from radiativetransfer_amd import _lib
    assert name in _lib.SIGNATURES


def test_null_context_is_an_argument_error():
    from radiativetransfer_amd import _lib
    lib = _lib.load()
    assert _lib.STATUS[lib.ftte_ray_spectra(None, 1, None, None, None, 8, 0.0, 1.0, 0.0, 0.0, None, None, None, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_ray_spectra_device(None, 1, None, None, None, 8, 0.0, 1.0, 0.0, 0.0, None, None, None, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_ray_segments(None, 1, None, None, None, None, 0, None, None, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[-16] == "FTTE_ERR_INTERNAL" and "FTTE_ERR_INTERNAL = -16" in _read("include", "ftte.h")


def test_python_surface():
    import radiativetransfer_amd as rt
    assert callable(rt.StellarTransfer.ray_spectra) and callable(rt.StellarTransfer.ray_segments)
