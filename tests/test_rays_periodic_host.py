"""The periodic ray walk of csrc/ftte_ray_math.h on the host (g++ through tests/_rays_periodic.py; no GPU): against the brute-force
intersection of a ray with every leaf's box in every image of the box it can reach, on fixed-seed random rays and on the named ones
over a uniform grid, a grid with a corner refined two levels and the three-level ingest golden; axis rays of three boxes against
three shifted copies of the walk that ends at the box, bit for bit; the body diagonal over two boxes; a ray that ends before its
first wrap against the non-periodic ray; origins 1 000 boxes away; the bound and the refusals; the walk under the sanitizers as a
program of its own; and the entry points where hosts look for them."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _analysis as A
import _rays as R
import _rays_periodic as P
import _spectra as S

SYMBOLS = ["ftte_ray_spectra_periodic", "ftte_ray_spectra_periodic_device", "ftte_ray_segments_periodic"]


def corner_levels(n=4):
    """base cell 0 refined, its first child refined again"""
    return np.array([2] * 8 + [1] * 7 + [0] * (n ** 3 - 1), dtype=np.int32)


@pytest.fixture(scope="module")
def trees(golden):
    g = golden("ingest6_three_levels_metals_velocities")
    out = {"uniform": A.Tree(4, np.zeros(64, dtype=np.int32)), "corner": A.Tree(4, corner_levels()), "ingest": A.Tree(int(g["out_n"]), g["out_level"])}
    return {k: (t, R.leaf_boxes(t)) for k, t in out.items()}


def _compare_all(walk, boxes):
    segments = tiny = 0
    worst = 0.0
    for r in range(walk.nray):
        s, t, w = P.compare(walk, boxes, r)
        segments, tiny, worst = segments + s, tiny + t, max(worst, w)
    return segments, tiny, worst


@pytest.mark.parametrize("name", ["uniform", "corner", "ingest"])
def test_random_rays_against_the_brute_force(trees, name):
    """2 000 rays with origins inside and up to a box outside, lengths up to 5 boxes, every tenth with one zero component"""
    tree, boxes = trees[name]
    o, d, tmax = P.random_rays(tree.n, 2000, seed=tree.ncell)
    assert (d[::10] == 0.0).sum() == 200 and tmax.max() > 4.5 * tree.n and o.min() < -0.5 * tree.n and o.max() > 1.5 * tree.n
    walk = P.Walk(tree, o, d, tmax)
    segments, tiny, worst = _compare_all(walk, boxes)
    bound = np.array([P.step_bound(tree.n, tree.max_level, t) for t in tmax])
    print(f"{name}: {segments} segments, {tiny} tiny, largest difference {worst:.3e} cells, at most {walk.steps.max()} steps, least bound {bound.min()}")
    assert tiny <= 0.01 * segments and segments > 5 * 2000
    assert np.all(walk.steps <= bound) and np.all(np.diff(walk.off) >= 1)


@pytest.mark.parametrize("name", ["uniform", "corner", "ingest"])
def test_named_rays_against_the_brute_force(trees, name):
    tree, boxes = trees[name]
    cases = P.named_rays(tree.n)
    for what, o, d, tmax in cases:
        assert R.arguments_ok(o, d, tmax) and P.refusal(o, tmax, tree.n) == 0, what
    walk = P.Walk(tree, [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
    segments, tiny, worst = _compare_all(walk, boxes)
    print(f"{name}: {segments} segments, {tiny} tiny, largest difference {worst:.3e} cells")
    assert tiny <= 0.01 * segments
    count = dict(zip([c[0] for c in cases], np.diff(walk.off)))
    assert count["a tmax shorter than the first leaf"] == 1
    for what in ("in a face plane", "along a box edge", "on the box's face, outwards", "negative zeros", "a tmax on a box face"):
        assert count[what] >= int(cases[[c[0] for c in cases].index(what)][3]), what  # at least a leaf per base cell of length


@pytest.mark.parametrize("name", ["uniform", "corner", "ingest"])
def test_axis_rays_repeat_the_one_box_list_bit_for_bit(trees, name):
    """all six +-e_a over 3 n from the box's face: three copies of the non-periodic list, t shifted by exactly j n"""
    tree, _ = trees[name]
    n = tree.n
    cases = P.axis_rays(n, 3)
    once = R.Walk(tree, [c[1] for c in cases], [c[2] for c in cases])
    thrice = P.Walk(tree, [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
    for r, case in enumerate(cases):
        leaf, a, b = once.of(r)
        assert leaf.size >= n and a[0] == 0.0 and b[-1] == float(n), case[0]
        got = thrice.of(r)
        assert np.array_equal(got[0], np.tile(leaf, 3)), case[0]
        assert S.same_bits(got[1], np.concatenate([a + j * float(n) for j in range(3)])), case[0]
        assert S.same_bits(got[2], np.concatenate([b + j * float(n) for j in range(3)])), case[0]


def test_the_body_diagonal_over_two_boxes_crosses_the_diagonal_leaves_only(trees):
    """every crossing is a three-way tie, the box's corner included: the wraps on the three axes follow each other through cells
    that give nothing"""
    n = 4
    for name in ("uniform", "corner"):
        tree, (lo, h) = trees[name]
        r3 = 1.0 / np.sqrt(3.0)
        length = P.diagonal_length(n)
        walk = P.Walk(tree, [(0, 0, 0), (n, n, n)], [(r3, r3, r3), (-r3, -r3, -r3)], [length, length])
        once = R.Walk(tree, [(0, 0, 0)], [(r3, r3, r3)]).of(0)[0]
        on_diagonal = np.nonzero((lo[:, 0] == lo[:, 1]) & (lo[:, 1] == lo[:, 2]))[0]
        assert sorted(once.tolist()) == sorted(on_diagonal.tolist())
        forth, back = walk.of(0)[0], walk.of(1)[0]
        assert np.array_equal(forth, np.tile(once, 2)) and np.array_equal(back, forth[::-1]), name
        assert walk.of(0)[2][-1] == length and walk.of(1)[2][-1] == length


def test_before_the_first_wrap_a_periodic_ray_is_the_non_periodic_ray(trees):
    """origins inside the box, a tmax that ends before the box does: the same bits"""
    for name, (tree, _) in trees.items():
        o, d, _ = R.random_rays(tree.n, 600, seed=600)
        o = np.random.default_rng(601).uniform(0.0, tree.n, o.shape)
        to_far_side = R.Walk(tree, o, d)
        tmax = np.random.default_rng(602).uniform(0.05, 0.999, 600) * to_far_side.start[:, 1]
        assert np.all(to_far_side.start[:, 0] == 0.0) and np.all(tmax > 0)
        want, got = R.Walk(tree, o, d, tmax), P.Walk(tree, o, d, tmax)
        assert np.array_equal(got.off, want.off) and np.array_equal(got.leaf, want.leaf), name
        assert S.same_bits(got.t_in, want.t_in) and S.same_bits(got.t_out, want.t_out), name
        assert want.leaf.size > 600


def test_image_and_local_origin():
    n = 4
    up, down, none = (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    for o, d, w, local in ((0.5, up, 0, 0.5), (4.0, up, 1, 0.0), (4.0, down, 0, 4.0), (4.0, none, 1, 0.0), (0.0, down, -1, 4.0), (0.0, up, 0, 0.0), (-0.0, down, -1, 4.0),
                           (-8.0, down, -3, 4.0), (-8.0, up, -2, 0.0), (4000.5, up, 1000, 0.5), (-3999.75, down, -1000, 0.25), (-0.25, up, -1, 3.75), (9.5, none, 2, 1.5)):
        got_w, got_local = P.image(n, (o, 0.5, 0.5), d)
        assert got_w[0] == w and got_local[0] == local, (o, d, got_w, got_local)
        assert got_w[1] == 0 and got_local[1] == 0.5
    # rounded: the local origin is the caller's coordinate minus w n in one rounding, inside [0, n]
    for o in (4000.3, -3999.3, -1e-300, np.nextafter(4.0, 0.0), np.nextafter(-4.0, 0.0)):
        w, local = P.image(n, (o, 0.5, 0.5), up)
        assert w[0] == np.floor(o / n) and 0.0 <= local[0] <= n and abs(local[0] - (o - w[0] * n)) <= 1e-12, (o, w, local)


def test_far_origins(trees):
    """1 000 boxes away: the segments are those of the ray moved 1 000 boxes back where o' is exact, bit for bit"""
    tree, boxes = trees["corner"]
    n = tree.n
    d = R.unit([(1.0, -1.0, 0.5)])[0]
    near, far = (0.5, 0.25, 0.375), (1000.0 * n + 0.5, -1000.0 * n + 0.25, 0.375)
    a, b = P.Walk(tree, [near], [d], [4.0 * n]), P.Walk(tree, [far], [d], [4.0 * n])
    assert np.array_equal(a.leaf, b.leaf) and S.same_bits(a.t_in, b.t_in) and S.same_bits(a.t_out, b.t_out) and a.leaf.size > 12
    P.compare(b, boxes, 0)
    c = P.Walk(tree, [(1000.0 * n + 0.3, -1000.0 * n + 0.6, -0.45)], [d], [4.0 * n])  # rounded: its own brute force holds
    P.compare(c, boxes, 0)


def test_nothing_drifts_over_a_thousand_boxes(trees):
    """+-e_0 from x = 0.3 over 1 000 boxes: every t_out against the exact F - 0.3 (rationals) within the two roundings the statement
    takes -- o' = o - w n from the caller's o and the integer image, then far - o' -- that is 2^-53 (|o'| + t) <= 2^-52 (t + n); and,
    from 0.3 and 40 random x, bit for bit the statement's own expression with o' in one rounding from the caller's o."""
    from fractions import Fraction
    tree, _ = trees["uniform"]
    n, boxes = tree.n, 1000
    k = np.arange(boxes * n)
    for x in [0.3] + np.random.default_rng(1000).uniform(0.0, 1.0, 40).tolist():
        for sign in (1.0, -1.0):
            walk = P.Walk(tree, [(x, 0.5, 0.5)], [(sign, 0.0, 0.0)], [float(boxes * n)])
            t_out = walk.of(0)[2]
            assert t_out.size == boxes * n + 1 and t_out[-1] == boxes * n
            w, far = (k // n, k % n + 1.0) if sign > 0 else (np.where(k == 0, 0, -1 - (k - 1) // n), np.where(k == 0, 0.0, n - 1.0 - (k - 1) % n))
            assert S.same_bits(t_out[:-1], (far - (x - w.astype(np.float64) * n)) * (1.0 / sign)), (x, sign)
            if x == 0.3:
                first = Fraction(1) - Fraction(x) if sign > 0 else Fraction(x)
                worst = max(abs(Fraction(float(t)) - (first + q)) / (Fraction(float(t)) + n) for q, t in enumerate(t_out[:-1]))
                print(f"d = {sign:+.0f} e_0: largest error {float(worst) * 2 ** 52:.3f} of the bound")
                assert worst <= Fraction(1, 2 ** 52)


def test_the_bound_and_the_refusals():
    assert P.step_bound(4, 0, 4.0) == 27 and P.step_bound(4, 0, 4.1) == 39 and P.step_bound(4, 2, 20.0) == 3 * 16 * 6 + 3 and P.step_bound(6, 3, 0.01) == 3 * 48 * 2 + 3
    assert P.step_bound(4, 40, 4.0) > 0 and P.step_bound(4, 41, 4.0) == 0                       # a tree deeper than 40 levels
    assert P.step_bound(4, 0, 4.0 * 2.0 ** 20) > 0 and P.step_bound(4, 0, 4.0 * 2.0 ** 20 + 1.0) == 0  # tmax / n above 2^20
    assert P.step_bound(2 ** 20, 40, 4.0) == 0 and P.step_bound(2 ** 10, 35, 2.0 ** 29) == 0   # the product beyond 2^62
    assert P.step_bound(4, 0, 0.0) == 0 and P.step_bound(4, 0, -1.0) == 0 and P.step_bound(4, 0, float("nan")) == 0
    good = (0.5, 0.5, 0.5)
    assert P.refusal(good, 1.0, 4) == 0 and P.refusal(good, None, 4) == 1 and P.refusal(good, 0.0, 4) == 1 and P.refusal(good, -2.0, 4) == 1
    assert P.refusal((0.5, -4.0 * 2.0 ** 20, 0.5), 1.0, 4) == 0 and P.refusal((0.5, -4.0 * 2.0 ** 20 - 1.0, 0.5), 1.0, 4) == 2
    assert not R.arguments_ok(good, (0.0, 0.0, 1.0), float("inf"))  # (a tmax that is not finite is the non-periodic refusal)


def test_walk_under_the_sanitizers(tmp_path):
    """tests/host/ray_periodic_check.cpp as a program with -fsanitize=address,undefined: the named cases and random rays over a
    uniform and a refined grid"""
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "ray_periodic_check")
    subprocess.check_call([gxx, *R.SANITIZE, "-DRAY_PERIODIC_CHECK_MAIN", "-I" + R.CSRC, P.SOURCE, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:])
    assert res.returncode == 0 and "periodic ray walk under the sanitizers: ok" in res.stdout, res.stdout[-4000:] + res.stderr[-4000:]


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
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_periodic", "")]


def test_null_context_is_an_argument_error():
    from radiativetransfer_amd import _lib
    lib = _lib.load()
    assert _lib.STATUS[lib.ftte_ray_spectra_periodic(None, 1, None, None, None, 8, 0.0, 1.0, 0.0, 0.0, None, None, None, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_ray_spectra_periodic_device(None, 1, None, None, None, 8, 0.0, 1.0, 0.0, 0.0, None, None, None, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_ray_segments_periodic(None, 1, None, None, None, None, 0, None, None, None)] == "FTTE_ERR_ARG"


def test_python_surface():
    import radiativetransfer_amd as rt
    for f in (rt.StellarTransfer.ray_spectra, rt.StellarTransfer.ray_segments):
        assert inspect.signature(f).parameters["periodic"].default is False
    with pytest.raises(ValueError):
        rt.StellarTransfer._rays([(0.5, 0.5, 0.5)], [(0.0, 0.0, 1.0)], None, True)
    assert "wrap" in _read("include", "ftte.h") and "No periodic wrap of a ray" not in _read("include", "ftte.h")
