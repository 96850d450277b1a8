"""The oblique rays on the GPU against the g++ evaluation of csrc/ftte_ray_math.h and csrc/ftte_spectra_math.h (tests/_rays.py; held
against the brute-force intersection by test_rays_host.py): the segment lists bit for bit on every host case; tau, N, W and dv90 bit
for bit on the ingest golden and a uniform grid; axis-aligned rays against sightline_spectra on the same context; rays at and around
every chunk edge over one and three passes of pixels beside an oblique ray through the same deep column; three batches by tau
alone; the _device variant, absent outputs, a missing ray between hitting ones, the refusals, the owner."""
import ctypes as C

import numpy as np
import pytest

import _analysis as A
import _rays as R
import _spectra as S
import radiativetransfer_amd as rt

pytestmark = pytest.mark.gpu

LYA = rt.LYMAN_ALPHA
DOPPLER = (LYA[0], 0.0, LYA[2], 0.0)
VSCALE = 1.0e5  # as test_spectra_gpu.py: the golden's velocities times this spread over +-3e7 cm/s
KEYS = ("tau", "N", "W", "dv90")


@pytest.fixture(scope="module")
def stellar():
    st = rt.StellarTransfer()
    yield st
    st.close()


@pytest.fixture(scope="module")
def ingest(golden):
    g = golden("ingest6_three_levels_metals_velocities")
    case = dict(n=int(g["out_n"]), level=g["out_level"], box=float(g["out_box"]), HI=g["out_HI"], tgas=g["out_tgas"], rho=g["out_rho"],
                vel=[VSCALE * g["out_vel" + c] for c in "xyz"])
    case["tree"] = A.Tree(case["n"], case["level"])
    return case


def load(st, case, velocity=True):
    st.set_grid(case["n"], case["level"], case["box"])
    st.set_medium(case["HI"], case["HI"], case["HI"], case.get("rho"), None, 0)  # (the helium species are not read)
    st.set_temperature(case["tgas"])
    if velocity:
        st.set_velocity(*case["vel"])


def assert_same(got, want, what="", keys=KEYS):
    for key in keys:
        assert S.same_bits(got[key], want[key]), f"{what}: {key} differs, largest relative difference " \
            f"{np.nanmax(np.abs(got[key] - want[key]) / np.maximum(np.abs(want[key]), 1e-300)):.3e}"


def assert_same_segments(got, walk, what=""):
    assert np.array_equal(got["offset"], walk.off), what
    assert np.array_equal(got["leaf"], walk.leaf), what
    assert S.same_bits(got["t_in"], walk.t_in) and S.same_bits(got["t_out"], walk.t_out), what


# ---- the segment lists

@pytest.mark.parametrize("name", ["uniform", "corner", "ingest"])
def test_segments_are_the_host_walk(stellar, ingest, name):
    """the named rays and the 2 000 random ones of test_rays_host.py: offsets, leaves, t_in and t_out bit for bit; needs a grid only"""
    level = {"uniform": np.zeros(64, dtype=np.int32), "corner": np.array([2] * 8 + [1] * 7 + [0] * 63, dtype=np.int32), "ingest": ingest["level"]}[name]
    n = ingest["n"] if name == "ingest" else 4
    tree = A.Tree(n, level)
    stellar.set_grid(n, level, 3.0e24)
    cases = R.named_rays(n)
    o, d, tmax = R.random_rays(n, 2000, seed=tree.ncell)
    o = np.concatenate([[c[1] for c in cases], o])
    d = np.concatenate([[c[2] for c in cases], d])
    tmax = np.concatenate([[c[3] for c in cases], tmax])
    walk = R.Walk(tree, o, d, tmax)
    assert walk.leaf.size > 3000 and (np.diff(walk.off) == 0).sum() > 500
    got = stellar.ray_segments(o, d, tmax)
    assert_same_segments(got, walk, name)
    assert_same_segments(stellar.ray_segments(o, d, tmax), walk, name + ", the second call")
    # without tmax every ray runs to the far side
    far = R.Walk(tree, o, d)
    assert far.leaf.size > walk.leaf.size
    assert_same_segments(stellar.ray_segments(o, d), far, name + ", no tmax")


# ---- the spectra

def test_ingest_golden_random_rays(stellar, ingest):
    """three levels, the golden's own HI, temperature and velocities (all three components), 500 random rays with origins inside and
    outside, some with a tmax, some missing; nvel 1, 64, 300; Lyman alpha and a pure Doppler line; Hubble flow; a period"""
    load(stellar, ingest)
    o, d, tmax = R.random_rays(ingest["n"], 500, seed=500)
    walk = R.Walk(ingest["tree"], o, d, tmax)
    counts = np.diff(walk.off)
    assert (counts == 0).sum() > 50 and counts.max() > 12
    span = 8.0e7
    q = 0
    for nvel in (1, 64, 300):
        for line in (LYA, DOPPLER):
            for hubble, period in ((0.0, 0.0), (3.0e-16, span)) if nvel == 300 else (((0.0, span), (3.0e-16, 0.0))[q % 2],):
                q += 1
                dv = span / nvel
                got = stellar.ray_spectra(o, d, nvel, -0.5 * span, dv, line, tmax, hubble, period)
                want = walk.spectra(ingest["box"], ingest["HI"], ingest["tgas"], ingest["vel"], nvel, -0.5 * span, dv, line, hubble, period)
                assert_same(got, want, f"nvel {nvel} damping {line[1]} hubble {hubble} period {period}")
                assert got["tau"].max() > 0 and np.all(got["N"][counts == 0] == 0) and np.all(got["tau"][counts == 0] == 0)
    # u comes from all three components: with one of them alone the spectra are others
    for keep in range(3):
        one = [v if a == keep else np.zeros_like(v) for a, v in enumerate(ingest["vel"])]
        assert not S.same_bits(walk.spectra(ingest["box"], ingest["HI"], ingest["tgas"], one, 300, -0.5 * span, span / 300, LYA)["tau"], want["tau"])


def test_uniform_grid_with_and_without_a_field(stellar):
    n = 8
    case = dict(n=n, level=np.zeros(n ** 3, dtype=np.int32), **S.random_medium(n ** 3, 8))
    tree = A.Tree(n, case["level"])
    load(stellar, case, velocity=False)
    o, d, tmax = R.random_rays(n, 300, seed=8)
    walk = R.Walk(tree, o, d, tmax)
    nvel, v0, dv = 200, -4.0e7, 4.0e5
    still = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=1e-17)
    assert_same(still, walk.spectra(case["box"], case["HI"], case["tgas"], None, nvel, v0, dv, LYA, 1e-17), "no velocity")
    stellar.set_velocity(*case["vel"])
    moving = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=1e-17)
    assert_same(moving, walk.spectra(case["box"], case["HI"], case["tgas"], case["vel"], nvel, v0, dv, LYA, 1e-17), "a field")
    assert not S.same_bits(moving["tau"], still["tau"]) and S.same_bits(moving["N"], still["N"])
    # a value array of the caller's
    other = case["HI"][::-1].copy()
    assert_same(stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=1e-17, value=other),
                walk.spectra(case["box"], other, case["tgas"], case["vel"], nvel, v0, dv, LYA, 1e-17), "value")


@pytest.mark.parametrize("izone", [1, 5, 15])
def test_axis_aligned_rays_equal_sightline_spectra(stellar, ingest, izone):
    """the rays along the pixel columns of a 13 x 11 map against the parent's function on the same context: tau and the summaries"""
    load(stellar, ingest)
    shape, span = (13, 11), 8.0e7
    o, d, tmax = R.axis_rays(ingest["tree"], izone, shape)
    for nvel, line, hubble, period in ((300, LYA, 3.0e-16, 0.0), (64, DOPPLER, 0.0, span)):
        want = stellar.sightline_spectra(izone, shape, nvel, -0.5 * span, span / nvel, line, hubble=hubble, period=period)
        got = stellar.ray_spectra(o, d, nvel, -0.5 * span, span / nvel, line, tmax, hubble, period)
        assert S.same_bits(got["tau"].reshape(shape + (nvel,)), want["tau"]), izone
        for key in ("N", "W", "dv90"):
            assert S.same_bits(got[key].reshape(shape), want[key]), (izone, key)
        assert got["tau"].max() > 0


# ---- chunk edges and pixel passes

@pytest.fixture(scope="module")
def edge_case():
    """a 4^3 grid with four refined columns along storage k: through their centres rays of 512, 513, 1027 and 1537 segments"""
    n = 4
    columns = {(1, 2): S.CHUNK, (2, 1): S.CHUNK + 1, (0, 3): 2 * S.CHUNK + 3, (0, 0): 3 * S.CHUNK + 1}
    level = S.deep_levels(n, columns)
    case = dict(n=n, level=level, columns=columns, **S.random_medium(level.size, S.CHUNK))
    case["tree"] = A.Tree(n, level)
    return case


@pytest.mark.parametrize("nvel", [S.PASS_PIXELS, 2 * S.PASS_PIXELS + 17])
def test_chunk_edges_and_pixel_passes(stellar, edge_case, nvel):
    """one launch with axis-aligned rays of 4, 512 (one full chunk), 513 (a second chunk of one record), 1027 and 1537 (a fourth
    chunk) segments, both ways along k, and oblique rays through the deepest column; one full pass of pixels, and two and 17 pixels"""
    assert stellar.counter("ray_chunk_segments") == S.CHUNK == R.CHUNK and stellar.counter("spectra_pass_pixels") == S.PASS_PIXELS
    case = edge_case
    load(stellar, case)
    n = case["n"]
    o = [(3.5, 3.5, 0.0)] + [(i + 0.5, j + 0.5, 0.0) for (i, j) in case["columns"]] + [(i + 0.5, j + 0.5, float(n)) for (i, j) in case["columns"]]
    d = [(0.0, 0.0, 1.0)] * 5 + [(0.0, 0.0, -1.0)] * 4
    o += [(0.5, 0.5, 0.0), (0.5, 0.5, 0.0), (0.47, 0.52, 0.0)]
    d += list(R.unit([(1e-4, 2e-4, 1.0), (-3e-3, 1e-3, 1.0), (0.02, -0.01, 1.0)]))
    walk = R.Walk(case["tree"], o, d)
    counts = np.diff(walk.off)
    assert counts[:5].tolist() == [4, S.CHUNK, S.CHUNK + 1, 2 * S.CHUNK + 3, 3 * S.CHUNK + 1] and counts[5:9].tolist() == counts[1:5].tolist()
    assert counts[9] > 3 * S.CHUNK and len(set(counts[9:].tolist())) == 3  # (the first stays in the deepest leaves all the way: four chunks, oblique chords)
    v0, dv = -5.0e7, 1.0e8 / nvel
    for line in (LYA, DOPPLER):
        want = walk.spectra(case["box"], case["HI"], case["tgas"], case["vel"], nvel, v0, dv, line, 2.0e-17)
        got = stellar.ray_spectra(o, d, nvel, v0, dv, line, hubble=2.0e-17)
        assert_same(got, want, f"nvel {nvel} damping {line[1]}")
        assert_same(stellar.ray_spectra(o, d, nvel, v0, dv, line, hubble=2.0e-17), got, "the second call")
    # a ray down a column is the ray up it read backwards: the same column density up to the order of the sum
    assert np.allclose(got["N"][5:9], got["N"][1:5], rtol=1e-12)


# ---- a batch seam by tau alone

def _on_device(st, o, d, nvel, v0, dv, line, with_tau=True, **more):
    import torch
    dev = torch.device("cuda", 0)
    nray = len(o)
    tau = torch.full((nray, nvel), -7.0, dtype=torch.float64, device=dev) if with_tau else None
    summary = torch.full((nray, 3), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    st.ray_spectra(o, d, nvel, v0, dv, line, tau_device_ptr=tau.data_ptr() if with_tau else 0, summary_device_ptr=summary.data_ptr(), **more)
    torch.cuda.synchronize()
    s = summary.cpu().numpy()
    return dict(tau=tau.cpu().numpy() if with_tau else None, N=s[:, 0], W=s[:, 1], dv90=s[:, 2])


def test_batch_seams_by_tau_alone(stellar):
    """4 608 rays x 4 096 pixels on a 4^3 grid: tau staged goes in three batches, the last one short, their seams where the restated
    rule puts them; tau to a device array goes in one; each call twice with the same bits"""
    n, nray, nvel = 4, 4608, 4 * S.PASS_PIXELS
    case = dict(n=n, level=np.zeros(n ** 3, dtype=np.int32), **S.random_medium(n ** 3, 72))
    load(stellar, case)
    assert stellar.counter("ray_work_bytes") == R.WORK_BYTES
    _, d, _ = R.random_rays(n, nray, seed=4608)
    o = np.random.default_rng(7).uniform(0.0, n, (nray, 3))  # every origin inside: every ray hits
    walk = R.Walk(A.Tree(n, case["level"]), o, d)
    staged, direct = R.batches(walk.off, nvel, True), R.batches(walk.off, nvel, False)
    assert len(staged) == 3 and staged[0][1] > staged[2][1] and staged[1][1] > staged[2][1] and len(direct) == 1, (staged, direct)
    for at, _ in staged[1:]:
        assert walk.off[at + 1] > walk.off[at] and walk.off[at] > walk.off[at - 1]  # hitting rays on both sides of every seam
    span, hubble = 1.0e8, 2.0e-17
    v0, dv = -0.5 * span, span / nvel
    want = walk.spectra(case["box"], case["HI"], case["tgas"], case["vel"], nvel, v0, dv, LYA, hubble, span)
    for name in ("host arrays", "host arrays, the second call"):
        assert_same(stellar.ray_spectra(o, d, nvel, v0, dv, LYA, hubble=hubble, period=span), want, name)
    for name in ("_device", "_device, the second call"):
        assert_same(_on_device(stellar, o, d, nvel, v0, dv, LYA, hubble=hubble, period=span), want, name)


# ---- the rest

def test_device_variant_absent_outputs_and_a_missing_ray(stellar, ingest):
    import torch
    load(stellar, ingest)
    n = ingest["n"]
    o, d, tmax = R.random_rays(n, 64, seed=64)
    o[10], d[10] = (-1.0, n + 1.0, 0.5), (1.0, 0.0, 0.0)  # misses, between two that hit
    o[9], d[9], o[11], d[11] = (0.5, 0.5, 0.5), R.unit([1.0, 1.0, 0.3]), (n - 0.5, 0.5, 0.5), R.unit([-1.0, 0.2, 0.3])
    tmax[9:12] = 0.0
    nvel, v0, dv = 300, -4.0e7, 8.0e7 / 300
    walk = R.Walk(ingest["tree"], o, d, tmax)
    want = walk.spectra(ingest["box"], ingest["HI"], ingest["tgas"], ingest["vel"], nvel, v0, dv, LYA, 3e-16)
    both = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=3e-16)
    assert_same(both, want, "host arrays")
    assert np.all(both["tau"][10] == 0) and both["N"][10] == 0 and both["W"][10] == 0 and both["dv90"][10] == 0
    assert both["tau"][9].max() > 0 and both["tau"][11].max() > 0
    only_summary = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=3e-16, want_tau=False)
    only_tau = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=3e-16, want_summary=False)
    assert only_summary["tau"] is None and only_tau["N"] is None and S.same_bits(only_tau["tau"], both["tau"])
    assert_same(only_summary, both, "summaries alone", ("N", "W", "dv90"))
    assert_same(_on_device(stellar, o, d, nvel, v0, dv, LYA, tmax=tmax, hubble=3e-16), want, "_device")
    assert_same(_on_device(stellar, o, d, nvel, v0, dv, LYA, with_tau=False, tmax=tmax, hubble=3e-16), want, "_device, summaries alone", ("N", "W", "dv90"))
    value = torch.from_numpy(np.ascontiguousarray(ingest["HI"][::-1].copy())).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    other = walk.spectra(ingest["box"], ingest["HI"][::-1], ingest["tgas"], ingest["vel"], nvel, v0, dv, LYA, 3e-16)
    assert_same(_on_device(stellar, o, d, nvel, v0, dv, LYA, tmax=tmax, hubble=3e-16, value_device_ptr=value.data_ptr()), other, "value on the device")


def _raw(st, o, d, tmax, nvel, v0, dv, hubble, period, line, tau, summary, nray=None):
    dp = C.POINTER(C.c_double)
    o, d, line = np.array(o, dtype=np.float64), np.array(d, dtype=np.float64), np.array(line, dtype=np.float64)
    t = None if tmax is None else np.array(tmax, dtype=np.float64)
    return st._lib.ftte_ray_spectra(st._ctx, len(o) if nray is None else nray, o.ctypes.data_as(dp), d.ctypes.data_as(dp), None if t is None else t.ctypes.data_as(dp),
                                    nvel, v0, dv, hubble, period, line.ctypes.data_as(dp), None, None if tau is None else tau.ctypes.data_as(dp),
                                    None if summary is None else summary.ctypes.data_as(dp))


def test_refusals_leave_the_outputs_untouched(ingest, golden):
    n, nvel = ingest["n"], 16
    o, d, _ = R.random_rays(n, 40, seed=40)
    tau, summary = np.full((40, nvel), -7.0), np.full((40, 3), -7.0)
    good = dict(o=o, d=d, tmax=None, nvel=nvel, v0=-4e7, dv=5e6, hubble=0.0, period=0.0, line=LYA)
    code = {v: k for k, v in rt._lib.STATUS.items()}
    lp = C.POINTER(C.c_int64)

    def refused(st, status, **change):
        rc = _raw(st, tau=tau, summary=summary, **{**good, **change})
        assert rc == code[status], (change, rt._lib.STATUS.get(rc, rc), st._lib.ftte_last_error(st._ctx))
        assert np.all(tau == -7.0) and np.all(summary == -7.0), change

    def spoiled(which, at, value):
        a = good[which].copy()
        a[at] = value
        return {which: a}

    with rt.StellarTransfer() as probe:
        idle = probe.counter("device_objects")
    with rt.StellarTransfer() as st:
        refused(st, "FTTE_ERR_STATE")                                                     # no grid
        st.set_grid(n, ingest["level"], ingest["box"])
        refused(st, "FTTE_ERR_STATE")                                                     # no medium
        assert st.ray_segments(o, d)["leaf"].size > 0                                     # (the geometry alone needs neither)
        st.set_medium(ingest["HI"], ingest["HI"], ingest["HI"], ingest["rho"], None, 0)
        refused(st, "FTTE_ERR_STATE")                                                     # no temperature
        assert b"temperature" in st._lib.ftte_last_error(st._ctx)
        st.set_temperature(ingest["tgas"])
        st.set_velocity(*ingest["vel"])
        for bad in (np.nan, np.inf, -np.inf):
            refused(st, "FTTE_ERR_ARG", **spoiled("o", (17, 1), bad))
            refused(st, "FTTE_ERR_ARG", **spoiled("d", (39, 2), bad))
            refused(st, "FTTE_ERR_ARG", tmax=np.where(np.arange(40) == 23, bad, 1.0))
        refused(st, "FTTE_ERR_ARG", **spoiled("d", 5, (0.0, 0.0, 0.0)))
        refused(st, "FTTE_ERR_ARG", **spoiled("d", 5, (0.6, 0.8, 1e-4)))                  # |d|^2 - 1 = 1e-8
        refused(st, "FTTE_ERR_ARG", nray=0)
        refused(st, "FTTE_ERR_ARG", nray=-2)
        for change in (dict(nvel=0), dict(nvel=-4), dict(dv=0.0), dict(dv=-1.0), dict(dv=float("nan")), dict(v0=float("inf")), dict(hubble=float("nan")),
                       dict(period=-1.0), dict(line=(1.3e-7, 606.0, 0.0, 0.0)), dict(line=(1.3e-7, 606.0, -1e-24, 0.0)),
                       dict(line=(1.3e-7, -1.0, 1.67e-24, 0.0)), dict(line=(1.3e-7, 606.0, 1.67e-24, -1.0)), dict(line=(float("nan"), 606.0, 1.67e-24, 0.0))):
            refused(st, "FTTE_ERR_ARG", **change)
        assert _raw(st, tau=None, summary=None, **good) == code["FTTE_ERR_ARG"]           # nothing asked for
        # one leaf without a line width, on some rays only: decided before anything is written
        walk = R.Walk(ingest["tree"], o, d)
        crossed = np.bincount(walk.leaf, minlength=ingest["tgas"].size)
        for bad in (0.0, -5.0, float("nan"), float("inf")):
            tgas = ingest["tgas"].copy()
            tgas[int(np.argmax(crossed))] = bad
            st.set_temperature(tgas)
            refused(st, "FTTE_ERR_ARG")
        st.set_temperature(ingest["tgas"])
        # the segment list: a capacity below the total leaves everything as it was, the offsets included
        total = walk.leaf.size
        offset, leaf, t_in, t_out = np.full(41, -7, dtype=np.int64), np.full(total, -7, dtype=np.int64), np.full(total, -7.0), np.full(total, -7.0)
        dp = C.POINTER(C.c_double)
        seg = lambda capacity, nray=40: st._lib.ftte_ray_segments(st._ctx, nray, o.ctypes.data_as(dp), d.ctypes.data_as(dp), None, offset.ctypes.data_as(lp),  # noqa: E731
                                                                  capacity, leaf.ctypes.data_as(lp), t_in.ctypes.data_as(dp), t_out.ctypes.data_as(dp))
        for capacity, nray in ((total - 1, 40), (1, 40), (-1, 40), (total, 0)):
            assert seg(capacity, nray) == code["FTTE_ERR_ARG"]
            assert np.all(offset == -7) and np.all(leaf == -7) and np.all(t_in == -7.0) and np.all(t_out == -7.0)
        assert seg(0) == 0 and np.array_equal(offset, walk.off) and np.all(leaf == -7)    # capacity 0: the offsets alone
        assert seg(total) == 0 and np.array_equal(leaf, walk.leaf) and S.same_bits(t_in, walk.t_in) and S.same_bits(t_out, walk.t_out)
        assert _raw(st, tau=tau, summary=summary, **good) == 0 and np.all(tau >= 0.0) and summary[:, 0].max() > 0  # and the context is still good
        held = st.counter("device_objects")
        assert held > idle
        # another grid: the working memory goes
        u = golden("analysis_uniform16")
        st.set_grid(int(u["n"]), u["level"], float(u["box"]))
        assert st.counter("device_objects") < held
        tau[:], summary[:] = -7.0, -7.0
        refused(st, "FTTE_ERR_STATE")
        # the owner: the same round trip with and without rays leaves the same number of device objects
        counts = []
        for with_rays in (False, True, True):
            st.set_grid(n, ingest["level"], ingest["box"])
            st.set_medium(ingest["HI"], ingest["HI"], ingest["HI"], ingest["rho"], None, 0)
            st.set_temperature(ingest["tgas"])
            st.project_map(5, (13, 11), mode=1, value=ingest["HI"])
            if with_rays:
                assert _raw(st, tau=tau, summary=summary, **{**good, "tmax": np.ones(40)}) == 0
                st.ray_segments(o, d)
            st.set_grid(int(u["n"]), u["level"], float(u["box"]))
            counts.append(st.counter("device_objects"))
        assert counts[0] == counts[1] == counts[2], counts
    with rt.StellarTransfer() as probe:
        assert probe.counter("device_objects") == idle                                    # close() released everything


def test_multi_device_context_refuses(golden):
    g = golden("analysis_uniform16")
    with rt.StellarTransfer(devices=[0, 0]) as st:
        st.set_grid(int(g["n"]), g["level"], float(g["box"]))
        for call in (lambda: st.ray_spectra([(0.5, 0.5, 0.5)], [(0.0, 0.0, 1.0)], 8, 0.0, 1e5, LYA), lambda: st.ray_segments([(0.5, 0.5, 0.5)], [(0.0, 0.0, 1.0)])):
            with pytest.raises(rt.FtteError) as err:
                call()
            assert err.value.status == "FTTE_ERR_UNSUPPORTED", str(err.value)
