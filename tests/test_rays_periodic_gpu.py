"""The periodic rays on the GPU against the g++ evaluation of csrc/ftte_ray_math.h and csrc/ftte_spectra_math.h
(tests/_rays_periodic.py; held against the brute force over the box's images by test_rays_periodic_host.py): the segment lists bit
for bit on every host case; tau, N, W and dv90 bit for bit on the ingest golden and a uniform grid; chunk edges reached only by
wrapping; three batches of long rays; the _device variant, absent outputs, the refusals, and the non-periodic calls unchanged on the
same context."""
import ctypes as C

import numpy as np
import pytest

import _analysis as A
import _rays as R
import _rays_periodic as P
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
    """the named rays, the six axis rays and the 2 000 random ones of test_rays_periodic_host.py, and the rays that end before their
    first wrap: offsets, leaves, t_in and t_out bit for bit; needs a grid only"""
    level = {"uniform": np.zeros(64, dtype=np.int32), "corner": np.array([2] * 8 + [1] * 7 + [0] * 63, dtype=np.int32), "ingest": ingest["level"]}[name]
    n = ingest["n"] if name == "ingest" else 4
    tree = A.Tree(n, level)
    stellar.set_grid(n, level, 3.0e24)
    cases = P.named_rays(n)
    o, d, tmax = P.random_rays(n, 2000, seed=tree.ncell)
    o = np.concatenate([[c[1] for c in cases], o])
    d = np.concatenate([[c[2] for c in cases], d])
    tmax = np.concatenate([[c[3] for c in cases], tmax])
    walk = P.Walk(tree, o, d, tmax)
    assert walk.leaf.size > 30000 and np.all(np.diff(walk.off) >= 1)
    assert_same_segments(stellar.ray_segments(o, d, tmax, periodic=True), walk, name)
    assert_same_segments(stellar.ray_segments(o, d, tmax, periodic=True), walk, name + ", the second call")
    # before the first wrap: the non-periodic call, the periodic call and the host walk agree
    inside = np.random.default_rng(601).uniform(0.0, n, (600, 3))
    far = R.Walk(tree, inside, d[-600:])
    short = np.random.default_rng(602).uniform(0.05, 0.999, 600) * far.start[:, 1]
    got = stellar.ray_segments(inside, d[-600:], short, periodic=True)
    assert_same_segments(got, P.Walk(tree, inside, d[-600:], short), name + ", before the first wrap")
    assert_same_segments(stellar.ray_segments(inside, d[-600:], short), P.Walk(tree, inside, d[-600:], short), name + ", the non-periodic call")


# ---- the spectra

def test_ingest_golden_random_rays(stellar, ingest):
    """three levels, the golden's own HI, temperature and velocities, 300 random rays of 3 to 5 boxes; nvel 1, 64, 300; Lyman alpha
    and a pure Doppler line; Hubble flow with and without a period"""
    load(stellar, ingest)
    o, d, tmax = P.random_rays(ingest["n"], 300, seed=300, shortest=3.0, longest=5.0)
    walk = P.Walk(ingest["tree"], o, d, tmax)
    counts = np.diff(walk.off)
    assert counts.min() > 12 and counts.max() > 60 and tmax.min() >= 3.0 * ingest["n"]
    span = 8.0e7
    q = 0
    for nvel in (1, 64, 300):
        for line in (LYA, DOPPLER):
            for hubble, period in ((0.0, 0.0), (3.0e-16, span), (3.0e-16, 0.0)) if nvel == 300 else (((0.0, span), (3.0e-16, 0.0))[q % 2],):
                q += 1
                dv = span / nvel
                got = stellar.ray_spectra(o, d, nvel, -0.5 * span, dv, line, tmax, hubble, period, periodic=True)
                want = walk.spectra(ingest["box"], ingest["HI"], ingest["tgas"], ingest["vel"], nvel, -0.5 * span, dv, line, hubble, period)
                assert_same(got, want, f"nvel {nvel} damping {line[1]} hubble {hubble} period {period}")
                assert got["tau"].max() > 0 and got["N"].min() > 0
    # s keeps growing across images: with s folded back into the box the Hubble-flow spectra are others
    size, s, u = walk.line_inputs(ingest["box"], ingest["vel"])
    folded = np.mod(s, ingest["box"])
    status, tau, _ = S.lines(walk.off, ingest["HI"][walk.leaf], size, ingest["tgas"][walk.leaf], folded, u, 300, -0.5 * span, span / 300, DOPPLER, 3.0e-16, 0.0)
    assert status == 0 and not S.same_bits(tau, want["tau"])


def test_uniform_grid_with_and_without_a_field(stellar):
    n = 8
    case = dict(n=n, level=np.zeros(n ** 3, dtype=np.int32), **S.random_medium(n ** 3, 8))
    tree = A.Tree(n, case["level"])
    load(stellar, case, velocity=False)
    o, d, tmax = P.random_rays(n, 300, seed=8, shortest=0.5, longest=4.0)
    walk = P.Walk(tree, o, d, tmax)
    nvel, v0, dv = 200, -4.0e7, 4.0e5
    still = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=1e-17, periodic=True)
    assert_same(still, walk.spectra(case["box"], case["HI"], case["tgas"], None, nvel, v0, dv, LYA, 1e-17), "no velocity")
    stellar.set_velocity(*case["vel"])
    moving = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=1e-17, periodic=True)
    assert_same(moving, walk.spectra(case["box"], case["HI"], case["tgas"], case["vel"], nvel, v0, dv, LYA, 1e-17), "a field")
    assert not S.same_bits(moving["tau"], still["tau"]) and S.same_bits(moving["N"], still["N"])


# ---- chunk edges reached only by wrapping

@pytest.fixture(scope="module")
def edge_case():
    """a 4^3 grid with refined columns along storage k: through their centres rays of 512 and 1537 segments a box"""
    n = 4
    columns = {(1, 2): S.CHUNK, (0, 0): 3 * S.CHUNK + 1}
    level = S.deep_levels(n, columns)
    case = dict(n=n, level=level, columns=columns, **S.random_medium(level.size, S.CHUNK))
    case["tree"] = A.Tree(n, level)
    return case


def _ending_in_segment(tree, o, d, boxes, count):
    """the tmax that ends the periodic ray in the middle of its segment `count`: the ray has that many"""
    long = P.Walk(tree, [o], [d], [float(boxes * tree.n)])
    assert long.leaf.size >= count
    return 0.5 * (long.t_in[count - 1] + long.t_out[count - 1])


@pytest.mark.parametrize("nvel", [S.PASS_PIXELS, 2 * S.PASS_PIXELS + 17])
def test_chunk_edges_reached_by_wrapping(stellar, edge_case, nvel):
    """axis rays whose record counts are 512 (128 boxes of a plain column: one full chunk), 513, 1 024 (two boxes of the 512 column),
    1 537 + 512 and + 513 (the deepest column into its second box: a fourth chunk filled to its edge), both ways along k"""
    assert stellar.counter("ray_chunk_segments") == S.CHUNK == R.CHUNK and stellar.counter("spectra_pass_pixels") == S.PASS_PIXELS
    case = edge_case
    load(stellar, case)
    n, tree = case["n"], case["tree"]
    up, down = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
    deep = 3 * S.CHUNK + 1
    plan = [((3.5, 3.5, 0.0), up, float(S.CHUNK), S.CHUNK), ((3.5, 3.5, float(n)), down, S.CHUNK + 0.5, S.CHUNK + 1),
            ((1.5, 2.5, 0.0), up, 2.0 * n, 2 * S.CHUNK), ((1.5, 2.5, float(n)), down, 2.0 * n, 2 * S.CHUNK)]
    for o, d in (((0.5, 0.5, 0.0), up), ((0.5, 0.5, float(n)), down)):
        for count in (deep + S.CHUNK, deep + S.CHUNK + 1):
            plan.append((o, d, _ending_in_segment(tree, o, d, 2, count), count))
    o, d, tmax = [p[0] for p in plan], [p[1] for p in plan], [p[2] for p in plan]
    walk = P.Walk(tree, o, d, tmax)
    assert np.diff(walk.off).tolist() == [p[3] for p in plan]
    assert np.all(np.array(tmax[4:]) > n)  # (the deepest column's counts lie in the second box)
    v0, dv = -5.0e7, 1.0e8 / nvel
    for line in (LYA, DOPPLER):
        want = walk.spectra(case["box"], case["HI"], case["tgas"], case["vel"], nvel, v0, dv, line, 2.0e-17)
        got = stellar.ray_spectra(o, d, nvel, v0, dv, line, tmax, hubble=2.0e-17, periodic=True)
        assert_same(got, want, f"nvel {nvel} damping {line[1]}")
        assert_same(stellar.ray_spectra(o, d, nvel, v0, dv, line, tmax, hubble=2.0e-17, periodic=True), got, "the second call")


# ---- batches

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


def test_batch_seams_from_long_rays(stellar):
    """4 608 rays of 4 boxes x 4 096 pixels on a 4^3 grid: tau staged goes in at least three batches, their seams where the restated
    rule puts them; each call twice with the same bits"""
    n, nray, nvel = 4, 4608, 4 * S.PASS_PIXELS
    case = dict(n=n, level=np.zeros(n ** 3, dtype=np.int32), **S.random_medium(n ** 3, 72))
    load(stellar, case)
    assert stellar.counter("ray_work_bytes") == R.WORK_BYTES
    o, d, _ = P.random_rays(n, nray, seed=4608)
    tmax = np.full(nray, 4.0 * n)
    walk = P.Walk(A.Tree(n, case["level"]), o, d, tmax)
    staged, direct = R.batches(walk.off, nvel, True), R.batches(walk.off, nvel, False)
    assert len(staged) >= 3 and staged[-1][1] < staged[0][1] and len(direct) == 1, (staged, direct)
    assert sum(b[1] for b in staged) == nray and np.diff(walk.off).min() >= 16
    span, hubble = 1.0e8, 2.0e-17
    v0, dv = -0.5 * span, span / nvel
    want = walk.spectra(case["box"], case["HI"], case["tgas"], case["vel"], nvel, v0, dv, LYA, hubble, span)
    for name in ("host arrays", "host arrays, the second call"):
        got = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=hubble, period=span, periodic=True)
        for at, m in staged:
            assert_same({k: got[k][at:at + m] for k in KEYS}, {k: want[k][at:at + m] for k in KEYS}, f"{name}, the batch from ray {at}")
    for name in ("_device", "_device, the second call"):
        assert_same(_on_device(stellar, o, d, nvel, v0, dv, LYA, tmax=tmax, hubble=hubble, period=span, periodic=True), want, name)


def test_device_variant_absent_outputs_and_the_existing_calls(stellar, ingest):
    import torch
    load(stellar, ingest)
    n = ingest["n"]
    o, d, tmax = P.random_rays(n, 64, seed=64, shortest=1.0, longest=4.0)
    nvel, v0, dv = 300, -4.0e7, 8.0e7 / 300
    # a non-periodic call before and after the periodic ones: the same bits
    before = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=3e-16)
    before_segments = stellar.ray_segments(o, d, tmax)
    walk = P.Walk(ingest["tree"], o, d, tmax)
    want = walk.spectra(ingest["box"], ingest["HI"], ingest["tgas"], ingest["vel"], nvel, v0, dv, LYA, 3e-16)
    both = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=3e-16, periodic=True)
    assert_same(both, want, "host arrays")
    only_summary = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=3e-16, want_tau=False, periodic=True)
    only_tau = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=3e-16, want_summary=False, periodic=True)
    assert only_summary["tau"] is None and only_tau["N"] is None and S.same_bits(only_tau["tau"], both["tau"])
    assert_same(only_summary, both, "summaries alone", ("N", "W", "dv90"))
    assert_same(_on_device(stellar, o, d, nvel, v0, dv, LYA, tmax=tmax, hubble=3e-16, periodic=True), want, "_device")
    assert_same(_on_device(stellar, o, d, nvel, v0, dv, LYA, with_tau=False, tmax=tmax, hubble=3e-16, periodic=True), want, "_device, summaries alone", ("N", "W", "dv90"))
    value = torch.from_numpy(np.ascontiguousarray(ingest["HI"][::-1].copy())).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    other = walk.spectra(ingest["box"], ingest["HI"][::-1], ingest["tgas"], ingest["vel"], nvel, v0, dv, LYA, 3e-16)
    assert_same(_on_device(stellar, o, d, nvel, v0, dv, LYA, tmax=tmax, hubble=3e-16, value_device_ptr=value.data_ptr(), periodic=True), other, "value on the device")
    assert_same_segments(stellar.ray_segments(o, d, tmax, periodic=True), walk, "the segments")
    after = stellar.ray_spectra(o, d, nvel, v0, dv, LYA, tmax, hubble=3e-16)
    assert_same(after, before, "the non-periodic call after the periodic ones")
    host = R.Walk(ingest["tree"], o, d, tmax)
    assert_same(after, host.spectra(ingest["box"], ingest["HI"], ingest["tgas"], ingest["vel"], nvel, v0, dv, LYA, 3e-16), "the non-periodic call")
    after_segments = stellar.ray_segments(o, d, tmax)
    assert_same_segments(after_segments, host, "the non-periodic segments")
    assert all(np.array_equal(before_segments[k], after_segments[k]) for k in before_segments)
    assert not S.same_bits(after["N"], both["N"])
    with pytest.raises(ValueError):
        stellar.ray_spectra(o, d, nvel, v0, dv, LYA, periodic=True)
    with pytest.raises(ValueError):
        stellar.ray_segments(o, d, periodic=True)


# ---- the refusals

def _raw(st, o, d, tmax, nvel, v0, dv, hubble, period, line, tau, summary):
    dp = C.POINTER(C.c_double)
    o, d, line = np.array(o, dtype=np.float64), np.array(d, dtype=np.float64), np.array(line, dtype=np.float64)
    t = None if tmax is None else np.array(tmax, dtype=np.float64)
    return st._lib.ftte_ray_spectra_periodic(st._ctx, len(o), o.ctypes.data_as(dp), d.ctypes.data_as(dp), None if t is None else t.ctypes.data_as(dp), nvel, v0, dv,
                                             hubble, period, line.ctypes.data_as(dp), None, tau.ctypes.data_as(dp), summary.ctypes.data_as(dp))


def test_refusals_leave_the_outputs_untouched(ingest):
    n, nvel = ingest["n"], 16
    o, d, tmax = P.random_rays(n, 40, seed=40)
    tau, summary = np.full((40, nvel), -7.0), np.full((40, 3), -7.0)
    good = dict(o=o, d=d, tmax=tmax, nvel=nvel, v0=-4e7, dv=5e6, hubble=0.0, period=0.0, line=LYA)
    code = {v: k for k, v in rt._lib.STATUS.items()}
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def refused(st, status, message=None, **change):
        rc = _raw(st, tau=tau, summary=summary, **{**good, **change})
        assert rc == code[status], (change, rt._lib.STATUS.get(rc, rc), st._lib.ftte_last_error(st._ctx))
        assert np.all(tau == -7.0) and np.all(summary == -7.0), change
        if message:
            assert message in st._lib.ftte_last_error(st._ctx), st._lib.ftte_last_error(st._ctx)

    def spoiled(which, at, value):
        a = good[which].copy()
        a[at] = value
        return {which: a}

    with rt.StellarTransfer() as st:
        load(st, ingest)
        refused(st, "FTTE_ERR_ARG", b"tmax", tmax=None)                                    # tmax absent
        refused(st, "FTTE_ERR_ARG", b"ray 23", **spoiled("tmax", 23, 0.0))                 # a tmax <= 0 among good ones: the first is named
        refused(st, "FTTE_ERR_ARG", b"ray 7", tmax=np.where(np.isin(np.arange(40), (7, 23)), -1.0, tmax))
        refused(st, "FTTE_ERR_ARG", **spoiled("tmax", 5, np.nan))
        refused(st, "FTTE_ERR_UNSUPPORTED", b"2^20", **spoiled("tmax", 31, n * 2.0 ** 20 + 1.0))  # tmax / n > 2^20
        refused(st, "FTTE_ERR_UNSUPPORTED", b"ray 12", **spoiled("o", (12, 1), -n * 2.0 ** 20 - 1.0))
        refused(st, "FTTE_ERR_ARG", **spoiled("d", 5, (0.6, 0.8, 1e-4)))                   # a non-unit direction
        refused(st, "FTTE_ERR_ARG", **spoiled("d", 5, (0.0, 0.0, 0.0)))
        refused(st, "FTTE_ERR_ARG", **spoiled("o", (17, 1), np.inf))
        # the segment list: everything untouched, the offsets included
        offset, leaf, t_in, t_out = np.full(41, -7, dtype=np.int64), np.full(8, -7, dtype=np.int64), np.full(8, -7.0), np.full(8, -7.0)
        bad = tmax.copy()
        bad[3] = -2.0
        for t in (None, bad):
            rc = st._lib.ftte_ray_segments_periodic(st._ctx, 40, o.ctypes.data_as(dp), d.ctypes.data_as(dp), None if t is None else t.ctypes.data_as(dp),
                                                    offset.ctypes.data_as(lp), 8, leaf.ctypes.data_as(lp), t_in.ctypes.data_as(dp), t_out.ctypes.data_as(dp))
            assert rc == code["FTTE_ERR_ARG"] and np.all(offset == -7) and np.all(leaf == -7) and np.all(t_in == -7.0) and np.all(t_out == -7.0)
        assert _raw(st, tau=tau, summary=summary, **good) == 0 and np.all(tau >= 0.0) and summary[:, 0].min() > 0  # and the context is still good


def test_multi_device_context_refuses(golden):
    g = golden("analysis_uniform16")
    with rt.StellarTransfer(devices=[0, 0]) as st:
        st.set_grid(int(g["n"]), g["level"], float(g["box"]))
        for call in (lambda: st.ray_spectra([(0.5, 0.5, 0.5)], [(0.0, 0.0, 1.0)], 8, 0.0, 1e5, LYA, [40.0], periodic=True),
                     lambda: st.ray_segments([(0.5, 0.5, 0.5)], [(0.0, 0.0, 1.0)], [40.0], periodic=True)):
            with pytest.raises(rt.FtteError) as err:
                call()
            assert err.value.status == "FTTE_ERR_UNSUPPORTED", str(err.value)
        tau, summary = np.full((1, 8), -7.0), np.full((1, 3), -7.0)
        rc = _raw(st, [(0.5, 0.5, 0.5)], [(0.0, 0.0, 1.0)], [40.0], 8, 0.0, 1e5, 0.0, 0.0, LYA, tau, summary)
        assert rt._lib.STATUS[rc] == "FTTE_ERR_UNSUPPORTED" and np.all(tau == -7.0) and np.all(summary == -7.0)
