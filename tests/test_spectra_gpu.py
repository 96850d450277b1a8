"""The sightline spectra on the GPU against the g++ evaluation of csrc/ftte_spectra_math.h on the segments the numpy walk finds
(tests/_spectra.py; held against an independent Voigt function, plain numpy and the projected map by test_spectra_host.py): tau, N, W
and dv90 bit for bit -- on the ingest golden under all 24 izones, on a uniform grid, on a tree whose one sightline spills over two
chunks and one pass of pixels; the _device variants, absent outputs, freshness, the refusals, the owner; and what a production map
runs: three batches with spilled lines on both sides of their seams, three batches by tau alone, lines at and around every chunk
edge over one, two and three passes of pixels, a window deeper than one round of the gather."""
import ctypes as C

import numpy as np
import pytest

import _analysis as A
import _spectra as S
import radiativetransfer_amd as rt

pytestmark = pytest.mark.gpu

DOPPLER = (rt.LYMAN_ALPHA[0], 0.0, rt.LYMAN_ALPHA[2], 0.0)
VSCALE = 1.0e5  # the golden's velocities reach 323: times this, u spreads over +-3e7 cm/s, some twenty thermal widths at 1e4 K


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


def assert_same(got, want, what=""):
    assert got["tau"].shape == want["tau"].shape, what
    for key in ("tau", "N", "W", "dv90"):
        assert S.same_bits(got[key], want[key]), f"{what}: {key} differs, largest relative difference " \
            f"{np.nanmax(np.abs(got[key] - want[key]) / np.maximum(np.abs(want[key]), 1e-300)):.3e}"


def test_line_constants():
    assert rt.LYMAN_ALPHA == S.LYMAN_ALPHA


@pytest.mark.parametrize("shape", [(13, 11), (50, 37)])
def test_ingest_golden_under_every_izone(stellar, ingest, shape):
    """three levels, the golden's own HI, temperature and velocities; per izone the whole box and a window clamped at 0 and in kend;
    nvel 1, 64 (one wavefront), 300 (partly filled rows); Lyman alpha and a pure Doppler line; Hubble flow; a period"""
    load(stellar, ingest)
    T, box = ingest["tree"], ingest["box"]
    span = 8.0e7
    seen = set()
    for izone in range(1, 25):
        windows = [((0.5, 0.5, 0.5), 1.0), ((0.1, 0.93, 0.95), 3.0)] if shape[0] == 13 else [((0.5, 0.5, 0.5), 1.0) if izone % 2 else ((0.1, 0.93, 0.95), 3.0)]
        for centre, zoom in windows:
            seg = S.Segments(T, box, izone, shape, centre, zoom)
            runs = [(nvel, line) for nvel in (1, 64, 300) for line in (rt.LYMAN_ALPHA, DOPPLER)] if shape[0] == 13 else \
                [((1, 64, 300)[izone % 3], (rt.LYMAN_ALPHA, DOPPLER)[(izone // 3) % 2])]
            for q, (nvel, line) in enumerate(runs):
                dv = span / nvel
                hubble = (0.0, 3.0e-16)[(izone + q) % 2 if shape[0] == 13 else (izone // 6) % 2]  # 3e-16 /s over the box's 1.4e23 cm: 4e7 cm/s
                period = (0.0, 0.0, span)[(izone + q) % 3] if shape[0] == 13 else (0.0, span)[(izone // 12) % 2]
                got = stellar.sightline_spectra(izone, shape, nvel, -0.5 * span, dv, line, centre, zoom, hubble, period)
                want = S.map_lines(seg, ingest["HI"], ingest["tgas"], ingest["vel"], nvel, -0.5 * span, dv, line, hubble, period)
                assert_same(got, want, f"izone {izone} {shape} zoom {zoom} nvel {nvel} damping {line[1]} hubble {hubble} period {period}")
                assert got["tau"].max() > 0
                seen.add((nvel, line[1] > 0, hubble > 0, period > 0))
    assert {s[0] for s in seen} == {1, 64, 300} and all({s[q] for s in seen} == {False, True} for q in (1, 2, 3))


def test_uniform_grid_and_no_velocity(stellar, golden):
    g = golden("analysis_uniform16")
    rng = np.random.default_rng(16)
    nc = g["level"].size
    case = dict(n=int(g["n"]), level=g["level"], box=float(g["box"]), HI=g["HI"], rho=g["rho"], tgas=10.0 ** rng.uniform(3.5, 5.0, nc),
                vel=[rng.uniform(-2e7, 2e7, nc) for _ in range(3)])
    T = A.Tree(case["n"], case["level"])
    load(stellar, case, velocity=False)
    assert stellar.counter("spectra_velocity") == 0
    shape, nvel, v0, dv = (20, 9), 200, -4.0e7, 4.0e5
    for izone in (2, 17):
        seg = S.Segments(T, case["box"], izone, shape)
        still = stellar.sightline_spectra(izone, shape, nvel, v0, dv, rt.LYMAN_ALPHA, hubble=1e-17)
        assert_same(still, S.map_lines(seg, case["HI"], case["tgas"], None, nvel, v0, dv, rt.LYMAN_ALPHA, 1e-17), "no velocity")
        stellar.set_velocity(*[np.zeros(nc)] * 3)
        assert_same(stellar.sightline_spectra(izone, shape, nvel, v0, dv, rt.LYMAN_ALPHA, hubble=1e-17), still, "zero velocities")
        stellar.set_velocity(*case["vel"])
        assert stellar.counter("spectra_velocity") == 1
        moving = stellar.sightline_spectra(izone, shape, nvel, v0, dv, rt.LYMAN_ALPHA, hubble=1e-17)
        assert_same(moving, S.map_lines(seg, case["HI"], case["tgas"], case["vel"], nvel, v0, dv, rt.LYMAN_ALPHA, 1e-17), "synthetic velocities")
        assert not S.same_bits(moving["tau"], still["tau"]) and S.same_bits(moving["N"], still["N"])
        stellar.set_velocity(None, None, None)
        assert_same(stellar.sightline_spectra(izone, shape, nvel, v0, dv, rt.LYMAN_ALPHA, hubble=1e-17), still, "the field dropped")


def test_a_sightline_beyond_two_chunks_and_one_pass(stellar):
    """a 4^3 base grid whose cells under pixel (0, 0) of izone 1 are refined level by level until that line holds 2 chunk + 3
    segments (the spill, three chunks, the last one of three records); its neighbours see 4; nvel one more than a pass holds"""
    chunk, one_pass = stellar.counter("spectra_chunk_segments"), stellar.counter("spectra_pass_pixels")
    assert chunk > 0 and one_pass > 0
    n, want_segments = 4, 2 * chunk + 3
    share = [want_segments // 4 + (1 if k < want_segments % 4 else 0) for k in range(4)]
    level = []
    for i in range(n):
        for j in range(n):
            for k in range(n):
                level += S.deep_column(share[k], 0, True) if (i, j) == (0, 0) else [0]
    level = np.array(level, dtype=np.int32)
    rng = np.random.default_rng(chunk)
    nc = level.size
    case = dict(n=n, level=level, box=3.0e24, HI=10.0 ** rng.uniform(-9, -5, nc), tgas=10.0 ** rng.uniform(3.5, 5.0, nc),
                vel=[rng.uniform(-2e7, 2e7, nc) for _ in range(3)])
    T = A.Tree(n, level)
    load(stellar, case)
    nvel = one_pass + 1
    v0, dv = -5.0e7, 1.0e8 / nvel
    for izone, line in ((1, rt.LYMAN_ALPHA), (5, DOPPLER)):  # (izone 5: the same columns, the depth mirrored)
        seg = S.Segments(T, case["box"], izone, (4, 4))
        counts = np.diff(seg.off)
        assert counts.max() == want_segments and counts.min() == 4 and (counts > 4).sum() == 1
        got = stellar.sightline_spectra(izone, (4, 4), nvel, v0, dv, line, hubble=2e-17)
        assert_same(got, S.map_lines(seg, case["HI"], case["tgas"], case["vel"], nvel, v0, dv, line, 2e-17), f"izone {izone}")
        assert_same(stellar.sightline_spectra(izone, (4, 4), nvel, v0, dv, line, hubble=2e-17), got, "the second call")


@pytest.mark.parametrize("name", ["analysis_refined6", "analysis_uniform16"])
def test_column_density_is_the_path_integral_map(stellar, golden, ingest, name):
    g = golden(name)
    cases = [dict(n=int(g["n"]), level=g["level"], box=float(g["box"]), HI=g["HI"], rho=g["rho"], tgas=np.full(g["HI"].size, 2.0e4))]
    if name == "analysis_refined6":
        cases.append(ingest)
    for case in cases:
        load(stellar, case, velocity=False)
        for izone, shape, centre, zoom in ((3, (50, 37), (0.5, 0.5, 0.5), 1.0), (20, (13, 11), (0.4, 0.6, 0.5), 2.0)):
            out = stellar.sightline_spectra(izone, shape, 8, -1e6, 2.5e5, DOPPLER, centre, zoom, want_tau=False)
            pixel = stellar.project_map(izone, shape, centre, zoom, mode=1, value=case["HI"])
            assert out["tau"] is None and np.array_equal(out["N"].astype(np.float32).view(np.uint32), np.ascontiguousarray(pixel).view(np.uint32))


def test_device_variants_absent_outputs_and_freshness(stellar, ingest):
    import torch
    load(stellar, ingest)
    izone, shape, nvel, v0, dv = 11, (13, 11), 300, -4.0e7, 8.0e7 / 300
    args = (izone, shape, nvel, v0, dv, rt.LYMAN_ALPHA)
    both = stellar.sightline_spectra(*args, hubble=3e-16)
    assert_same(stellar.sightline_spectra(*args, hubble=3e-16), both, "two calls")
    # either output absent: the other one's bits stay
    only_summary = stellar.sightline_spectra(*args, hubble=3e-16, want_tau=False)
    only_tau = stellar.sightline_spectra(*args, hubble=3e-16, want_summary=False)
    assert only_summary["tau"] is None and only_tau["N"] is None and S.same_bits(only_tau["tau"], both["tau"])
    assert all(S.same_bits(only_summary[k], both[k]) for k in ("N", "W", "dv90"))
    # a value array of the caller's equal to the medium's HI, on the host and on the device; tau and the summaries into torch tensors
    assert_same(stellar.sightline_spectra(*args, hubble=3e-16, value=ingest["HI"]), both, "value = HI")
    dev = torch.device("cuda", 0)
    value = torch.from_numpy(np.ascontiguousarray(ingest["HI"])).to(dev)
    tau = torch.full((shape[1], shape[0], nvel), -7.0, dtype=torch.float64, device=dev)
    summary = torch.full((shape[1], shape[0], 3), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    stellar.sightline_spectra(*args, hubble=3e-16, value_device_ptr=value.data_ptr(), tau_device_ptr=tau.data_ptr(), summary_device_ptr=summary.data_ptr())
    torch.cuda.synchronize()
    on_device = dict(tau=tau.cpu().numpy().transpose(1, 0, 2), **{k: summary.cpu().numpy()[:, :, q].T for q, k in enumerate(("N", "W", "dv90"))})
    assert_same(on_device, both, "_device")
    summary.fill_(-7.0)
    torch.cuda.synchronize()
    stellar.sightline_spectra(*args, hubble=3e-16, summary_device_ptr=summary.data_ptr())  # value NULL: the medium's HI; tau absent
    torch.cuda.synchronize()
    assert S.same_bits(summary.cpu().numpy()[:, :, 1].T, both["W"])
    # the velocity field from device arrays
    vel_dev = [torch.from_numpy(np.ascontiguousarray(-v)).to(dev) for v in ingest["vel"]]
    torch.cuda.synchronize()
    stellar.set_velocity(device_ptrs=[v.data_ptr() for v in vel_dev])
    seg = S.Segments(ingest["tree"], ingest["box"], izone, shape)
    want = S.map_lines(seg, ingest["HI"], ingest["tgas"], [-v for v in ingest["vel"]], nvel, v0, dv, rt.LYMAN_ALPHA, 3e-16)
    assert_same(stellar.sightline_spectra(*args, hubble=3e-16), want, "velocities from the device")
    stellar.set_velocity(*ingest["vel"])
    # another temperature, another medium: the spectrum is the new one's
    hot = 3.0 * ingest["tgas"]
    stellar.set_temperature(hot)
    got = stellar.sightline_spectra(*args, hubble=3e-16)
    assert_same(got, S.map_lines(seg, ingest["HI"], hot, ingest["vel"], nvel, v0, dv, rt.LYMAN_ALPHA, 3e-16), "after set_temperature")
    assert not S.same_bits(got["tau"], both["tau"])
    HI2 = ingest["HI"][::-1].copy()
    stellar.set_medium(HI2, HI2, HI2, ingest["rho"], None, 0)
    assert_same(stellar.sightline_spectra(*args, hubble=3e-16), S.map_lines(seg, HI2, hot, ingest["vel"], nvel, v0, dv, rt.LYMAN_ALPHA, 3e-16), "after set_medium")


def _raw(st, izone, shape, centre, zoom, nvel, v0, dv, hubble, period, line, tau, summary):
    dp = C.POINTER(C.c_double)
    centre, line = np.array(centre, dtype=np.float64), np.array(line, dtype=np.float64)
    return st._lib.ftte_sightline_spectra(st._ctx, izone, shape[0], shape[1], centre.ctypes.data_as(dp), zoom, nvel, v0, dv, hubble, period,
                                          line.ctypes.data_as(dp), None, None if tau is None else tau.ctypes.data_as(dp),
                                          None if summary is None else summary.ctypes.data_as(dp))


def test_refusals_leave_the_outputs_untouched(ingest, golden):
    shape, nvel = (13, 11), 16
    tau, summary = np.full((shape[1], shape[0], nvel), -7.0), np.full((shape[1], shape[0], 3), -7.0)
    good = dict(izone=5, shape=shape, centre=(0.5, 0.5, 0.5), zoom=1.0, nvel=nvel, v0=-4e7, dv=5e6, hubble=0.0, period=0.0, line=rt.LYMAN_ALPHA)
    code = {v: k for k, v in rt._lib.STATUS.items()}

    def refused(st, status, **change):
        rc = _raw(st, tau=tau, summary=summary, **{**good, **change})
        assert rc == code[status], (change, rt._lib.STATUS.get(rc, rc), st._lib.ftte_last_error(st._ctx))
        assert np.all(tau == -7.0) and np.all(summary == -7.0), change

    with rt.StellarTransfer() as probe:
        idle = probe.counter("device_objects")
    with rt.StellarTransfer() as st:
        refused(st, "FTTE_ERR_STATE")                                                     # no grid
        with pytest.raises(rt.FtteError) as err:
            st.set_velocity(*ingest["vel"])
        assert err.value.status == "FTTE_ERR_STATE"
        st.set_grid(ingest["n"], ingest["level"], ingest["box"])
        refused(st, "FTTE_ERR_STATE")                                                     # no medium
        st.set_medium(ingest["HI"], ingest["HI"], ingest["HI"], ingest["rho"], None, 0)
        refused(st, "FTTE_ERR_STATE")                                                     # no temperature
        assert b"temperature" in st._lib.ftte_last_error(st._ctx)
        st.set_temperature(ingest["tgas"])
        with pytest.raises(rt.FtteError) as err:
            st.set_velocity(ingest["vel"][0], None, ingest["vel"][2])
        assert err.value.status == "FTTE_ERR_ARG"
        st.set_velocity(*ingest["vel"])
        for izone in (0, 25, -3):
            refused(st, "FTTE_ERR_IZONE", izone=izone)
        for change in (dict(shape=(0, 11)), dict(shape=(13, -1)), dict(zoom=0.0), dict(zoom=float("nan")), dict(centre=(1.7, 0.5, 0.5), zoom=2.0),
                       dict(nvel=0), dict(nvel=-4), dict(dv=0.0), dict(dv=-1.0), dict(dv=float("nan")), dict(period=-1.0),
                       dict(line=(1.3e-7, 606.0, 0.0, 0.0)), dict(line=(1.3e-7, 606.0, -1e-24, 0.0)), dict(line=(1.3e-7, -1.0, 1.67e-24, 0.0)),
                       dict(line=(1.3e-7, 606.0, 1.67e-24, -1.0))):
            refused(st, "FTTE_ERR_ARG", **change)
        assert _raw(st, tau=None, summary=None, **good) == code["FTTE_ERR_ARG"]           # nothing asked for
        # one leaf without a line width, on some sightlines only: decided before anything is written
        for bad in (0.0, -5.0, float("nan"), float("inf")):
            tgas = ingest["tgas"].copy()
            tgas[tgas.size // 2] = bad
            st.set_temperature(tgas)
            refused(st, "FTTE_ERR_ARG")
        refused(st, "FTTE_ERR_ARG", line=(1.3e-7, 606.0, 1e-320, 0.0))                      # 2 k T / mass overflows
        st.set_temperature(ingest["tgas"])
        assert _raw(st, tau=tau, summary=summary, **good) == 0 and np.all(tau >= 0.0) and np.all(summary[:, :, 0] > 0)  # and the context is still good
        held = st.counter("device_objects")
        assert held > idle
        # another grid: the velocity field and the working memory go, and nothing answers until medium and temperature are set
        u = golden("analysis_uniform16")
        st.set_grid(int(u["n"]), u["level"], float(u["box"]))
        assert st.counter("device_objects") < held and st.counter("spectra_velocity") == 0
        tau[:], summary[:] = -7.0, -7.0
        refused(st, "FTTE_ERR_STATE")
        # the owner: the same round trip with and without a velocity field and spectra leaves the same number of device objects
        counts = []
        for with_spectra in (False, True, True):
            st.set_grid(ingest["n"], ingest["level"], ingest["box"])
            st.set_medium(ingest["HI"], ingest["HI"], ingest["HI"], ingest["rho"], None, 0)
            st.set_temperature(ingest["tgas"])
            st.project_map(5, shape, mode=1, value=ingest["HI"])
            if with_spectra:
                st.set_velocity(*ingest["vel"])
                assert _raw(st, tau=tau, summary=summary, **good) == 0
            st.set_grid(int(u["n"]), u["level"], float(u["box"]))
            counts.append(st.counter("device_objects"))
        assert counts[0] == counts[1] == counts[2], counts
    with rt.StellarTransfer() as probe:
        assert probe.counter("device_objects") == idle                                    # close() released everything


def test_multi_device_context_refuses(golden):
    g = golden("analysis_uniform16")
    with rt.StellarTransfer(devices=[0, 0]) as st:
        st.set_grid(int(g["n"]), g["level"], float(g["box"]))
        for call in (lambda: st.set_velocity(g["HI"], g["HI"], g["HI"]), lambda: st.set_velocity(None, None, None),
                     lambda: st.sightline_spectra(1, (4, 4), 8, 0.0, 1e5, rt.LYMAN_ALPHA)):
            with pytest.raises(rt.FtteError) as err:
                call()
            assert err.value.status == "FTTE_ERR_UNSUPPORTED", str(err.value)


# ---- the batch loop, the chunk edges, the pixel passes and the second round of the gather: what a production map runs

LYA = rt.LYMAN_ALPHA


def assert_same_summaries(got, want, what=""):
    for key in ("N", "W", "dv90"):
        assert S.same_bits(got[key], want[key]), f"{what}: {key} differs"


def _sizes_are_the_restated_ones(st):
    """the tests below place their seams and edges by S.CHUNK and S.PASS_PIXELS (and, through tests/host/spectra_batch_check.cpp, by
    the budget of a batch and the lanes of a workgroup): another constant in the library fails here"""
    assert st.counter("spectra_chunk_segments") == S.CHUNK and st.counter("spectra_pass_pixels") == S.PASS_PIXELS


def _on_device(st, args, shape, nvel, with_tau, **more):
    """the _device variant into tensors filled with -7, as the host variant's dict"""
    import torch
    dev = torch.device("cuda", 0)
    tau = torch.full((shape[1], shape[0], nvel), -7.0, dtype=torch.float64, device=dev) if with_tau else None
    summary = torch.full((shape[1], shape[0], 3), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    st.sightline_spectra(*args, tau_device_ptr=tau.data_ptr() if with_tau else 0, summary_device_ptr=summary.data_ptr(), **more)
    torch.cuda.synchronize()
    out = {k: summary.cpu().numpy()[:, :, q].T for q, k in enumerate(("N", "W", "dv90"))}
    out["tau"] = tau.cpu().numpy().transpose(1, 0, 2) if with_tau else None
    return out


SEAM_N, SEAM_NVEL, SEAM_MOST = 64, 70, 2 * S.CHUNK + 3


@pytest.fixture(scope="module")
def seam_case():
    level = S.deep_levels(SEAM_N, S.seam_columns(SEAM_N, SEAM_NVEL, SEAM_MOST))
    case = dict(n=SEAM_N, level=level, **S.random_medium(level.size, SEAM_N))
    case["tree"] = A.Tree(SEAM_N, level)
    return case


@pytest.mark.parametrize("izone", [1, 5])
def test_batch_seams_with_spilled_lines_on_either_side(stellar, seam_case, izone):
    """a 64 x 64 map over a 64^3 grid whose lines hold 64 segments, but for columns refined (S.seam_columns) until the lines at the
    first and the last line of the map and on both sides of every batch seam hold 513 to 1027: three launches, the last one short,
    each with spilled lines of differing lengths in slots other than 0, and the working memory used again by the next.  The seams lie
    elsewhere where tau is staged (host arrays; tau absent: fit 2006) and where the spill alone decides (tau to a device array: fit
    2040), and the tree has columns for both.  izone 5 is the same tree with the depth mirrored and the map axes swapped (the check
    pass then numbers its lanes along the other axis)."""
    _sizes_are_the_restated_ones(stellar)
    case = seam_case
    load(stellar, case)
    shape, nvel, v0, dv, hubble = (SEAM_N, SEAM_N), SEAM_NVEL, -5.0e7, 1.0e8 / SEAM_NVEL, 1.0e-17
    seg = S.Segments(case["tree"], case["box"], izone, shape)
    counts = S.line_counts(seg)
    assert counts.max() == SEAM_MOST and counts.min() == SEAM_N
    staged, direct = S.seam_conditions(counts, nvel, True), S.seam_conditions(counts, nvel, False)
    assert len(staged) == len(direct) == 3 and staged[1][0] != direct[1][0]
    want = {line[1] > 0: S.map_lines(seg, case["HI"], case["tgas"], case["vel"], nvel, v0, dv, line, hubble) for line in (LYA, DOPPLER)}
    host = lambda line, **more: stellar.sightline_spectra(izone, shape, nvel, v0, dv, line, hubble=hubble, **more)  # noqa: E731
    device = lambda line, with_tau: _on_device(stellar, (izone, shape, nvel, v0, dv, line), shape, nvel, with_tau, hubble=hubble)  # noqa: E731
    runs = (("host arrays", LYA, True, lambda: host(LYA)),
            ("host arrays, tau staged and not asked for", DOPPLER, False, lambda: host(DOPPLER, want_tau=False)),
            ("_device, tau and summaries", DOPPLER, True, lambda: device(DOPPLER, True)),
            ("_device, summaries alone", LYA, False, lambda: device(LYA, False)))
    for what, line, with_tau, call in runs:
        for name in (what, what + ", the second call"):
            got = call()
            if with_tau:
                assert_same(got, want[line[1] > 0], f"izone {izone}, {name}")
            else:
                assert got["tau"] is None
                assert_same_summaries(got, want[line[1] > 0], f"izone {izone}, {name}")


def test_batch_seams_by_tau_alone(stellar):
    """no line beyond a chunk: 72 x 64 lines of four full pixel passes each stage 144 MiB of tau, in batches of 2046, 2046 and 516
    (the smallest map with three: the size is the budget's, not the grid's); a period equal to the span wraps every line's wings and
    the cores Hubble flow carries beyond the window"""
    _sizes_are_the_restated_ones(stellar)
    n, shape, nvel, izone = 4, (72, 64), 4 * S.PASS_PIXELS, 14
    bs = S.batches(shape[0] * shape[1], nvel, True, n)
    assert len(bs) == 3 and bs[0][1] == bs[1][1] > bs[2][1] and bs[0][1] % shape[0] != 0  # (a seam inside a row of the map)
    case = dict(n=n, level=np.zeros(n ** 3, dtype=np.int32), **S.random_medium(n ** 3, 72))
    load(stellar, case)
    span, hubble = 1.0e8, 2.0e-17
    v0, dv = -0.5 * span, span / nvel
    seg = S.Segments(A.Tree(n, case["level"]), case["box"], izone, shape)
    assert np.all(S.line_counts(seg) == n) and (hubble * seg.s + seg.velocity(case["vel"]) > v0 + span).any()
    want = S.map_lines(seg, case["HI"], case["tgas"], case["vel"], nvel, v0, dv, LYA, hubble, span)
    got = stellar.sightline_spectra(izone, shape, nvel, v0, dv, LYA, hubble=hubble, period=span)
    assert_same(got, want, "three batches of tau")
    assert got["tau"][:, :, -S.PASS_PIXELS:].min() > 0
    assert_same_summaries(stellar.sightline_spectra(izone, shape, nvel, v0, dv, LYA, hubble=hubble, period=span, want_tau=False), want, "the second call")


EDGE_NVEL = 2 * S.PASS_PIXELS + 17


@pytest.fixture(scope="module")
def edge_case():
    """a 4^3 grid with five refined columns: lines of a chunk, a chunk and one, two chunks, two and three, three and one.  The leaves of
    two of them move so that a tenth of the column absorbs at -3e7 cm/s and the rest five pixels from the upper end of a spectrum of
    EDGE_NVEL pixels over +-5e7 (the second line mirrored, for the izone that mirrors the depth): dv90 then spans all three passes"""
    n = 4
    columns = {(1, 2): S.CHUNK, (2, 1): S.CHUNK + 1, (3, 3): 2 * S.CHUNK, (0, 3): 2 * S.CHUNK + 3, (0, 0): 3 * S.CHUNK + 1}
    level = S.deep_levels(n, columns)
    case = dict(n=n, level=level, counts=sorted([n] * (n * n - len(columns)) + list(columns.values())), **S.random_medium(level.size, S.CHUNK))
    case["tree"] = A.Tree(n, level)
    seg = S.Segments(case["tree"], case["box"], 1, (n, n))
    far = -5.0e7 + (EDGE_NVEL - 4.5) * (1.0e8 / EDGE_NVEL)
    for (i, j), sign in (((0, 0), 1.0), ((0, 3), -1.0)):
        q = i * n + j
        leaves = seg.leaf[seg.off[q]:seg.off[q + 1]]
        column = case["HI"][leaves] * seg.size[seg.off[q]:seg.off[q + 1]]
        case["vel"][2][leaves] = sign * np.where(np.cumsum(column) <= 0.1 * column.sum(), -3.0e7, far)
    return case


@pytest.mark.parametrize("nvel", [S.PASS_PIXELS, 2 * S.PASS_PIXELS, EDGE_NVEL])
def test_chunk_edges_and_pixel_passes(stellar, edge_case, nvel):
    """one launch with lines of 4, 512 (the last count that stays in LDS), 513 (a second chunk of one record), 1024 (two full chunks:
    no remainder), 1027 and 1537 (a fourth chunk) segments, in slots other than 0, under izone 1 and under 5 (depth mirrored, map axes
    swapped); one full pass of pixels, two full passes, and two passes and 17 pixels, where dv90 of one line runs from the first pass
    into the third"""
    _sizes_are_the_restated_ones(stellar)
    case = edge_case
    load(stellar, case)
    shape, v0, dv = (4, 4), -5.0e7, 1.0e8 / nvel
    three_passes = nvel > 2 * S.PASS_PIXELS
    assert three_passes or nvel % S.PASS_PIXELS == 0
    hubble = 0.0 if three_passes else 2.0e-17
    for izone in (1, 5):
        seg = S.Segments(case["tree"], case["box"], izone, shape)
        counts = S.line_counts(seg)
        assert sorted(counts.tolist()) == case["counts"] and counts[0] > 3 * S.CHUNK and (counts[1:] > S.CHUNK).sum() == 3
        assert (counts == S.CHUNK).sum() == 1 and (counts == S.CHUNK + 1).sum() == 1 and (counts == 2 * S.CHUNK).sum() == 1
        for line in (LYA, DOPPLER):
            want = S.map_lines(seg, case["HI"], case["tgas"], case["vel"], nvel, v0, dv, line, hubble)
            got = stellar.sightline_spectra(izone, shape, nvel, v0, dv, line, hubble=hubble)
            if three_passes:
                run = np.cumsum(want["tau"].reshape(-1, nvel), axis=1)
                p_lo, p_hi = (run >= 0.05 * run[:, -1:]).argmax(axis=1), (run >= 0.95 * run[:, -1:]).argmax(axis=1)
                split = (p_lo < S.PASS_PIXELS) & (p_hi >= 2 * S.PASS_PIXELS)
                assert split.any() and np.diff(seg.off)[split].max() > S.CHUNK, (p_lo, p_hi)
                assert np.array_equal(want["dv90"].ravel()[split], (p_hi - p_lo)[split] * dv)
            assert_same(got, want, f"izone {izone} nvel {nvel} damping {line[1]}")
            assert_same(stellar.sightline_spectra(izone, shape, nvel, v0, dv, line, hubble=hubble), got, "the second call")


@pytest.mark.parametrize("most", [S.CHUNK, S.CHUNK + 1])
def test_the_longest_line_of_a_map_at_the_chunk_and_one_beyond(stellar, most):
    """the host gives a call a spill where its longest line exceeds a chunk, and the kernel spills a line that does: the two draw the
    line at the same count.  A map whose longest line holds exactly a chunk has no spill; with one record more the spill's stride is
    a chunk and one"""
    _sizes_are_the_restated_ones(stellar)
    n, shape, nvel, v0, dv = 4, (4, 4), 70, -5.0e7, 1.0e8 / 70
    level = S.deep_levels(n, {(2, 1): most})
    case = dict(n=n, level=level, **S.random_medium(level.size, most))
    load(stellar, case)
    T = A.Tree(n, level)
    for izone, line in ((1, LYA), (5, DOPPLER)):
        seg = S.Segments(T, case["box"], izone, shape)
        counts = S.line_counts(seg)
        assert counts.max() == most and (counts == n).sum() == n * n - 1 and counts[0] == n
        got = stellar.sightline_spectra(izone, shape, nvel, v0, dv, line, hubble=1.0e-17)
        assert_same(got, S.map_lines(seg, case["HI"], case["tgas"], case["vel"], nvel, v0, dv, line, 1.0e-17), f"izone {izone}")


def test_the_second_round_of_the_gather(stellar):
    """a uniform 257^3 grid, the whole depth: a workgroup's 256 lanes take the line's base cells 256 at a time, the grid is a cube and
    the window no deeper than it, so this is the smallest grid at which the gather takes a second round (one lane of it: the slots go
    on from the first round's total, the scan's buffers are used again).  Its time is the upload's: 17 million leaves, five fields."""
    _sizes_are_the_restated_ones(stellar)
    n, shape, nvel, v0, dv, hubble = S.LANES + 1, (3, 2), 64, -5.0e7, 1.0e8 / 64, 1.0e-17
    kstart, kend = A.map_depth(n)
    assert kend - kstart + 1 > S.LANES
    case = dict(n=n, level=np.zeros(n ** 3, dtype=np.int32), **S.random_medium(n ** 3, n))
    load(stellar, case)
    for izone in (1, 5, 15):  # (5: the depth against storage k; 15: against storage i, base cells n^2 leaves apart)
        seg = S.uniform_segments(n, case["box"], izone, shape)
        assert np.all(np.diff(seg.off) == n) and np.unique(seg.leaf).size == seg.leaf.size
        want = S.map_lines(seg, case["HI"], case["tgas"], case["vel"], nvel, v0, dv, LYA, hubble)
        assert_same(stellar.sightline_spectra(izone, shape, nvel, v0, dv, LYA, hubble=hubble), want, f"izone {izone}")
    stellar.set_grid(4, np.zeros(64, dtype=np.int32), case["box"])  # (the fixture does not hold 17 million leaves for the tests after this one)
