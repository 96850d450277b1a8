"""The sightline spectra on the GPU against the g++ evaluation of csrc/ftte_spectra_math.h on the segments the numpy walk finds
(tests/_spectra.py; held against an independent Voigt function, plain numpy and the projected map by test_spectra_host.py): tau, N, W
and dv90 bit for bit -- on the ingest golden under all 24 izones, on a uniform grid, on a tree whose one sightline spills over two
chunks and one pass of pixels; the _device variants, absent outputs, freshness, the refusals, the owner."""
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


def _deep_column(crossings, level, first):
    """the depth-first level list of a cell the sightline crosses `crossings` times: the two depth children on the line (the upper
    children along the map axes below a base cell, the lower ones further down: a pixel at the centre of its base cell) share them"""
    if crossings == 1:
        return [level]
    a = b = 1 if first else 0
    out = []
    for child in range(8):
        ca, cb, cc = child >> 2, (child >> 1) & 1, child & 1
        if (ca, cb) == (a, b):
            out += _deep_column(crossings // 2 if cc == 0 else crossings - crossings // 2, level + 1, False)
        else:
            out.append(level + 1)
    return out


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
                level += _deep_column(share[k], 0, True) if (i, j) == (0, 0) else [0]
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
