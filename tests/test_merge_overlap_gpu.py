"""The brick sweep's J merge block by block behind the stages (option "merge_overlap" = 1, the default) against the single merge
after the last stage (0), and layout-1 direction groups marching through the layout-0 frame against the oracle.

The block merge adds each cell's accumulators in the same order as the single merge, so J must agree bit for bit; the layout-1
groups read the same opacities in the same order from another place, so one direction per izone still matches the oracle's device
arithmetic bit for bit.
"""
import numpy as np
import pytest

import _oracle as O
from radiativetransfer_amd import synthetic

pytestmark = pytest.mark.gpu

DEFAULTS = (("merge_overlap", 1), ("chunk", 0), ("share", 2), ("lanes", 2), ("engine", 0), ("team", -1))


@pytest.fixture
def eng(engine):
    yield engine
    for key, value in DEFAULTS:
        engine.set_option(key, value)


def directions(total):
    import radiativetransfer_amd as rt
    nside = 1
    while 12 * nside * nside < total:
        nside *= 2
    ang = np.array([rt.pix2ang_nest(nside, i) for i in range(total)])
    return ang[:, 0].copy(), ang[:, 1].copy(), np.full(total, 1.0 / total)


def both(eng, phi, theta, w, uvb):
    """J with the block merge, then with the single merge; checks that the block merge had several merge points."""
    eng.set_option("merge_overlap", 1)
    J1 = eng.transport(phi, theta, w, uvb)
    points, blocks = eng.counter("merge_points"), eng.counter("merge_blocks")
    assert points > 1 and blocks > 0
    assert eng.counter(f"merge_final_{points - 1}") == blocks
    assert eng.counter(f"merge_stage_{points - 1}") == eng.counter("brick_stages") - 1
    eng.set_option("merge_overlap", 0)
    J0 = eng.transport(phi, theta, w, uvb)
    return J1, J0


def test_bench_shape_bitwise(eng):
    """256^3 with the benchmark's 96 directions on two frequency groups (both lanes of streams in use)."""
    n, nnu = 256, 2
    kappa, uvb, box = synthetic.uniform_workload(n, nnu, seed=7)
    eng.set_uniform_grid(n, box)
    eng.set_opacity(kappa)
    phi, theta, w = directions(96)
    J1, J0 = both(eng, phi, theta, w, uvb)
    assert eng.counter("brick_accumulators_1") > 0
    assert np.array_equal(J1, J0)


@pytest.mark.parametrize("chunk", [4, 8, 16])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("share", [0, 1, 2])
@pytest.mark.parametrize("n", [77, 130])
def test_ragged_bitwise(eng, n, share, lanes, chunk):
    """Grids of ragged bricks and ragged merge blocks, every accumulator sharing rule, one or two streams of frequency groups (three
    groups: the lanes split them unevenly), several brick lengths."""
    nnu = 3
    kappa, uvb, box = synthetic.uniform_workload(n, nnu, seed=n + chunk, tau_median=0.3)
    eng.set_option("share", share)
    eng.set_option("lanes", lanes)
    eng.set_option("chunk", chunk)
    eng.set_uniform_grid(n, box)
    eng.set_opacity(kappa)
    phi, theta, w = directions(48)
    J1, J0 = both(eng, phi, theta, w, uvb)
    assert np.array_equal(J1, J0)


def one_per_izone():
    phi, theta, _ = O.healpix_directions(3)
    pick = {}
    for p, t in zip(phi, theta):
        pick.setdefault(O.fold_direction(p, t)[2], (p, t))
    return [pick[z] for z in range(1, 25)]


@pytest.mark.parametrize("team", [0, 2])
@pytest.mark.parametrize("n", [77, 130])
def test_every_izone_in_layout0_frame(eng, n, team):
    """One direction per izone, so every mirror of the layout-1 groups' frame, on ragged grids; both forms of the brick kernel.
    Bit for bit with the oracle's device arithmetic, with either merge."""
    kappa, uvb, box = synthetic.uniform_workload(n, 2, seed=3 * n, tau_median=0.3)
    eng.set_option("engine", 2)
    eng.set_option("team", team)
    eng.set_option("chunk", 8)
    eng.set_uniform_grid(n, box)
    eng.set_opacity(kappa)
    layout1 = 0
    for p, t in one_per_izone():
        phi, theta, w = np.array([p]), np.array([t]), np.array([0.37])
        ref = O.sweep_uniform(n, kappa, box, phi, theta, w, uvb, arith=O.ARITH_DEVICE)
        for overlap in (1, 0):
            eng.set_option("merge_overlap", overlap)
            J = eng.transport(phi, theta, w, uvb)
            assert np.array_equal(J, ref), f"izone {O.fold_direction(p, t)[2]}, merge_overlap {overlap}"
        layout1 += eng.counter("brick_accumulators_1")
    assert layout1 == 8  # the izones whose march runs along jc


def test_device_opacities_step_after_step(eng):
    """The benchmark's loop: opacities handed over on the device before every sweep (after the first sweep the copy and the layout-2
    transpose in one pass, layout 1 left out) give what a fresh upload gives."""
    import torch
    n, nnu = 96, 2
    phi, theta, w = directions(48)
    eng.set_uniform_grid(n, 1.0)
    dev = torch.device("cuda", 0)
    out = []
    for seed in (1, 2, 3):
        kappa, uvb, box = synthetic.uniform_workload(n, nnu, seed=seed, tau_median=0.3)
        k = torch.from_numpy(kappa).to(dev)
        eng.set_opacity_device(nnu, k.data_ptr())
        J = torch.empty((nnu, n ** 3), dtype=torch.float64, device=dev)
        eng.transport_device(phi, theta, w, uvb, J.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out.append((kappa, uvb, J.cpu().numpy().reshape(-1)))
    for kappa, uvb, J in out:
        eng.set_opacity(kappa)
        assert np.array_equal(eng.transport(phi, theta, w, uvb).reshape(-1), J)
