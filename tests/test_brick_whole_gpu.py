"""The whole-brick form of the brick sweep (csrc/ftte_brick.hip, brick_kernel<4, 0, 0, false, true>: grids that are a multiple of
64, one wavefront per brick) against the oracle with the device arithmetic, through the C ABI.

In this form row 0 of a brick takes the ray from the brick below at the END of a shape step (brick_step), and the hand-over to the
brick on the right is a buffer store every lane issues.  Neither changes an operand or the order of a sum: a single direction is
the oracle's bits, several agree to the rounding of their sum (SUM_RTOL, as in test_brick_gpu.py).  Every case asserts counter
"brick_whole": none passes by running another form.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _oracle as O
from radiativetransfer_amd import synthetic

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SUM_RTOL = 64 * EPS
OPTIONS = (("engine", 0), ("team", -1), ("chunk", 0), ("group", 0))


@pytest.fixture
def whole(engine):
    engine.set_option("engine", 2)
    engine.set_option("team", 0)  # one wavefront per brick: the pair kernel has no whole-brick form
    yield engine
    for key, value in OPTIONS:
        engine.set_option(key, value)


def one_per_izone():
    """24 directions, one per izone: every rotation of the memory frame, every chain class, both orders of a three-piece sum."""
    phi, theta, _ = O.healpix_directions(3)
    pick = {}
    for p, t in zip(phi, theta):
        pick.setdefault(O.fold_direction(p, t)[2], (p, t))
    return [pick[z] for z in range(1, 25)]


def oracle_per_direction(n, kappa, box, uvb):
    """The oracle's J of each of the 24 directions alone (the calls side by side: the oracle has no mutable globals)."""
    O.lib()

    def one(pt):
        phi, theta, w = np.array([pt[0]]), np.array([pt[1]]), np.array([0.37])
        ref = O.sweep_uniform(n, kappa, box, phi, theta, w, uvb, arith=O.ARITH_DEVICE)
        ref.setflags(write=False)
        return phi, theta, w, ref

    with ThreadPoolExecutor(max_workers=O.oracle_threads()) as pool:
        return list(pool.map(one, one_per_izone()))


@pytest.fixture(scope="module")
def two_bricks_wide():
    """n = 128: 2 x 16 bricks across, so both the u-faces and the v-faces are exchanged; two frequency groups."""
    n = 128
    kappa, uvb, box = synthetic.uniform_workload(n, 2, seed=n, tau_median=0.3)
    return n, kappa, uvb, box, oracle_per_direction(n, kappa, box, uvb)


@pytest.mark.parametrize("chunk", [16, 7, 1])
def test_every_izone_bitwise(whole, two_bricks_wide, chunk):
    n, kappa, uvb, box, cases = two_bricks_wide
    whole.set_option("chunk", chunk)
    whole.set_uniform_grid(n, box)
    whole.set_opacity(kappa)
    for phi, theta, w, ref in cases:
        J = whole.transport(phi, theta, w, uvb)
        assert whole.counter("brick_whole") == 1
        assert np.array_equal(J, ref), f"izone {O.fold_direction(phi[0], theta[0])[2]}"


def planted(n, tau_planted):
    """kappa dx = 0.01, and tau_planted on every cell where one coordinate is 0 or 7 (mod 8) and another 0 or 63 (mod 64): the
    first and last row and the first and last lane of a brick, whichever axes a rotation makes rows and lanes of."""
    c = np.arange(n)
    row = np.isin(c % 8, (0, 7))
    lane = np.isin(c % 64, (0, 63))
    mask = np.zeros((n, n, n), bool)
    for a in range(3):
        for b in range(3):
            if a != b:
                shape_a, shape_b = [1, 1, 1], [1, 1, 1]
                shape_a[a] = shape_b[b] = n
                mask |= row.reshape(shape_a) & lane.reshape(shape_b)
    tau = np.where(mask, tau_planted, 0.01)
    return tau.reshape(1, n ** 3)


FIELDS = {
    "planted_thick": lambda n: planted(n, 2.0),
    "planted_opaque": lambda n: planted(n, 1.0e4),  # complete extinction: Iout = 0, and Iin = 0 downstream
    "zero": lambda n: np.zeros((1, n ** 3)),
    "all_thick": lambda n: np.full((1, n ** 3), 5.0),
}


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_planted_fields_bitwise(whole, field):
    n, box = 64, 1.0
    kappa = np.ascontiguousarray(FIELDS[field](n) * n)  # kappa dx = the optical depth of a cell
    uvb = np.array([1.0])
    whole.set_option("chunk", 16)
    whole.set_uniform_grid(n, box)
    whole.set_opacity(kappa)
    extinct = False
    for phi, theta, w, ref in oracle_per_direction(n, kappa, box, uvb):
        J = whole.transport(phi, theta, w, uvb)
        assert whole.counter("brick_whole") == 1
        assert np.array_equal(J, ref), f"izone {O.fold_direction(phi[0], theta[0])[2]}"
        extinct |= bool(np.any(ref == 0.0))
    assert extinct == (field == "planted_opaque")  # the opaque cells really put rays out, nothing else does


@pytest.fixture(scope="module")
def full_set():
    """n = 128, the 192 directions of nside 4, three frequency groups.  (The oracle adds a direction's w * mean into J in the order
    of the directions, starting from nothing: one call per direction, side by side, added in that order is one call's bits.)"""
    n = 128
    kappa, uvb, box = synthetic.uniform_workload(n, 3, seed=11, tau_median=0.2)
    phi, theta, w = O.healpix_directions(3)
    O.lib()
    with ThreadPoolExecutor(max_workers=O.oracle_threads()) as pool:
        ref = None
        for part in pool.map(lambda d: O.sweep_uniform(n, kappa, box, phi[d:d + 1], theta[d:d + 1], w[d:d + 1], uvb, arith=O.ARITH_DEVICE), range(len(phi))):
            ref = part if ref is None else ref + part
    ref.setflags(write=False)
    return n, kappa, uvb, box, phi, theta, w, ref


@pytest.mark.parametrize("group", [3, 2])
def test_groups_of_directions(whole, full_set, group):
    n, kappa, uvb, box, phi, theta, w, ref = full_set
    whole.set_option("group", group)
    whole.set_option("chunk", 16)
    whole.set_uniform_grid(n, box)
    whole.set_opacity(kappa)
    J = whole.transport(phi, theta, w, uvb)
    assert whole.counter("brick_whole") == 1
    J_again = whole.transport(phi, theta, w, uvb)
    assert np.array_equal(J, J_again)  # no atomics, a fixed order: reproducible bit for bit
    print("max relative difference from the oracle:", np.max(np.abs(J - ref) / ref) / EPS, "eps")
    assert np.allclose(J, ref, rtol=SUM_RTOL, atol=0)
