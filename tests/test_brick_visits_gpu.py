"""Two passes of an izone per visit (csrc/ftte_brick.hip, brick_duo_kernel: a workgroup of two wavefronts per seat, the helper's
sums reach J through the owner) against the oracle with the device arithmetic, through the C ABI.

Reference: O.sweep_uniform(..., arith=O.ARITH_DEVICE) per direction, summed in list order.  A cell's J is now
(J before + the owner's directions) + (0 + the helper's directions), visit after visit: another association of the same terms, so
the bound is SUM_RTOL = 64 eps, the project's bound for sums over directions, and no case is bitwise against the oracle.  CPU
pre-check (new_association below, asserted in the fixtures before anything runs on the GPU): the oracle's per-direction J added
in that association differs from the list-order sum by 9.73 eps for the 96 benchmark directions on n = 128 with 5 groups, by
2.95 eps for izone 22, 3.00 and 2.91 eps for izones 15, 20 and 23 on n = 128 and 64, and by 1.93, 1.59 and 0.50 eps on the thick,
the opaque and the all-zero field -- the reference is inside 64 eps on its own.

Every case asserts counter "brick_duo" (the linked seats of the plan: linked visits x bricks), "brick_whole" == 1, and a second
call equal to the first bit for bit.  The fallbacks (a chunk that does not divide the grid, the pair form) assert "brick_duo" == 0
and each other's bits: both are forms this change does not touch, and they agree bit for bit before and after it.
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
GMAX = 3  # directions per pass at two frequency groups and more


@pytest.fixture
def duo(engine):
    engine.set_option("engine", 2)
    yield engine
    for key, value in OPTIONS:
        engine.set_option(key, value)


def bench_directions():
    """The benchmark's 96 directions (the first 96 NESTED pixels of nside 4) and the izone of each."""
    phi, theta, w = O.healpix_directions(3, 96)
    izone = np.array([O.fold_direction(p, t)[2] for p, t in zip(phi, theta)])
    return phi, theta, w, izone


def passes_of(members):
    """The passes of an izone as the planner forms them: as few as GMAX allows, of equal size where possible."""
    npass = (len(members) + GMAX - 1) // GMAX
    out, b = [], 0
    for q in range(npass):
        size = len(members) // npass + (1 if q < len(members) % npass else 0)
        out.append(members[b:b + size])
        b += size
    return out


def new_association(parts, izone):
    """The per-direction J `parts` (list order) added the way the visits add them: per izone visit after visit, a linked visit as
    (sum so far + the owner's directions) + (0 + the helper's directions); then the izones.  (Which izones share an accumulator, and
    the turn p(i) of a layer's directions, move terms within these sums as they did before.)"""
    total = None
    for z in sorted(set(izone.tolist())):
        acc = None
        passes = passes_of([d for d in range(len(parts)) if izone[d] == z])
        for v in range(0, len(passes), 2):
            for d in passes[v]:
                acc = parts[d].copy() if acc is None else acc + parts[d]
            if v + 1 < len(passes):
                helper = np.zeros_like(acc)
                for d in passes[v + 1]:
                    helper = helper + parts[d]
                acc = acc + helper
        total = acc if total is None else total + acc
    return total


def per_direction(n, kappa, box, phi, theta, w, uvb):
    O.lib()
    with ThreadPoolExecutor(max_workers=O.oracle_threads()) as pool:
        parts = list(pool.map(lambda d: O.sweep_uniform(n, kappa, box, phi[d:d + 1], theta[d:d + 1], w[d:d + 1], uvb, arith=O.ARITH_DEVICE), range(len(phi))))
    for p in parts:
        p.setflags(write=False)
    return parts


def list_order_sum(parts, dirs):
    ref = None
    for d in dirs:
        ref = parts[d].copy() if ref is None else ref + parts[d]
    return ref


def rel_dev(a, ref):
    """Largest |a - ref| / ref; a cell where the reference is zero (complete extinction) must be zero."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.max(np.where(ref != 0, np.abs(a - ref) / ref, np.where(a == 0, 0.0, np.inf)))


def precheck(parts, izone, dirs, what):
    """The reference against itself: the new association of the oracle's terms inside SUM_RTOL of their list-order sum."""
    ref = list_order_sum(parts, dirs)
    alt = new_association([parts[d] for d in dirs], izone[dirs])
    dev = rel_dev(alt, ref)
    print(f"{what}: new association of the oracle's terms differs from their list-order sum by {dev / EPS:.2f} eps")
    assert dev <= SUM_RTOL
    ref.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def wide():
    """n = 128 (2 x 16 bricks across: u- and v-faces are exchanged), 5 frequency groups, the 96 benchmark directions one by one."""
    n = 128
    kappa, uvb, box = synthetic.uniform_workload(n, 5, seed=n, tau_median=0.3)
    phi, theta, w, izone = bench_directions()
    counts = {z: int(np.sum(izone == z)) for z in set(izone.tolist())}
    assert len(counts) == 16 and counts[22] == 11 and counts[15] == 7 and counts[20] == 1 and counts[23] == 2
    return n, kappa, uvb, box, phi, theta, w, izone, per_direction(n, kappa, box, phi, theta, w, uvb)


def run(eng, n, box, kappa, uvb, phi, theta, w, ref, linked, what):
    eng.set_uniform_grid(n, box)
    eng.set_opacity(np.ascontiguousarray(kappa))
    J = eng.transport(phi, theta, w, uvb)
    assert eng.counter("brick_duo") == linked and eng.counter("brick_whole") == 1
    again = eng.transport(phi, theta, w, uvb)
    assert np.array_equal(J, again)  # a fixed order: reproducible bit for bit
    print(f"{what}: max relative difference from the oracle {rel_dev(J, ref) / EPS:.2f} eps")
    assert np.allclose(J, ref, rtol=SUM_RTOL, atol=0)
    return J


@pytest.mark.parametrize("chunk", [16, 1])
def test_four_passes(duo, wide, chunk):
    """The 11 directions of izone 22: four passes, two linked visits, the second accumulating onto the first.  chunk 1: a layer
    per brick, where the prologue and the exchange meet at every layer."""
    n, kappa, uvb, box, phi, theta, w, izone, parts = wide
    dirs = np.flatnonzero(izone == 22)
    ref = precheck([p[:2] for p in parts], izone, dirs, "izone 22")
    duo.set_option("team", 0)
    duo.set_option("chunk", chunk)
    bricks = (n // 64) * (n // 8) * (n // chunk)
    run(duo, n, box, kappa[:2], uvb[:2], phi[dirs], theta[dirs], w[dirs], ref, 2 * bricks, f"four passes, chunk {chunk}")


def odd_set(izone):
    """izone 15 (7 directions: a linked visit and a lone pass that accumulates), izone 20 (one direction) and izone 23, of opposite
    parity to 15 in the same layout for one and for two bricks across: it shares 15's accumulator."""
    return np.flatnonzero(np.isin(izone, (15, 20, 23)))


def test_odd_passes_two_bricks_wide(duo, wide):
    n, kappa, uvb, box, phi, theta, w, izone, parts = wide
    dirs = odd_set(izone)
    ref = precheck([p[:2] for p in parts], izone, dirs, "izones 15, 20, 23")
    duo.set_option("team", 0)
    duo.set_option("chunk", 16)
    run(duo, n, box, kappa[:2], uvb[:2], phi[dirs], theta[dirs], w[dirs], ref, (n // 64) * (n // 8) * (n // 16), "odd passes, n 128")
    assert duo.counter("brick_groups") == 5 and duo.counter("brick_accumulators") == 2  # 15 and 23 share one, 20 has its own


def test_odd_passes_one_brick_wide(duo):
    """n = 64: one brick across, domain faces only."""
    n = 64
    kappa, uvb, box = synthetic.uniform_workload(n, 2, seed=n, tau_median=0.3)
    phi, theta, w, izone = bench_directions()
    dirs = odd_set(izone)
    parts = dict(zip(dirs.tolist(), per_direction(n, kappa, box, phi[dirs], theta[dirs], w[dirs], uvb)))
    ref = precheck(parts, izone, dirs, "izones 15, 20, 23, n 64")
    duo.set_option("team", 0)
    duo.set_option("chunk", 16)
    run(duo, n, box, kappa, uvb, phi[dirs], theta[dirs], w[dirs], ref, (n // 8) * (n // 16), "odd passes, n 64")
    assert duo.counter("brick_groups") == 5 and duo.counter("brick_accumulators") == 2


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
    return np.where(mask, tau_planted, 0.01).reshape(1, n ** 3)


FIELDS = {
    "planted_thick": lambda n: planted(n, 2.0),
    "planted_opaque": lambda n: planted(n, 1.0e4),  # complete extinction: Iout = 0, and Iin = 0 downstream
    "zero": lambda n: np.zeros((1, n ** 3)),
}


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_hard_fields(duo, field):
    """One linked visit (the 6 directions of izone 3) on n = 64."""
    n, box = 64, 1.0
    kappa = np.ascontiguousarray(FIELDS[field](n) * n)  # kappa dx = the optical depth of a cell
    uvb = np.array([1.0])
    phi, theta, w, izone = bench_directions()
    dirs = np.flatnonzero(izone == 3)
    assert len(dirs) == 6
    parts = dict(zip(dirs.tolist(), per_direction(n, kappa, box, phi[dirs], theta[dirs], w[dirs], uvb)))
    ref = precheck(parts, izone, dirs, field)
    duo.set_option("team", 0)
    duo.set_option("chunk", 16)
    run(duo, n, box, kappa, uvb, phi[dirs], theta[dirs], w[dirs], ref, (n // 8) * (n // 16), field)
    assert bool(np.any(ref == 0.0)) == (field == "planted_opaque")  # the opaque cells really put rays out, nothing else does


def test_bench_set(duo, wide):
    """All 96 benchmark directions, 5 frequency groups, default options: 36 passes in 23 visits, 13 of them linked."""
    n, kappa, uvb, box, phi, theta, w, izone, parts = wide
    ref = precheck(parts, izone, np.arange(96), "the 96 benchmark directions")
    for key, value in OPTIONS:
        duo.set_option(key, value)
    run(duo, n, box, kappa, uvb, phi, theta, w, ref, 13 * (n // 64) * (n // 8) * (n // 16), "bench set")
    assert duo.counter("brick_groups") == 36 and duo.counter("brick_form") == 0


def test_fallbacks_sweep_single_passes(duo, wide):
    """The directions of the four passes at chunk 7 (no multiple of the grid) and with the pair form: no visit is shared, and the
    two untouched forms agree bit for bit as they always have."""
    n, kappa, uvb, box, phi, theta, w, izone, parts = wide
    dirs = np.flatnonzero(izone == 22)
    ref = list_order_sum([p[:2] for p in parts], dirs)
    duo.set_uniform_grid(n, box)
    duo.set_opacity(np.ascontiguousarray(kappa[:2]))
    duo.set_option("team", 0)
    duo.set_option("chunk", 7)
    J7 = duo.transport(phi[dirs], theta[dirs], w[dirs], uvb[:2])
    assert duo.counter("brick_duo") == 0 and duo.counter("brick_whole") == 1 and duo.counter("brick_form") == 0
    duo.set_option("team", 2)
    duo.set_option("chunk", 16)
    J2 = duo.transport(phi[dirs], theta[dirs], w[dirs], uvb[:2])
    assert duo.counter("brick_duo") == 0 and duo.counter("brick_whole") == 0 and duo.counter("brick_form") == 2
    assert np.array_equal(J7, J2)
    assert np.allclose(J7, ref, rtol=SUM_RTOL, atol=0)
