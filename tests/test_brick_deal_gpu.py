"""Option "nu_deal" of the brick sweep (brick_deal, csrc/ftte_brick_rec.h): which workgroup of a stage launch sweeps which (brick,
frequency group) pair.  It decides where work runs, never what is computed: every pair is still swept once, with the same inputs
and the same store-or-accumulate bit, so J with run lengths 1 and 16 is BYTE FOR BYTE the J of run length 0 (the placement
`work % nnu`), and for a single direction all three are the oracle's bits (device arithmetic), as in test_brick_gpu.py.

Every frequency group has opacities of its own (the first groups of an eight-group log-normal workload, s_nu = 1, 0.37, 0.14, ...),
so a workgroup that took another group's slot, or a pair swept twice or not at all, shows in J.

Forms: the whole-brick form (n = 64) with 1, 2, 3, 4, 5 and 8 groups on one and two streams; the general form on ragged bricks
(n = 70); the pair kernel (team = 2); the masked form of the hybrid sweep of a small refined tree.  Each with one direction per
izone alone, and with all 24 in one sweep (stages of many tasks: there the run length of 16 turns the groups too)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _oracle as O
import radiativetransfer_amd as rt
from radiativetransfer_amd import synthetic

pytestmark = pytest.mark.gpu

DEALS = (1, 16)
NNU_ALL = 8


def one_per_izone():
    phi, theta, _ = O.healpix_directions(3)
    pick = {}
    for p, t in zip(phi, theta):
        pick.setdefault(O.fold_direction(p, t)[2], (p, t))
    return [pick[z] for z in range(1, 25)]


def uniform_case(n):
    """Eight groups on an n^3 grid and the oracle's J of each of the 24 directions alone, computed once: groups do not touch each
    other, so the first k rows are the oracle's J of a sweep of the first k groups."""
    kappa, uvb, box = synthetic.uniform_workload(n, NNU_ALL, seed=n, tau_median=0.3)
    O.lib()

    def one(pt):
        phi, theta, w = np.array([pt[0]]), np.array([pt[1]]), np.array([0.37])
        ref = O.sweep_uniform(n, kappa, box, phi, theta, w, uvb, arith=O.ARITH_DEVICE)
        ref.setflags(write=False)
        return phi, theta, w, ref

    with ThreadPoolExecutor(max_workers=O.oracle_threads()) as pool:
        cases = list(pool.map(one, one_per_izone()))
    kappa.setflags(write=False)
    return n, kappa, uvb, box, cases


@pytest.fixture(scope="module")
def whole64():
    return uniform_case(64)


@pytest.fixture(scope="module")
def ragged70():
    return uniform_case(70)


@pytest.fixture
def bricks(engine):
    default = engine.counter("nu_deal")
    engine.set_option("engine", 2)
    yield engine
    for key, value in (("engine", 0), ("team", -1), ("chunk", 0), ("lanes", 2), ("nu_deal", default)):
        engine.set_option(key, value)


def check_uniform(eng, case, nnu, whole=None, form=None):
    n, kappa8, uvb8, box, cases = case
    kappa, uvb = np.ascontiguousarray(kappa8[:nnu]), uvb8[:nnu].copy()
    eng.set_uniform_grid(n, box)
    eng.set_opacity(kappa)

    def sweep(deal, phi, theta, w):
        eng.set_option("nu_deal", deal)
        J = eng.transport(phi, theta, w, uvb)
        assert eng.counter("brick_dataflow") == 0  # a launch per stage: the forms that take the deal
        if whole is not None:
            assert eng.counter("brick_whole") == whole
        if form is not None:
            assert eng.counter("brick_form") == form
        return J

    for phi, theta, w, ref in cases:
        J0 = sweep(0, phi, theta, w)
        izone = O.fold_direction(phi[0], theta[0])[2]
        assert np.array_equal(J0, ref[:nnu]), f"izone {izone}, nu_deal 0"
        for deal in DEALS:
            assert sweep(deal, phi, theta, w).tobytes() == J0.tobytes(), f"izone {izone}, nu_deal {deal}"
    phi = np.array([c[0][0] for c in cases]); theta = np.array([c[1][0] for c in cases]); w = np.full(len(cases), 1.0 / len(cases))
    J0 = sweep(0, phi, theta, w)
    for deal in DEALS:
        assert sweep(deal, phi, theta, w).tobytes() == J0.tobytes(), f"24 directions, nu_deal {deal}"


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("nnu", [1, 2, 3, 4, 5, 8])
def test_whole_bricks(bricks, whole64, nnu, lanes):
    bricks.set_option("team", 0)
    bricks.set_option("chunk", 4)  # 16 chunks x 8 rows of bricks per group: stages of up to 8 tasks per group of directions
    bricks.set_option("lanes", lanes)
    check_uniform(bricks, whole64, nnu, whole=1, form=0)


@pytest.mark.parametrize("nnu", [3, 8])
def test_ragged_bricks_general_form(bricks, ragged70, nnu):
    bricks.set_option("team", 0)
    bricks.set_option("chunk", 7)
    check_uniform(bricks, ragged70, nnu, whole=0, form=0)


@pytest.mark.parametrize("nnu", [2, 4])
def test_pair_kernel(bricks, whole64, nnu):
    bricks.set_option("team", 2)
    bricks.set_option("chunk", 4)
    check_uniform(bricks, whole64, nnu, form=2)


def test_masked_bricks_of_the_hybrid_sweep():
    """A refined block off the centre of a 64^3 grid, three groups: whole bricks outside the box, bricks the box cuts through
    (brick_kernel<..., MASKED>), the segment forest inside."""
    n, nnu = 64, 3
    blocks = [(30 + a, 31 + b, 33 + c) for a in range(3) for b in range(2) for c in range(4)]
    level = synthetic.refine_levels(n, blocks, depth=1)
    rho = synthetic.lognormal_density(len(level), seed=n)
    _, s_nu, uvb = synthetic.frequency_groups(nnu)
    kappa = (0.15 * n) * s_nu[:, None] * rho[None, :] * (2.0 ** level)[None, :]
    dirs = one_per_izone()
    with rt.DiffuseTransfer() as e:
        e.set_grid(n, level, 1.0)
        e.set_opacity(kappa)

        def sweep(deal, phi, theta, w):
            e.set_option("nu_deal", deal)
            return e.transport(phi, theta, w, uvb)

        for p, t in dirs:
            phi, theta, w = np.array([p]), np.array([t]), np.array([0.37])
            J0 = sweep(0, phi, theta, w)
            ref = O.sweep_tree(n, level, kappa, 1.0, phi, theta, w, uvb, arith=O.ARITH_DEVICE)
            assert np.array_equal(J0, ref), f"izone {O.fold_direction(p, t)[2]}, nu_deal 0"
            for deal in DEALS:
                assert sweep(deal, phi, theta, w).tobytes() == J0.tobytes(), f"izone {O.fold_direction(p, t)[2]}, nu_deal {deal}"
        assert e.counter("hybrid_boxes") >= 1  # the hybrid plan was taken
        phi = np.array([d[0] for d in dirs]); theta = np.array([d[1] for d in dirs]); w = np.full(len(dirs), 1.0 / len(dirs))
        J0 = sweep(0, phi, theta, w)
        for deal in DEALS:
            assert sweep(deal, phi, theta, w).tobytes() == J0.tobytes(), f"24 directions, nu_deal {deal}"
