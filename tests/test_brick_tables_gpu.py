"""The device tables of the brick plans and the buffers that remember what they were sent (csrc/ftte_bricks.h) through whole sweeps:
one context that goes from grid to grid, from one number of frequency groups to another, through emission and brick order, and from
direction list to direction list must give, sweep for sweep, exactly the J of a fresh context that has seen nothing else.  The
uniform grid's plan and the hybrid sweep's base plan share one set of tables, the fine block has its own, and the group records and
the background are copied only when their bytes change: every comparison is bit for bit."""
import numpy as np
import pytest

import _oracle as O
import radiativetransfer_amd as rt
from radiativetransfer_amd import synthetic

pytestmark = pytest.mark.gpu


def uniform_case(n, nnu, seed):
    rho = synthetic.lognormal_density(n ** 3, seed=seed)
    _, s_nu, uvb = synthetic.frequency_groups(nnu)
    return (0.15 * n) * s_nu[:, None] * rho[None, :], uvb


def patch_case(n, blocks, nnu, seed):
    level = synthetic.refine_levels(n, blocks, depth=1)
    rho = synthetic.lognormal_density(len(level), seed=seed)
    _, s_nu, uvb = synthetic.frequency_groups(nnu)
    return level, (0.15 * n) * s_nu[:, None] * rho[None, :] * (2.0 ** level)[None, :], uvb


def fresh(n, level, kappa, uvb, dirs, prepare=None):
    """J of a context that has seen this grid and this state only"""
    with rt.DiffuseTransfer() as e:
        if level is None:
            e.set_uniform_grid(n, 1.0)
        else:
            e.set_grid(n, level, 1.0)
        e.set_opacity(kappa)
        if prepare:
            prepare(e)
        return e.transport(*dirs, uvb)


def test_uniform_and_hybrid_plans_share_their_tables_across_grids():
    dirs = O.healpix_directions(2)
    k64, uvb2 = uniform_case(64, 2, seed=3)
    k72, _ = uniform_case(72, 2, seed=4)  # ragged: 72 = 64 + 8, the kernel does not take the whole-brick form
    blocks = [(28 + a, 30 + b, 31 + c) for a in range(4) for b in range(4) for c in range(3)]  # test_hybrid_equals_whole_tree_forest_path
    level, kref, uvb3 = patch_case(64, blocks, 3, seed=5)
    with rt.DiffuseTransfer() as e:
        e.set_uniform_grid(64, 1.0)
        e.set_opacity(k64)
        J64 = e.transport(*dirs, uvb2)
        e.set_grid(64, level, 1.0)
        e.set_opacity(kref)
        Jref = e.transport(*dirs, uvb3)
        assert e.counter("hybrid_boxes") == 1
        e.set_uniform_grid(72, 1.0)
        e.set_opacity(k72)
        J72 = e.transport(*dirs, uvb2)
        assert e.counter("hybrid_boxes") == 0
        e.set_grid(64, level, 1.0)
        e.set_opacity(kref)
        Jref_again = e.transport(*dirs, uvb3)
        assert e.counter("hybrid_boxes") == 1
    assert np.array_equal(J64, fresh(64, None, k64, uvb2, dirs))
    Jref_fresh = fresh(64, level, kref, uvb3, dirs)
    assert np.array_equal(Jref, Jref_fresh)
    assert np.array_equal(J72, fresh(72, None, k72, uvb2, dirs))
    assert np.array_equal(Jref_again, Jref_fresh)
    assert np.all(J64 > 0) and np.all(Jref > 0) and np.all(J72 > 0)


def test_group_records_follow_what_they_name():
    n = 64
    dirs = O.healpix_directions(2)
    k2, uvb2 = uniform_case(n, 2, seed=7)
    k3, uvb3 = uniform_case(n, 3, seed=8)
    S = 0.3 * uvb2[:, None] * synthetic.lognormal_density(n ** 3, seed=9)[None, :]
    with rt.DiffuseTransfer() as e:
        e.set_uniform_grid(n, 1.0)
        e.set_opacity(k2)
        J2 = e.transport(*dirs, uvb2)
        e.set_opacity(k3)
        J3 = e.transport(*dirs, uvb3)
        e.set_opacity(k2)
        J2_again = e.transport(*dirs, uvb2)
        e.set_source_function(S)
        J2_source = e.transport(*dirs, uvb2)
        e.set_source_function(None)
        J2_plain = e.transport(*dirs, uvb2)
        e.set_option("tiled", 1)
        J2_tiled = e.transport(*dirs, uvb2)
        e.set_option("tiled", 0)
        J2_rows = e.transport(*dirs, uvb2)
    J2_fresh = fresh(n, None, k2, uvb2, dirs)
    assert np.array_equal(J2, J2_fresh)
    assert np.array_equal(J3, fresh(n, None, k3, uvb3, dirs))
    assert np.array_equal(J2_again, J2_fresh) and np.array_equal(J2_again, J2)
    assert np.array_equal(J2_source, fresh(n, None, k2, uvb2, dirs, lambda f: f.set_source_function(S)))
    assert not np.array_equal(J2_source, J2)
    assert np.array_equal(J2_plain, J2_fresh)
    assert np.array_equal(J2_tiled, fresh(n, None, k2, uvb2, dirs, lambda f: f.set_option("tiled", 1)))
    assert np.array_equal(J2_rows, J2_fresh)


def test_fine_block_keeps_tables_of_its_own():
    n, lo = 64, (16, 16, 16)  # test_fine_block_swept_by_bricks_of_its_own_every_izone_bitwise
    blocks = [(lo[0] + a, lo[1] + b, lo[2] + c) for a in range(32) for b in range(32) for c in range(32)]
    level, kappa, uvb = patch_case(n, blocks, 2, seed=41)
    phi, theta, _ = O.healpix_directions(3)
    pick = {}
    for p, t in zip(phi, theta):
        pick.setdefault(O.fold_direction(p, t)[2], (p, t))
    def some(zones):
        return (np.array([pick[z][0] for z in zones]), np.array([pick[z][1] for z in zones]), np.full(len(zones), 1.0 / len(zones)))
    first, other = some([1, 8, 14, 23]), some([3, 10, 17, 20, 24])
    with rt.DiffuseTransfer() as e:
        e.set_grid(n, level, 1.0)
        e.set_opacity(kappa)
        J_a = e.transport(*first, uvb)
        assert e.counter("fine_block") == 64
        J_b = e.transport(*first, uvb)
        J_c = e.transport(*other, uvb)
        assert e.counter("fine_block") == 64
        J_d = e.transport(*first, uvb)
        assert e.counter("fine_block") == 64
    J_first = fresh(n, level, kappa, uvb, first)
    assert np.array_equal(J_a, J_first) and np.array_equal(J_b, J_first) and np.array_equal(J_d, J_first)
    assert np.array_equal(J_c, fresh(n, level, kappa, uvb, other))
    assert not np.array_equal(J_c, J_first)
