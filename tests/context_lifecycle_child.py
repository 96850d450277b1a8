"""Child process of test_context_lifecycle_gpu.py: contexts driven through every path that keeps device buffers, streams or
events, destroyed, and made anew.  ftte_counter "device_objects" counts the owned objects alive in the process, so it runs in a
process of its own.  Prints "context lifecycle OK" or raises."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import radiativetransfer_amd as rt  # noqa: E402
from radiativetransfer_amd import synthetic  # noqa: E402


def golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def directions(level):
    phi, theta = np.array([rt.pix2ang_nest(level, i) for i in range(12 * level * level)]).T
    return phi.copy(), theta.copy(), np.full(phi.size, 1.0 / phi.size)


def uniform_kappa(n, nnu, seed):
    rho = synthetic.lognormal_density(n ** 3, seed=seed)
    _, s_nu, uvb = synthetic.frequency_groups(nnu)
    return (0.15 * n) * s_nu[:, None] * rho[None, :], uvb


def refined_case(n, nnu, seed):
    """A cube of 32^3 base cells refined once: the hybrid sweep gives it a fine block (tests/test_hybrid_gpu.py)."""
    blocks = [(16 + a, 16 + b, 16 + c) for a in range(32) for b in range(32) for c in range(32)]
    level = synthetic.refine_levels(n, blocks, depth=1)
    rho = synthetic.lognormal_density(len(level), seed=seed)
    _, s_nu, uvb = synthetic.frequency_groups(nnu)
    return level, (0.15 * n) * s_nu[:, None] * rho[None, :] * (2.0 ** level)[None, :], uvb


def diffuse_round(e, multi):
    """What a multi-device context takes as well; returns J of the first uniform sweep."""
    n = 64
    phi, theta, w = directions(1)
    e.set_uniform_grid(n, 1.0)
    k2, uvb2 = uniform_kappa(n, 2, seed=7)
    k4, uvb4 = uniform_kappa(n, 4, seed=8)
    e.set_opacity(k2)
    J_first = e.transport(phi, theta, w, uvb2)
    e.set_opacity(k4)                                  # more frequency groups: every buffer sized by them grows
    e.transport(phi, theta, w, uvb4)
    e.set_opacity(k2)                                  # fewer again, with emission once
    e.set_emissivity(1e-3 * k2)
    e.transport(phi, theta, w, uvb2)
    e.set_emissivity(None)

    level, kappa, uvb = refined_case(n, 2, seed=41)
    e.set_grid(n, level, 1.0)
    e.set_opacity(kappa)
    e.transport(phi[:3], theta[:3], w[:3], uvb)        # hybrid sweep
    if not multi:
        assert e.counter("fine_block") == 64, e.counter("fine_block")
    e.set_option("forest", 1)                          # the whole tree through the segment forests
    e.transport(phi[:2], theta[:2], w[:2], uvb)
    e.set_option("forest", 0)
    J = np.empty_like(kappa)                           # pageable host arrays
    e.iterate_into(kappa, phi[:3], theta[:3], w[:3], uvb, J)
    return J_first


def stellar_round(e):
    g = golden("chem_uvb_refined")
    tabs = golden("point16_homogeneous")["tables"]
    nc = g["level"].size
    e.set_grid(int(g["n"]), g["level"], float(g["box"]))
    e.set_rate_coefficients(float(g["logtem0"]), float(g["logtem9"]), float(g["dlogtem"]), g["k"])
    e.set_medium(g["HI"], g["HeI"], g["HeII"], g["rho"], None, 0)
    e.set_temperature(g["tgas"])
    e.set_rate_tables(tabs)
    e.set_zero_rates()
    e.point_sources(np.array([5, nc // 2]), np.array([50.0, 20.0]))
    e.solve_rate_equations(True, g["J"], g["ksi"], use_point_rates=True)
    neutral, total = e.hydrogen_mass()
    assert 0.0 < neutral < total


def last_steps(e):
    """A different uniform grid (everything sized by the old one goes), swept through the host-array lanes."""
    n = 48
    phi, theta, w = directions(1)
    e.set_uniform_grid(n, 1.0)
    kappa, uvb = uniform_kappa(n, 4, seed=9)
    J = np.empty_like(kappa)
    e.iterate_into(kappa, phi, theta, w, uvb, J)
    e.iterate_into(kappa, phi, theta, w, uvb, J)


def main():
    e = rt.StellarTransfer()
    n0 = e.counter("device_objects")
    assert n0 >= 1, n0                                 # the context's stream
    J_rounds = []
    for _ in range(3):
        J_rounds.append(diffuse_round(e, multi=False))
        stellar_round(e)
        last_steps(e)
        assert e.counter("device_objects") > n0
        e.close()
        e = rt.StellarTransfer()
        assert e.counter("device_objects") == n0, (e.counter("device_objects"), n0)
    assert np.array_equal(J_rounds[0], J_rounds[2]) and np.all(np.isfinite(J_rounds[0])) and J_rounds[0].max() > 0
    e.close()

    m = rt.DiffuseTransfer(devices=[0, 0])
    m0 = m.counter("device_objects")
    assert m0 == 2 * n0, (m0, n0)                      # nothing of the single-device contexts is left
    diffuse_round(m, multi=True)
    last_steps(m)
    assert m.counter("device_objects") > m0
    m.close()
    m = rt.DiffuseTransfer(devices=[0, 0])
    assert m.counter("device_objects") == m0, (m.counter("device_objects"), m0)
    m.close()
    print("context lifecycle OK")


if __name__ == "__main__":
    main()
