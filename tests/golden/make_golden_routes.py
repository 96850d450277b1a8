#!/usr/bin/env python3
"""Golden vectors for the cross-check of oracle/_ref/ref_harness's two routes through a direction: the reference's own driver
lines lifted from equiSources.f90:1393-1801 (what every golden is made with) and ref_harness.f90's own restatement of the same
steps, on a uniform and on a refined cell array, 48 directions of nAngularLevel = 2.  Needs oracle/_ref (make -C oracle ref).
Writes tests/golden/driver_routes.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as M  # noqa: E402
import _oracle  # noqa: E402
from radiativetransfer_amd import synthetic  # noqa: E402

BOX = 1.0


def directions():
    phi, theta, w = _oracle.healpix_directions(2)
    return phi, theta, w, synthetic.frequency_groups(3)[2]


def cases():
    """(n, level, kappa[3][ncell]): a 12^3 uniform grid and a 6^3 base grid with two blocks refined twice."""
    kap, _, _ = synthetic.uniform_workload(12, 3, seed=8, tau_median=0.4)
    level = synthetic.refine_levels(6, [(2, 2, 3), (5, 1, 4)], depth=2)
    return [(12, np.zeros(12 ** 3, np.int32), kap),
            (6, level, 2.0 * synthetic.frequency_groups(3)[1][:, None] * synthetic.lognormal_density(len(level), seed=3)[None, :])]


def run(n, level, kappa, lifted):
    phi, theta, w, uvb = directions()
    return M.run_reference(n, level, kappa, BOX, uvb, phi, theta, w, lifted=lifted)[0]


def main():
    phi, theta, w, uvb = directions()
    out = {"phi": phi, "theta": theta, "w": w, "uvb": uvb, "box": BOX}
    for c, (n, level, kappa) in enumerate(cases()):
        out.update({f"n{c}": n, f"level{c}": level, f"kappa{c}": kappa,
                    f"J{c}_lifted": run(n, level, kappa, True), f"J{c}_restated": run(n, level, kappa, False)})
    path = os.path.join(HERE, "driver_routes.npz")
    np.savez_compressed(path, **out)
    print(f"driver_routes: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
