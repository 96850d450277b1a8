"""Writes tests/golden/voigt_table.npz: the Voigt function H(a, x) = Re w(x + i a) from scipy's Faddeeva function, the independent
reference tests/test_spectra_host.py holds the profile of csrc/ftte_spectra_math.h against (the test itself does not import scipy).

    python tests/golden/make_golden_voigt.py

  a          the damping parameters: 1e-5, 4.7e-4 (HI Lyman alpha near 1e4 K), 4.7e-3
  x_core     linspace(0, 2, 2001);  x_mid  linspace(2, 8, 6001);  x_wing  geomspace(8, 1e4, 4000)
  x_switch   geomspace(1e-8, 0.05, 2000): across the header's switch at x^2 = 1e-4
  H_<grid>   [len(a)][len(x_<grid>)]
"""
import os

import numpy as np
from scipy.special import wofz

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    a = np.array([1.0e-5, 4.7e-4, 4.7e-3])
    grids = dict(core=np.linspace(0.0, 2.0, 2001), mid=np.linspace(2.0, 8.0, 6001), wing=np.geomspace(8.0, 1.0e4, 4000),
                 switch=np.geomspace(1.0e-8, 0.05, 2000))
    out = dict(a=a)
    for name, x in grids.items():
        out["x_" + name] = x
        out["H_" + name] = np.array([wofz(x + 1j * ai).real for ai in a])
    path = os.path.join(HERE, "voigt_table.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
