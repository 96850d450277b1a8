"""A g++ shared library of one of the csrc `*_math.h` headers for the tests (tests/_chem_advance.py, _thermal.py, _thermochem.py):
built from a source under tests/host when that source or a header is newer, in a temporary directory where the tree is read-only,
renamed into place in one step, and loaded once."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")

# -ffp-contract=off: every product is rounded before the sum, as in the library's build
FLAGS = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-Wall", "-Werror"]
SANITIZE = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


class HostLib:
    """name: of the library (lib<name>.so beside its source); source: file under tests/host; headers: of csrc, local: of tests/host;
    what: for the error text; declare(L): sets the argtypes and restypes of the loaded library"""

    def __init__(self, name, source, headers, what, declare, local=()):
        self.name, self.what, self.declare = name, what, declare
        self.source = os.path.join(HERE, "host", source)
        self.deps = [self.source] + [os.path.join(CSRC, h) for h in headers] + [os.path.join(HERE, "host", h) for h in local]
        self.path = os.path.join(HERE, "host", f"lib{name}.so")
        self._lib = None

    def build(self):
        """the shared library, rebuilt when the source or a header is newer; in a temporary directory where the tree is read-only"""
        if os.path.exists(self.path) and all(os.path.getmtime(d) <= os.path.getmtime(self.path) for d in self.deps):
            return self.path
        gxx = shutil.which("g++")
        if not gxx:
            raise RuntimeError(f"no g++: the host evaluation of {self.what} cannot be built")
        if not os.access(os.path.dirname(self.path), os.W_OK):
            self.path = os.path.join(tempfile.mkdtemp(prefix=self.name + "_"), f"lib{self.name}.so")
        tmp = self.path + f".{os.getpid()}.tmp"
        subprocess.check_call([gxx, *FLAGS, "-shared", "-I" + CSRC, self.source, "-o", tmp])
        os.replace(tmp, self.path)
        return self.path

    def __call__(self):
        if self._lib is None:
            L = C.CDLL(self.build())
            self.declare(L)
            self._lib = L
        return self._lib


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
