"""The population-slot entry points exist everywhere a host reaches them: exported by libftte.so, named in the version script,
declared in the header, bound for Fortran and for Python.  Needs the built library, no GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ftte_stellar_beta_tables", "ftte_set_population_tables", "ftte_get_population_tables", "ftte_point_sources_populations"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_resolves_in_the_library(name):
    lib = ctypes.CDLL(os.path.join(ROOT, "radiativetransfer_amd", "libftte.so"))
    assert getattr(lib, name) is not None


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_named_where_hosts_look(name):
    assert re.search(r"^\s*%s;" % name, _read("radiativetransfer_amd", "csrc", "ftte.map"), re.M)
    assert re.search(r"^int %s\(ftte_ctx \*ctx," % name, _read("include", "ftte.h"), re.M)
    assert "bind(C, name='%s')" % name in _read("fortran", "ftte_binding.f90")
    from radiativetransfer_amd import _lib
    assert name in _lib.SIGNATURES


def test_null_context_is_an_argument_error():
    from radiativetransfer_amd import _lib
    lib = _lib.load()
    assert _lib.STATUS[lib.ftte_set_population_tables(None, 1, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_get_population_tables(None, 0, None)] == "FTTE_ERR_ARG"
    assert _lib.STATUS[lib.ftte_point_sources_populations(None, 0, None, None, None, None)] == "FTTE_ERR_ARG"
    assert lib.ftte_counter(None, b"population_slots") == -1
