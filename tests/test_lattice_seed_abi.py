"""rsrec_chebyshev_lattice is declared in include/rsrec.h, bound in rslmtoasa_amd/_lib.py and exported by the built library (no compute here)."""
import ctypes as C
import inspect
import os
import re

from rslmtoasa_amd import _lib
from rslmtoasa_amd.recursion import Recursion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rsrec_chebyshev_lattice"


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsrec.h")).read(), flags=re.S)


def test_symbol_in_header_binding_and_library():
    txt = header_text()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, txt)
    assert m, NAME + " is not declared in include/rsrec.h"
    params = [q.strip() for q in m.group(1).split(",")]
    assert len(params) == 11 and params[0].startswith("rsrec_t") and params[-1].replace(" ", "") == "double*m_g"
    assert re.search(r"#define\s+RSREC_LATTICE_NGROUP_MAX\s+16\b", txt)
    assert NAME in _lib.exported_symbols()
    res, args = _lib._SIGNATURES[NAME]
    assert res is C.c_int and len(args) == len(params)
    want = {"int": C.c_int, "double": C.c_double}
    for q, arg in zip(params, args):
        assert arg is (C.c_void_p if "*" in q else want[q.split()[0]]), q
    assert hasattr(_lib.lib(), NAME), "librsrec.so does not export " + NAME


def test_python_front_end():
    for name, params in (("chebyshev_lattice", ["seeds", "coefs", "group", "download"]), ("bloch_average", ["kpts", "cr", "group", "download"]),
                         ("bloch_average_spectral", ["green", "kpts", "cr", "group"]), ("cell_moments", ["rng", "group"])):
        got = list(inspect.signature(getattr(Recursion, name)).parameters)[1:]
        assert got[:len(params)] == params, (name, got)
        assert "kk" in getattr(Recursion, name).__doc__            # the docstrings state the normalisation
