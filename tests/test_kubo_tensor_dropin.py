"""Several responses to several applied fields through the zero-edit drop-in (oracle/_ref/rslmto_dropin.x, tests/test_fortran_dropin.py
has the machinery): with RSREC_KUBO_FIELDS=y and RSREC_KUBO_RESPONSES=spin recursion_gpu%compute_moments_stochastic forms the diagonal
moments of the four (response, field) pairs (charge | spin) x (x | y) in one rsrec_kubo_moments_diag_tensor call, and conductivity_gpu
writes the namelist pair's files under the reference's names, the further response's with the prefix spin_, the further field's with
Ey_ and Ey_spin_.  The conductivity_fccPt case (v_alpha = y, v_beta = x), per_type (its vectors are not drawn at random, so runs have
the same input), patched to linear_out = 'charge':
  A  RSREC_KUBO_FIELDS=y RSREC_KUBO_RESPONSES=spin;
  B .. E  RSREC_KUBO_DIAG=1 and neither variable, one run per pair, linear_out and the hamiltonian namelist's v_beta patched.
A's files against the matching run's unprefixed ones, every number at 1e-6 relative or 1e-9 absolute -- the comparison of
tests/test_kubo_diag_dropin.py.  Cubic Pt makes several components vanish by symmetry; the two that must not -- charge under field y
(longitudinal) and spin under field x (the fixture's spin-Hall response) -- are shown to be there and to differ."""
import copy

import numpy as np
import pytest

from helpers import program_built
from test_conductivity_dropin import run_case
from test_fortran_dropin import DROPIN, MANIFEST
from test_kubo_diag_dropin import CASE, FILES, table
from test_kubo_multi_dropin import assert_tables_agree

pytestmark = pytest.mark.gpu
REGION = "kubo-tensor-gpu"
AXIS = {"x": "1, 0, 0", "y": "0, 1, 0"}
PREFIX = {("charge", "x"): "", ("spin", "x"): "spin_", ("charge", "y"): "Ey_", ("spin", "y"): "Ey_spin_"}


def test_drop_in_further_fields_match_their_own_runs(tmp_path, monkeypatch):
    if not program_built(DROPIN):               # (warns: the program holds reference object code, test_fortran_dropin.py)
        return
    for (op, axis) in PREFIX:
        case = copy.deepcopy(MANIFEST[CASE])
        case["patch"].setdefault("control", {})["linear_out"] = "'%s'" % op
        case["patch"].setdefault("hamiltonian", {})["v_beta"] = AXIS[axis]
        monkeypatch.setitem(MANIFEST, "%s_%s_%s" % (CASE, op, axis), case)
    monkeypatch.delenv("RSREC_KUBO_DIAG", raising=False)
    monkeypatch.setenv("RSREC_KUBO_FIELDS", "y")                       # (run_case hands the environment on to the program)
    monkeypatch.setenv("RSREC_KUBO_RESPONSES", "spin")
    _, log_a = run_case(DROPIN, CASE + "_charge_x", tmp_path / "a")
    monkeypatch.delenv("RSREC_KUBO_FIELDS")
    monkeypatch.delenv("RSREC_KUBO_RESPONSES")
    monkeypatch.setenv("RSREC_KUBO_DIAG", "1")
    assert REGION in log_a, log_a[-3000:]                              # the timer report names the route
    assert "conductivity-integrand-gpu-resident" in log_a, log_a[-3000:]
    names = None
    for (op, axis), prefix in PREFIX.items():
        work = tmp_path / ("%s_%s" % (op, axis))
        _, log = run_case(DROPIN, "%s_%s_%s" % (CASE, op, axis), work)
        assert REGION not in log
        assert not list(work.glob("E?_*"))                             # without the variables no field-prefixed file is written
        if names is None:
            names = FILES + sorted(p.name for p in work.glob("Pt_cond*.out"))
            assert len(names) > len(FILES)
        for fn in names:
            assert_tables_agree(table(tmp_path / "a" / (prefix + fn)), table(work / fn), prefix + fn)
    # not vacuous: the longitudinal charge response and the spin-Hall response are there, and they are not copies of each other
    long_y, hall_x = table(tmp_path / "a" / "Ey_fort.123")[:, 1:], table(tmp_path / "a" / "spin_fort.123")[:, 1:]
    assert np.abs(long_y).max(axis=0).max() > 1e-6 and np.abs(hall_x).max(axis=0).max() > 1e-6
    assert np.abs(long_y - hall_x).max() > 1e-6
