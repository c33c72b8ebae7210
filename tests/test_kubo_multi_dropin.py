"""Several responses to one applied field through the zero-edit drop-in (oracle/_ref/rslmto_dropin.x, tests/test_fortran_dropin.py
has the machinery): with RSREC_KUBO_RESPONSES=charge recursion_gpu%compute_moments_stochastic forms the diagonal moments of the
namelist's linear_out ('spin') and of the charge response in one rsrec_kubo_moments_diag_multi call, and conductivity_gpu writes the
charge response's files with the prefix charge_ beside the namelist response's own.  The conductivity_fccPt case, per_type (its
vectors are not drawn at random, so runs have the same input), three runs:
  A  RSREC_KUBO_RESPONSES=charge;
  B  the case patched to linear_out = 'charge', RSREC_KUBO_DIAG=1;
  C  the case as it is, RSREC_KUBO_DIAG=1.
A's charge_* files against B's unprefixed ones and A's unprefixed files against C's, every number at 1e-6 relative or 1e-9 absolute --
the comparison of tests/test_kubo_diag_dropin.py."""
import copy

import numpy as np
import pytest

from helpers import program_built
from test_conductivity_dropin import run_case
from test_fortran_dropin import DROPIN, MANIFEST
from test_kubo_diag_dropin import CASE, FILES, table

pytestmark = pytest.mark.gpu
REGION = "kubo-multi-gpu"


def assert_tables_agree(mine, ref, what):
    assert mine.shape == ref.shape and ref.shape[0] > 1000 and np.isfinite(ref).all(), what
    bad = ~((np.abs(mine - ref) <= 1e-6 * np.abs(ref)) | (np.abs(mine - ref) <= 1e-9))
    assert not bad.any(), (what, np.argwhere(bad)[:5], mine[bad][:5], ref[bad][:5])


def test_drop_in_further_response_matches_its_own_run(tmp_path, monkeypatch):
    if not program_built(DROPIN):               # (warns: the program holds reference object code, test_fortran_dropin.py)
        return
    charge_case = copy.deepcopy(MANIFEST[CASE])
    charge_case["patch"].setdefault("control", {})["linear_out"] = "'charge'"
    monkeypatch.setitem(MANIFEST, CASE + "_charge_out", charge_case)
    monkeypatch.delenv("RSREC_KUBO_DIAG", raising=False)
    monkeypatch.setenv("RSREC_KUBO_RESPONSES", "charge")               # (run_case hands the environment on to the program)
    _, log_a = run_case(DROPIN, CASE, tmp_path / "a")
    monkeypatch.delenv("RSREC_KUBO_RESPONSES")
    monkeypatch.setenv("RSREC_KUBO_DIAG", "1")
    _, log_b = run_case(DROPIN, CASE + "_charge_out", tmp_path / "b")
    _, log_c = run_case(DROPIN, CASE, tmp_path / "c")
    # the timer report names the route
    assert REGION in log_a, log_a[-3000:]
    assert REGION not in log_b and REGION not in log_c
    assert "conductivity-integrand-gpu-resident" in log_a, log_a[-3000:]
    names = FILES + sorted(p.name for p in (tmp_path / "c").glob("Pt_cond*.out"))
    assert len(names) > len(FILES)
    for fn in names:
        assert_tables_agree(table(tmp_path / "a" / ("charge_" + fn)), table(tmp_path / "b" / fn), "charge_" + fn)
        assert_tables_agree(table(tmp_path / "a" / fn), table(tmp_path / "c" / fn), fn)
    # the two responses differ: the prefixed files are not copies of the namelist response's
    assert np.abs(table(tmp_path / "a" / "charge_fort.123")[:, 1:] - table(tmp_path / "a" / "fort.123")[:, 1:]).max() > 1e-6
    assert not list((tmp_path / "b").glob("charge_*")) and not list((tmp_path / "c").glob("charge_*"))
