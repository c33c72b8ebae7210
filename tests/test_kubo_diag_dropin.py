"""The orbital-diagonal Kubo route through the zero-edit drop-in (oracle/_ref/rslmto_dropin.x, tests/test_fortran_dropin.py has the
machinery): with RSREC_KUBO_DIAG=1 recursion_gpu%compute_moments_stochastic calls rsrec_kubo_moments_diag and stores only
mu_nm_stochastic(l, l, n, m, i) -- conductivity.f90:289, :292 read nothing else -- and conductivity_gpu takes the integrand from the
moments left on the device (rsrec_kubo_integrand_diag with a null pointer).  The conductivity_fccPt case, per_type (its vectors are
not drawn at random, so two runs have the same input): fort.123, cond_total.out, cond_total_orb_real.out, cond_total_orb_im.out and
Pt_cond*.out of the run with the switch against the same build's run without it, every number at 1e-6 relative or 1e-9 absolute --
the comparison of tests/test_conductivity_dropin.py."""
import re

import numpy as np
import pytest

from helpers import program_built
from test_conductivity_dropin import run_case
from test_fortran_dropin import DROPIN, fortran_float

pytestmark = pytest.mark.gpu
CASE = "Generated_conductivity_fccPt_spin"
FILES = ["fort.123", "cond_total.out", "cond_total_orb_real.out", "cond_total_orb_im.out"]


def table(path):
    return np.array([[fortran_float(t) for t in line.split()] for line in path.read_text().splitlines() if line.strip()])


def test_drop_in_with_diagonal_moments_matches_full_route(tmp_path, monkeypatch):
    if not program_built(DROPIN):               # (warns: the program holds reference object code, test_fortran_dropin.py)
        return
    monkeypatch.delenv("RSREC_KUBO_DIAG", raising=False)
    _, log_full = run_case(DROPIN, CASE, tmp_path / "full")
    monkeypatch.setenv("RSREC_KUBO_DIAG", "1")                         # (run_case hands the environment on to the program)
    _, log_diag = run_case(DROPIN, CASE, tmp_path / "diag")
    # the timer report names the route: the resident one only under the switch, today's region without it
    assert "conductivity-integrand-gpu-resident" in log_diag, log_diag[-3000:]
    assert "conductivity-integrand-gpu-resident" not in log_full, log_full[-3000:]
    assert re.search(r"conductivity-integrand-gpu(?!-)", log_full), log_full[-3000:]
    names = FILES + sorted(p.name for p in (tmp_path / "full").glob("Pt_cond*.out"))
    assert len(names) > len(FILES)
    for fn in names:
        full, diag = table(tmp_path / "full" / fn), table(tmp_path / "diag" / fn)
        assert full.shape == diag.shape and full.shape[0] > 1000 and np.isfinite(full).all(), fn
        bad = ~((np.abs(diag - full) <= 1e-6 * np.abs(full)) | (np.abs(diag - full) <= 1e-9))
        assert not bad.any(), (fn, np.argwhere(bad)[:5], diag[bad][:5], full[bad][:5])
