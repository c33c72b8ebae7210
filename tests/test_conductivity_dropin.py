"""The conductivity post-processing through both Fortran builds (tests/test_fortran_dropin.py has the machinery):
  * the zero-edit drop-in oracle/_ref/rslmto_dropin.x, whose type(conductivity) is fortran/conductivity_gpu.f90 -- gamma_nm is never
    allocated and the integrand comes from rsrec_kubo_integrand;
  * oracle/_ref/kubo_gpu.x, the reference's own host conductivity_mod on the same GPU moments.
Every line of fort.123 (energy, Re and Im of the integrand) must agree at 1e-6 relative or 1e-9 absolute.  The Simpson-integrated
cond_*.out files are left out: the reference's simpson_f reads past its arrays in both builds (the kubo_gpu.x paragraph)."""
import os
import re
import shutil

import numpy as np
import pytest

from helpers import program_built
from oracle.make_fixtures import patch_namelist
from rslmtoasa_amd._proc import run_with_unlimited_stack
from test_fortran_dropin import DROPIN, EXE, MANIFEST, SCF, fortran_float

pytestmark = pytest.mark.gpu
KUBO = os.path.join(os.path.dirname(EXE), "kubo_gpu.x")
CASES = ["Generated_conductivity_fccPt_spin", "Generated_conductivity_fccPt_spin_random_vec"]


def run_case(exe, name, work):
    case = MANIFEST[name]
    shutil.copytree(os.path.join(SCF, case["inputs"]), work)
    inp = work / "input.nml"
    inp.write_text(patch_namelist(inp.read_text(), case["patch"]))
    r = run_with_unlimited_stack([exe], cwd=work, env={"OMP_NUM_THREADS": "8", "RSREC_REPORT": "1"}, timeout=1500, scrub=False)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "fatal" not in log.lower(), log[-3000:]
    rows = [[fortran_float(t) for t in line.split()] for line in (work / "fort.123").read_text().splitlines() if line.strip()]
    return np.array(rows), log


@pytest.mark.parametrize("name", CASES)
def test_fort123_drop_in_matches_host_integrand(name, tmp_path):
    if not (program_built(DROPIN) and program_built(KUBO)):     # (warns: the programs hold reference object code, test_fortran_dropin.py)
        return
    gpu, log = run_case(DROPIN, name, tmp_path / "dropin")
    host, _ = run_case(KUBO, name, tmp_path / "host")
    assert "conductivity-integrand-gpu" in log, log[-3000:]           # the drop-in's integrand came from the device
    assert re.search(r"rsrec report: library_calls=(\d+)", log)
    assert gpu.shape == host.shape and gpu.shape[1] == 3 and gpu.shape[0] > 1000
    bad = ~((np.abs(gpu - host) <= 1e-6 * np.abs(host)) | (np.abs(gpu - host) <= 1e-9))
    assert not bad.any(), (np.argwhere(bad)[:5], gpu[bad][:5], host[bad][:5])
