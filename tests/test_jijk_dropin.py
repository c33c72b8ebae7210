"""exchange_gpu's calculate_jijk through oracle/_ref/jijk_gpu.x (tests/fortran/jijk_gpu_driver.f90 on the object set of the zero-edit
drop-in): the reference's bcc Fe exchange input with one trio (tests/golden/jijk_dropin/inputs/bccFe: njijk = 1, the trio
(1, 2634, 2635) displaced along (1, 0.5, 0.25); block, lld 10, nsp 2) up to the pair recursion, then the routine.  Mode `gpu`: the
drop-in type, one rsrec_spin_lattice call on the resident chains.  Mode `plain`: the reference's own type(exchange) over the same
objects, with the host intersite stage."""
import os
import shutil

import numpy as np
import pytest

from helpers import program_built
from rslmtoasa_amd._proc import run_with_unlimited_stack
from test_fortran_dropin import ROOT, fortran_float

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "oracle", "_ref", "jijk_gpu.x")
INPUTS = os.path.join(ROOT, "tests", "golden", "jijk_dropin", "inputs", "bccFe")
TOL = 1e-12                      # kernel against restatement, relative to the trio's largest component (test_gpu_aux.py)
HALF_UNIT = 0.5e-9               # half a unit in the last digit of an F14.9 field


def run(mode, work):
    shutil.copytree(INPUTS, work, copy_function=shutil.copyfile)
    r = run_with_unlimited_stack([DRIVER], cwd=work, env={"OMP_NUM_THREADS": "8", "RSREC_REPORT": "1", "JIJK_DRIVER_MODE": mode}, timeout=1200,
                                 scrub=False)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "fatal" not in log.lower(), log[-3000:]
    return log


def jijk_values(log):
    """Per trio: (the atoms, the displacement line, the 9 components printed in 3F14.9)."""
    out, lines = [], log.splitlines()
    for k, line in enumerate(lines):
        if "Jijk tensor between trio" in line:
            atoms = [int(t.strip(",")) for t in line.split() if t.strip(",").isdigit()]
            assert "Displacement vector:" in lines[k + 1]
            out.append((atoms, lines[k + 1].strip(), [fortran_float(t) for l in lines[k + 2:k + 5] for t in l.split()]))
    return out


def test_jijk_matches_the_plain_type(tmp_path):
    if not program_built(DRIVER):
        return
    gpu = run("gpu", tmp_path / "gpu")
    plain = run("plain", tmp_path / "plain")
    assert "jijk-gpu" in gpu and "fetch-intersite" not in gpu, gpu[-3000:]          # the stage ran on the device, without the host arrays
    assert "host_intersite_allocated=F" in gpu, gpu[-3000:]
    assert "jijk-gpu" not in plain and "host_intersite_allocated=T" in plain, plain[-3000:]
    a, b = jijk_values(gpu), jijk_values(plain)
    print("gpu  ", a)
    print("plain", b)
    assert len(a) == len(b) == 1
    assert a[0][0] == b[0][0] == [1, 2634, 2635] and a[0][1] == b[0][1]
    va, vb = np.array(a[0][2]), np.array(b[0][2])
    assert va.shape == vb.shape == (9,)
    tol = HALF_UNIT + TOL * np.abs(vb).max()
    print("worst deviation %.2e (bound %.2e), largest component %.3e" % (np.abs(va - vb).max(), tol, np.abs(vb).max()))
    assert np.abs(va - vb).max() <= tol
    assert np.abs(vb).max() > 100 * HALF_UNIT               # the comparison sees digits
