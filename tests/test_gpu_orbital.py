"""chebyshev_orbital_mod (recursion.f90:2834-3049) as a device-resident loop: rsrec_orbital_moments, its Python / Fortran callers.

What the compiled reference leaves behind for this routine (tests/golden/fccPt_orbital[_hoh].npz, oracle/make_fixtures.py
run_orbital_case): per seed atom the full-precision sums of left_vec, left_vec1 and left_vec2 it prints (:2972), and unit 50 with the
trace of the resulting Green function -- which for this non-magnetic case is rounding noise (1e-13).  The moments themselves are a
local variable.  So: the CPU oracle is pinned on the printed sums (tests/test_oracle_golden.py), the GPU is held to the oracle's
moments at 1e-10 per seed and in sum, and the reference's unit-50 file is reproduced end to end through the Fortran override.
Parity of the moments against the reference itself is therefore pinned only through the left vectors: stated, not hidden."""
import os
import shutil

import numpy as np
import pytest

from helpers import RTOL, load_golden, orbital_unit50_energy_resolved, program_built
from oracle.make_fixtures import ORBITAL_CASES, patch_namelist
from rslmtoasa_amd._proc import run_with_unlimited_stack
from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["fccPt_orbital", "fccPt_orbital_hoh", "bccFe_orbital"]      # the last: ferromagnetic bcc Fe with spin-orbit coupling (round 4), a non-zero orbital moment


def make_rec(z, lld):
    ham = Hamiltonian(ee=z["ee"], lsham=z["lsham"], eeo=z.get("eeo"), enim=z.get("enim"), hoh=bool(z["hoh"]))
    lat = Lattice(nn=z["nn"], iz=z["iz"], irec=np.array([1], np.int32), nmax=0, ntype=z["ee"].shape[3])
    return Recursion(ham, lat, Control(lld=lld, nsp=int(z["nsp"])), Energy(), device=0)


@pytest.mark.parametrize("name", CASES)
def test_orbital_moments_match_oracle(name, oracle_lib):
    z = load_golden(name)
    kk, lld = int(z["kk"]), int(z["lld"])
    a, b = float(z["acheb"]), float(z["bcheb"])
    p = {k: z[k] for k in ("nn", "iz", "ee", "lsham", "eeo", "enim") if k in z}
    p.update(nmax=0, hoh=int(z["hoh"]), nsp=int(z["nsp"]))
    seeds = np.arange(1, kk + 1, dtype=np.int32)
    mu_o, ms_o, _ = oracle_lib.Oracle(p).orbital_moments(seeds, lld, a, b, z["cr"], float(z["alat"]), per_seed=True)
    rec = make_rec(z, lld)
    import rslmtoasa_amd.recursion as R
    orig = R.chebyshev_scaling
    R.chebyshev_scaling = lambda emin, emax: (a, b)
    try:
        mu, ms = rec.chebyshev_orbital_mod(z["cr"], float(z["alat"]), per_seed=True)
        sub = np.array([7, 3, 100], np.int32)
        mu_sub = rec.chebyshev_orbital_mod(z["cr"], float(z["alat"]), seeds=sub)
    finally:
        R.chebyshev_scaling = orig
    rec.close()
    scale = np.abs(ms_o).max(axis=(0, 1))                            # per (level, seed); some are exact zeros (a seed at the origin: X|r> = Y|r> = 0)
    err = np.abs(ms - ms_o).max(axis=(0, 1))
    assert np.all(err <= RTOL * np.maximum(scale, 1e-3 * scale.max())), float((err / np.maximum(scale, 1e-3 * scale.max())).max())
    assert np.abs(mu * kk - mu_o).max() <= RTOL * np.abs(ms_o).max()         # the sum over all seeds (cancels to ~0 in parts: absolute bar)
    assert np.abs(mu_sub - ms_o[:, :, :, sub - 1].sum(axis=3)).max() <= RTOL * np.abs(ms_o).max()
    if name == "bccFe_orbital":
        # magnetic case: the GPU's own moments against the REFERENCE's unit-50 file (energy-resolved column: a linear map of Re tr(mu_n),
        # 7 printed digits) -- the moments themselves are pinned here, not only the left vectors
        f50 = z["fort50"]
        col3 = orbital_unit50_energy_resolved(mu * kk, kk, a, b, z["ene"])
        assert np.abs(f50[:, 2]).max() > 1e-4
        assert np.all(np.abs(col3 - f50[:, 2]) <= 5.1e-7 * np.abs(f50[:, 2]) + 1e-9 * np.abs(f50[:, 2]).max()), float(np.abs(col3 - f50[:, 2]).max())


def gpu_unit50_column3(name):
    """Column 3 of unit 50 (the energy-resolved orbital moment, recursion.f90:3007-3046) from the GPU's moments over all seed atoms of
    the stored fixture, on the reference's energy mesh."""
    z = load_golden(name)
    kk, lld = int(z["kk"]), int(z["lld"])
    a, b = float(z["acheb"]), float(z["bcheb"])
    rec = make_rec(z, lld)
    import rslmtoasa_amd.recursion as R
    orig, R.chebyshev_scaling = R.chebyshev_scaling, lambda emin, emax: (a, b)
    try:
        mu = rec.chebyshev_orbital_mod(z["cr"], float(z["alat"]))
    finally:
        R.chebyshev_scaling = orig
        rec.close()
    return z, orbital_unit50_energy_resolved(mu * kk, kk, a, b, z["ene"])


def test_fortran_override_reproduces_the_reference_file(tmp_path):
    """kubo_gpu.x (the reference's modules + type(recursion_gpu)) in the orbital-moment workflow: unit 50 against the compiled
    reference's file.  Column 1 (E - E_F) to its printed digits; the trace columns are rounding noise in both."""
    # without reference code: the device moments of the stored fixture give a trace column at rounding-noise level, as the
    # reference's file has it (a non-magnetic case)
    z, col3 = gpu_unit50_column3("fccPt_orbital")
    assert col3.shape == z["fort50"][:, 2].shape and np.abs(z["fort50"][:, 2]).max() < 1e-9 and np.abs(col3).max() < 1e-9
    exe = os.path.join(ROOT, "oracle", "_ref", "kubo_gpu.x")
    if not program_built(exe):
        return
    work = tmp_path / "run"
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "scf", "inputs", "conductivity_fccPt"), work)
    inp = work / "input.nml"
    inp.write_text(patch_namelist(inp.read_text(), ORBITAL_CASES["fccPt_orbital"][1]))
    r = run_with_unlimited_stack([exe], cwd=work, env={"OMP_NUM_THREADS": "8", "RSREC_ORBITAL": "1"}, timeout=900, scrub=False)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "fatal" not in log.lower() and "chebyshev-orbital-gpu" in log, log[-3000:]
    rows = np.array([[float(v) for v in l.split()] for l in (work / "fort.50").read_text().splitlines() if l.strip()])
    ref = z["fort50"]
    assert rows.shape == ref.shape
    assert np.abs(rows[:, 0] - ref[:, 0]).max() <= 1e-6 * np.abs(ref[:, 0]).max()
    assert np.abs(ref[:, 2]).max() < 1e-9 and np.abs(rows[:, 2]).max() < 1e-9


def test_zero_edit_program_reproduces_the_reference_file_on_a_magnetic_case(tmp_path):
    """The reference's OWN main program (rslmto_dropin.x: unmodified sources, GPU types behind the module names) with
    post_processing = 'orbital_modern' (calculation.f90:208, :1158-1269) on ferromagnetic bcc Fe with spin-orbit coupling: unit 50 --
    E - E_F, the integrated and the energy-resolved orbital moment -- against the compiled reference's file of the same run
    (tests/golden/bccFe_orbital.npz), all three columns to the printed digits.  recursion%chebyshev_orbital_mod is the device-resident
    loop (rsrec_orbital_moments) behind `type(recursion)`."""
    # without reference code: the energy-resolved column from the device moments of the stored fixture, at the bar of
    # test_orbital_moments_match_oracle
    z, col3 = gpu_unit50_column3("bccFe_orbital")
    f50 = z["fort50"]
    assert np.all(np.abs(col3 - f50[:, 2]) <= 5.1e-7 * np.abs(f50[:, 2]) + 1e-9 * np.abs(f50[:, 2]).max()), float(np.abs(col3 - f50[:, 2]).max())
    exe = os.path.join(ROOT, "oracle", "_ref", "rslmto_dropin.x")
    if not program_built(exe):
        return
    work = tmp_path / "run"
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "scf", "inputs", "bulk_bccFe"), work)
    inp = work / "input.nml"
    # (pre_processing = 'none': the fixture's run -- oracle/dump_kubo.f90 -- goes straight to the post-processing branch; the case file's
    # 'bravais' would run an SCF iteration first and move the Fermi level the output is referred to)
    patch = dict(ORBITAL_CASES["bccFe_orbital"][1], calculation={"pre_processing": "'none'", "post_processing": "'orbital_modern'"})
    inp.write_text(patch_namelist(inp.read_text(), patch))
    r = run_with_unlimited_stack([exe], cwd=work, env={"OMP_NUM_THREADS": "8", "RSREC_REPORT": "1"}, timeout=900, scrub=False)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "fatal" not in log.lower() and "chebyshev-orbital-gpu" in log and "rsrec report: library_calls=" in log, log[-3000:]
    rows = np.array([[float(v) for v in l.split()] for l in (work / "fort.50").read_text().splitlines() if l.strip()])
    ref = z["fort50"]
    assert rows.shape == ref.shape and np.abs(ref[:, 2]).max() > 1e-4
    for col in range(3):
        # 7 printed digits; a last-digit flip of either file is one unit of its 7th digit
        assert np.all(np.abs(rows[:, col] - ref[:, col]) <= 2.1e-6 * np.abs(ref[:, col]) + 1e-9 * np.abs(ref[:, col]).max()), (col, float(np.abs(rows[:, col] - ref[:, col]).max()))
