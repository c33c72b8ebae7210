"""The conductivity files of the zero-edit drop-in (oracle/_ref/rslmto_dropin.x, tests/test_fortran_dropin.py has the machinery) now
that their Simpson integrals come from the device (rsrec_kubo_conductivity, region conductivity-tensor-gpu of the timer report):
cond_total.out, cond_total_orb_{real,im}.out and, with 'per_type', <symbol>_cond*.out.

The cases Generated_conductivity_fccPt_spin ('per_type') and ..._random_vec, one run each:
  * every number of those files is finite and below 1e50 in magnitude (the host tail's read past its arrays left 1e104 ... 1e133 there);
  * cond_total.out's columns 2-3 are the restatement (tests/cond_tensor_reference.py) of fort.123's columns 2-3, divided by loop_over,
    within 1e-6 (H / 3) sum_k c_k |y_k| / loop_over + 1e-6 |value|: both files print 7 significant digits, so every input carries at most
    5e-7 relative error and so does the printed output;
  * the 18 columns of cond_total_orb_real.out sum to cond_total.out's column 2 within 19 x 5e-7 x the row's largest magnitude (19
    printed numbers of 7 digits each); the same for _im and column 3;
  * the per-type files pass the same two checks without the division (the case has one type: its series are fort.123's).
A third run of the per_type case with RSREC_HOST_COND_TAIL=1 must take the host tail (region conductivity-tensor-host and no
conductivity-tensor-gpu); its values carry the stray read and are not compared."""
import re

import numpy as np
import pytest

import cond_tensor_reference as CT
from helpers import program_built
from test_conductivity_dropin import run_case
from test_fortran_dropin import DROPIN, fortran_float

pytestmark = pytest.mark.gpu
CASES = {"Generated_conductivity_fccPt_spin": "per_type", "Generated_conductivity_fccPt_spin_random_vec": "random_vec"}


def table(path):
    return np.array([[fortran_float(t) for t in line.split()] for line in path.read_text().splitlines() if line.strip()])


def namelist_value(text, key):
    m = re.search(r"(?im)^\s*%s\s*=\s*([^!\n,/]+)" % re.escape(key), text)
    assert m, key
    return m.group(1).strip().strip("'\"")


def scaled_mesh(work):
    """x = (energy%ene - b) / a and nv1 of the run, from its input.nml as energy%e_mesh (energy.f90:174-207) and
    calculate_conductivity_tensor (:238-252) form them; also energy%ene - fermi, fort.123's first column."""
    text = (work / "input.nml").read_text()
    emin, emax, fermi = (float(namelist_value(text, k)) for k in ("energy_min", "energy_max", "fermi"))
    ch = int(namelist_value(text, "channels_ldos"))
    nv1 = ch + 1 if ch % 2 == 0 else ch
    ch = ch if ch % 2 == 0 else ch - 1
    edel = (emax - emin) / ch
    edel = (fermi - emin) / round((fermi - emin) / edel)
    ene = emin + edel * np.arange(ch + 10)
    return CT.scaled_axis(ene, emin, emax), nv1, ene - fermi


def loop_over(work, calctype):
    text = (work / "input.nml").read_text()
    assert namelist_value(text, "cond_calctype") == calctype
    return int(namelist_value(text, "random_vec_num")) if calctype == "random_vec" else 1      # (one type: Pt)


def check_files(work, total, orb_real, orb_im, x, nv1, col1, divide):
    f123 = table(work / "fort.123")
    tot, orr, oim = table(work / total), table(work / orb_real), table(work / orb_im)
    nen = x.size
    assert f123.shape == (nen, 3) and tot.shape == (nen, 3) and orr.shape == (nen, 19) and oim.shape == (nen, 19)
    for t in (tot, orr, oim):
        assert np.isfinite(t).all() and np.abs(t).max() < 1e50, total
    assert np.abs(f123[:, 0] - col1).max() <= 1e-6 * np.abs(col1).max()              # the mesh of the run is the mesh restated here
    assert np.array_equal(tot[:, 0], f123[:, 0])
    y = f123[:, 1:3].T
    want = CT.simpson_limits(x, nv1, y, 0.0) / divide
    c = np.zeros(nen + 1)
    for I in range(2, nv1 + 10, 2):
        c[I - 2:I + 1] += (1.0, 4.0, 1.0)
    scale = (x[1] - x[0]) / 3.0 * (np.abs(y) * c[:nen]).sum(axis=1) / divide
    got = tot[:, 1:3].T
    bound = 1e-6 * scale[:, None] + 1e-6 * np.abs(want)
    err = np.abs(got - want)
    print(total, "max err / bound", (err / bound).max(), "max |value|", np.abs(want).max(axis=1))
    assert np.abs(want).max() > 0 and (err <= bound).all(), (total, np.argwhere(err > bound)[:5])
    for orb, col in ((orr, 1), (oim, 2)):
        rows = np.concatenate([orb[:, 1:], tot[:, col:col + 1]], axis=1)
        assert (np.abs(orb[:, 1:].sum(axis=1) - tot[:, col]) <= 19 * 5e-7 * np.abs(rows).max(axis=1)).all(), total


@pytest.mark.parametrize("name", sorted(CASES))
def test_drop_in_conductivity_files_come_from_the_device(name, tmp_path, monkeypatch):
    if not program_built(DROPIN):               # (warns: the program holds reference object code, test_fortran_dropin.py)
        return
    monkeypatch.delenv("RSREC_HOST_COND_TAIL", raising=False)
    work = tmp_path / "gpu"
    _, log = run_case(DROPIN, name, work)
    assert "conductivity-tensor-gpu" in log and "conductivity-tensor-host" not in log, log[-3000:]
    x, nv1, col1 = scaled_mesh(work)
    n = loop_over(work, CASES[name])
    check_files(work, "cond_total.out", "cond_total_orb_real.out", "cond_total_orb_im.out", x, nv1, col1, float(n))
    if CASES[name] == "per_type":
        assert sorted(p.name for p in work.glob("Pt_cond*.out")) == ["Pt_cond.out", "Pt_cond_orb_im.out", "Pt_cond_orb_real.out"]
        check_files(work, "Pt_cond.out", "Pt_cond_orb_real.out", "Pt_cond_orb_im.out", x, nv1, col1, 1.0)
    else:
        assert not list(work.glob("Pt_cond*.out"))


def test_host_tail_switch_takes_the_host_route(tmp_path, monkeypatch):
    if not program_built(DROPIN):
        return
    monkeypatch.setenv("RSREC_HOST_COND_TAIL", "1")                    # (run_case hands the environment on to the program)
    _, log = run_case(DROPIN, "Generated_conductivity_fccPt_spin", tmp_path / "host")
    assert "conductivity-tensor-host" in log and "conductivity-tensor-gpu" not in log, log[-3000:]
