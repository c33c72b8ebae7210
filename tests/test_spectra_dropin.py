"""The moment stage of an SCF iteration on the device in both Fortran builds (fortran/bands_gpu.f90: calculate_magnetic_moments,
calculate_orbital_moments and calculate_moments from ONE rsrec_block_spectra / rsrec_chebyshev_spectra call while g0 is pending), against
the manifest's expected values and against the same run with the inherited host routines over a downloaded g0 (RSREC_HOST_MOMENTS).

With RSREC_DEFER_G0 the device run never produces g0: its timer report has `spectra-gpu` and no Green region; the host run has the
Green region and no `spectra-gpu`.  The energy-resolved files and the log lines of the two runs agree to two units of the last printed
digit of each column's largest entry (es16.6: seven significant digits; f10.6: 1e-6).  Rows in which either run prints a magnitude above
1e100 are left out (at most the last tenth of a file): with nv1 = channels_ldos + 1 (energy.f90:184-188) the reference's simpson_f
reads Y(nv1 + 10), one element past its arrays, and the rows whose Fermi function reaches that point show whatever lies behind the
array (1e219 in the runs recorded here) -- not a function of the input.  The integrands are of order 1 to 100 on a mesh 5 Ry wide, so a
genuine entry is below 1e3.  The device route pads its integrands with a zero there, so its own rows are clean.

Like its neighbours the test needs the programs build() links where the reference sources are readable; a tree without them returns
early."""
import math
import os
import re
import shutil

import pytest

from helpers import program_built
from oracle.make_fixtures import patch_namelist
from rslmtoasa_amd._proc import run_with_unlimited_stack
from test_cheb_ldos_dropin import expected_misses
from test_fortran_dropin import DROPIN, EXE, MANIFEST, SCF, fortran_float

pytestmark = pytest.mark.gpu

CASES = ["Example_bulk_bccFe_nsp4_block", "Example_bulk_bccFe_nsp2_chebyshev"]
GREEN_REGIONS = ("bgreen-gpu", "chebyshev-green-gpu")
MOMENT_LINE = re.compile(r"(Spin|Orbital) moment of atom\s+(\d+) is((?:\s+-?\d+\.\d+)+)")


def run_case(exe, case, work, env):
    shutil.copytree(os.path.join(SCF, case["inputs"]), work)
    inp = work / "input.nml"
    inp.write_text(patch_namelist(inp.read_text(), case["patch"]))
    # every child drives the GPU itself under its own time limit, one at a time; a failing run ends the test (the asserts below)
    r = run_with_unlimited_stack([exe], cwd=work, env=dict(env, OMP_NUM_THREADS="8", RSREC_REPORT="1"), timeout=900, scrub=False)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "fatal" not in log.lower(), log[-3000:]
    return log


def columns(work, suffix):
    out = {}
    for fn in sorted(os.listdir(work)):
        if fn.endswith(suffix):
            rows = [[fortran_float(v) for v in line.split()] for line in (work / fn).read_text().splitlines()]
            out[fn] = rows
    return out


def es_unit(col):
    """One unit of the seventh significant digit (es16.6) of the column's largest entry."""
    big = max(abs(v) for v in col)
    return 10.0 ** (math.floor(math.log10(big)) - 6) if big > 0 else 0.0


def moment_lines(log):
    """(kind, atom) -> the LAST such line of the run (the converged iteration)."""
    return {(m.group(1), int(m.group(2))): tuple(float(v) for v in m.group(3).split()) for m in MOMENT_LINE.finditer(log)}


def compare_runs(dev_work, dev_log, host_work, host_log):
    for suffix in ("_spinene.out", "_orbene.out"):
        a, b = columns(dev_work, suffix), columns(host_work, suffix)
        assert set(a) == set(b) and a, suffix
        for fn in a:
            assert len(a[fn]) == len(b[fn]) > 1000 and all(len(r) == 4 for r in a[fn] + b[fn]), fn
            keep = [k for k, (ra, rb) in enumerate(zip(a[fn], b[fn])) if max(abs(v) for v in ra + rb) < 1e100]   # (module docstring)
            assert len(keep) >= 0.9 * len(a[fn]), (fn, len(keep))
            for c, (ca, cb) in enumerate(zip(zip(*[a[fn][k] for k in keep]), zip(*[b[fn][k] for k in keep]))):
                worst, unit = max(abs(x - y) for x, y in zip(ca, cb)), es_unit(cb)
                print("%s column %d: device vs host, worst printed difference %.3e (unit %.1e)" % (fn, c + 1, worst, unit))
                assert worst <= 2.0 * unit * (1 + 1e-9), (fn, c, worst, unit)
    ma, mb = moment_lines(dev_log), moment_lines(host_log)
    assert set(ma) == set(mb) and any(k[0] == "Spin" for k in ma) and any(k[0] == "Orbital" for k in ma)
    for k in ma:
        assert len(ma[k]) == len(mb[k]) == (1 if k[0] == "Spin" else 3), (k, ma[k], mb[k])
        worst = max(abs(x - y) for x, y in zip(ma[k], mb[k]))
        print("%s moment of atom %d: device %r host %r" % (k + (ma[k], mb[k])))
        assert worst <= 2.0e-6 * (1 + 1e-9), (k, ma[k], mb[k])


@pytest.mark.parametrize("name", CASES)
def test_scf_moments_from_device_spectra(name, tmp_path):
    if not program_built(EXE):
        return
    case = MANIFEST[name]
    dev_log = run_case(EXE, case, tmp_path / "device", {"RSREC_DEFER_G0": "1"})
    assert "spectra-gpu" in dev_log, dev_log[-3000:]
    assert not any(r in dev_log for r in GREEN_REGIONS), dev_log[-3000:]
    bad = expected_misses(case, tmp_path / "device")
    assert not bad, bad
    host_log = run_case(EXE, case, tmp_path / "host", {"RSREC_DEFER_G0": "1", "RSREC_HOST_MOMENTS": "1"})
    assert any(r in host_log for r in GREEN_REGIONS) and "spectra-gpu" not in host_log, host_log[-3000:]
    bad = expected_misses(case, tmp_path / "host")
    assert not bad, bad
    compare_runs(tmp_path / "device", dev_log, tmp_path / "host", host_log)


def test_zero_edit_dropin_takes_the_device_route(tmp_path):
    """The reference's own main program over the shadow modules: RSREC_DEFER_G0 alone puts its SCF loop on the device route."""
    if not program_built(DROPIN):
        return
    case = MANIFEST[CASES[0]]
    log = run_case(DROPIN, case, tmp_path / "dropin", {"RSREC_DEFER_G0": "1"})
    # (the reference's main program goes on to calculate_orbital_quadrupoles after the SCF loop, which fetches g0 once: a Green region
    # outside `calculation-of-DOS` is expected here)
    assert "spectra-gpu" in log, log[-3000:]
    bad = expected_misses(case, tmp_path / "dropin")
    assert not bad, bad
