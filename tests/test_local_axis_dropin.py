"""Local-axis SCF runs of the zero-edit program on the device stages (RSREC_LOCAL_AXIS_DEVICE, fortran/recursion_gpu.f90).

rsrec_block_lanczos_local_axis leaves the chains resident in each site's local frame; with the switch set `recursion_gpu` announces them
and `bands_gpu` takes its device routes as in a collinear run:
  run A  RSREC_LOCAL_AXIS_DEVICE=1                    the densities of states of calculate_fermi from rsrec_block_ldos (`ldos-gpu`)
  run B  RSREC_LOCAL_AXIS_DEVICE=1 RSREC_DEFER_G0=1   also the moment stage from one rsrec_block_spectra call (`spectra-gpu`), with the
                                                      local-axis tails of bands.f90:849-853 and :427-432, :458-467 restated
Both meet the manifest's expected values at the case's tolerances, and their `Local / Global spin moment projections` lines agree with
a run without the switch (the inherited host routines) to two units of the printed f10.6, the bound tests/test_spectra_dropin.py uses
for moment lines.  Without the switch a local-axis run shows no `ldos-gpu` region (tests/test_fortran_dropin.py).

Like its neighbours the test needs the program build() links where the reference sources are readable; a tree without it returns
early."""
import re

import pytest

from helpers import program_built
from test_cheb_ldos_dropin import expected_misses
from test_fortran_dropin import DROPIN, MANIFEST
from test_spectra_dropin import run_case

pytestmark = pytest.mark.gpu

CASES = ["Generated_bulk_bccFe_nsp4_local_axis", "Generated_bulk_Pt2MnGa_nsp4_local_axis"]
PROJECTION_LINE = re.compile(r"(Local|Global) spin moment projections of atom\s+(\d+) is((?:\s+-?\d+\.\d+)+)")


def projection_lines(log):
    """(frame, atom) -> the LAST such line of the run (the last iteration)."""
    return {(m.group(1), int(m.group(2))): tuple(float(v) for v in m.group(3).split()) for m in PROJECTION_LINE.finditer(log)}


@pytest.mark.parametrize("name", CASES)
def test_local_axis_scf_on_the_device_stages(name, tmp_path):
    if not program_built(DROPIN):
        return
    case = MANIFEST[name]
    assert "local_axis" in str(case["patch"])
    host_log = run_case(DROPIN, case, tmp_path / "host", {})
    assert "ldos-gpu" not in host_log and "spectra-gpu" not in host_log, host_log[-3000:]
    ref = projection_lines(host_log)
    assert any(k[0] == "Local" for k in ref) and any(k[0] == "Global" for k in ref), host_log[-3000:]
    runs = (("A", {"RSREC_LOCAL_AXIS_DEVICE": "1"}, "ldos-gpu"),
            ("B", {"RSREC_LOCAL_AXIS_DEVICE": "1", "RSREC_DEFER_G0": "1"}, "spectra-gpu"))
    for tag, env, region in runs:
        log = run_case(DROPIN, case, tmp_path / tag, env)
        assert "ldos-gpu" in log and region in log, log[-3000:]
        bad = expected_misses(case, tmp_path / tag)
        assert not bad, (tag, bad)
        got = projection_lines(log)
        assert set(got) == set(ref), (tag, sorted(got), sorted(ref))
        for k in sorted(ref):
            assert len(got[k]) == len(ref[k]) == 3, (tag, k, got[k], ref[k])
            worst = max(abs(x - y) for x, y in zip(got[k], ref[k]))
            print("run %s, %s projections of atom %d: %r, without the switch %r" % ((tag,) + k + (got[k], ref[k])))
            assert worst <= 2.0e-6 * (1 + 1e-9), (tag, k, got[k], ref[k])
