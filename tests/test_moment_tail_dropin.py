"""The integrals behind the SCF spectra in both Fortran builds (fortran/bands_gpu.f90: `device_tail`): the Simpson tails of
calculate_magnetic_moments, calculate_orbital_moments and calculate_moments from ONE rsrec_spectra_integrals call per spectra image,
against the same run with the reference's host loops kept (RSREC_HOST_MOMENT_TAIL); and calculate_orbital_quadrupoles of the zero-edit
drop-in without a g0, against the same run with the inherited routines over a downloaded g0 (RSREC_HOST_MOMENTS).

The case runs the single SCF step its manifest entry sets (self%nstep = 1, the fewest the namelist allows): two routes are compared, not
a converged result.  The timer report shows the route: `moment-integrals-gpu` in one run, `moment-integrals-host` in the other, never both.
Files and log lines agree to two units of the last printed digit, rows above 1e100 left out (at most the last tenth of a file): the
rules, and the reason, of tests/test_spectra_dropin.py.

Like its neighbours the test needs the programs build() links where the reference sources are readable; a tree without them returns
early."""
import re

import pytest

from helpers import program_built
from test_fortran_dropin import DROPIN, EXE, MANIFEST
from test_spectra_dropin import GREEN_REGIONS, columns, compare_runs, es_unit, run_case

pytestmark = pytest.mark.gpu

CASE = "Example_bulk_bccFe_nsp4_block"
QUAD_LINE = re.compile(r"(Orbital quadrupoles|Traceless orbital quadrupoles) of atom\s+(\d+) [A-Za-z0-9 ]+=((?:\s+-?\d+\.\d+)+)")


def report_paths(log):
    """The rows of g_timer's report as paths: the report prints a tree, a row's depth is where its label starts."""
    head = re.search(r"(?m)^\s*CATEGORY\s+MEAN\s+MAX\s+MIN\s+TOTAL\s.*$", log)
    assert head, log[-3000:]
    stack, paths = [], []
    for line in log[head.end():].splitlines():
        m = re.match(r"^([^\w]*)([\w][\w-]*)\*?\s+\S+(\s+\S+){6}\s*$", line)
        if not m:
            continue
        depth = len(m.group(1))
        while stack and stack[-1][0] >= depth:
            stack.pop()
        stack.append((depth, m.group(2)))
        paths.append(tuple(label for _, label in stack))
    assert paths, log[-3000:]
    return paths


def case():
    c = MANIFEST[CASE]
    assert c["patch"]["self"]["nstep"] == "1"
    return c


def test_device_tail_against_host_tail(tmp_path):
    if not program_built(EXE):
        return
    dev_log = run_case(EXE, case(), tmp_path / "device", {"RSREC_DEFER_G0": "1"})
    assert "moment-integrals-gpu" in dev_log and "moment-integrals-host" not in dev_log, dev_log[-3000:]
    assert "spectra-gpu" in dev_log and not any(r in dev_log for r in GREEN_REGIONS), dev_log[-3000:]
    host_log = run_case(EXE, case(), tmp_path / "host", {"RSREC_DEFER_G0": "1", "RSREC_HOST_MOMENT_TAIL": "1"})
    assert "moment-integrals-host" in host_log and "moment-integrals-gpu" not in host_log, host_log[-3000:]
    assert "spectra-gpu" in host_log and not any(r in host_log for r in GREEN_REGIONS), host_log[-3000:]
    compare_runs(tmp_path / "device", dev_log, tmp_path / "host", host_log)


def quad_lines(log):
    return {(m.group(1), int(m.group(2))): tuple(float(v) for v in m.group(3).split()) for m in QUAD_LINE.finditer(log)}


@pytest.fixture(scope="module")
def dropin_runs(tmp_path_factory):
    """The zero-edit drop-in on the device route and with RSREC_HOST_MOMENTS, once for the tests below; None where it is not built."""
    if not program_built(DROPIN):
        return None
    work = tmp_path_factory.mktemp("dropin")
    dev_log = run_case(DROPIN, case(), work / "device", {"RSREC_DEFER_G0": "1"})
    host_log = run_case(DROPIN, case(), work / "host", {"RSREC_DEFER_G0": "1", "RSREC_HOST_MOMENTS": "1"})
    return work / "device", dev_log, work / "host", host_log


def quad_columns(dev_work, host_work):
    """<sym>_orbquadene.out of the two runs.  Columns 1-7 (the energy and the six integrals) by the rule of the module docstring, two units
    u_c of the last printed digit of the column's largest entry.  Columns 8 and 9 are not integrals but combinations of columns 2-4, formed
    from the unrounded values: -((qxx - qyy)/pi) and -((2 qzz - qxx - qyy)/pi).  Two runs whose integrals agree to 2 u_c each can differ
    there by the same combination of those bounds, 2 (u_2 + u_3) and 2 (2 u_4 + u_2 + u_3), whatever the size of the combination itself --
    in a cubic cell qxx = qyy, column 8 is the rounding error of its operands and its own largest entry says nothing about its accuracy.
    Their bound is the larger of that and the column's own 2 u_c (the printing of the combination rounds once more)."""
    a, b = columns(dev_work, "_orbquadene.out"), columns(host_work, "_orbquadene.out")
    assert set(a) == set(b) and a
    for fn in a:
        assert len(a[fn]) == len(b[fn]) > 1000 and all(len(r) == 9 for r in a[fn] + b[fn]), fn
        keep = [k for k, (ra, rb) in enumerate(zip(a[fn], b[fn])) if max(abs(v) for v in ra + rb) < 1e100]
        assert len(keep) >= 0.9 * len(a[fn]), (fn, len(keep))
        cols = list(zip(zip(*[a[fn][k] for k in keep]), zip(*[b[fn][k] for k in keep])))
        unit = [es_unit(cb) for _, cb in cols]
        bound = [2.0 * u for u in unit]
        bound[7] = max(bound[7], 2.0 * (unit[1] + unit[2]))
        bound[8] = max(bound[8], 2.0 * (2.0 * unit[3] + unit[1] + unit[2]))
        worst = [max(abs(x - y) for x, y in zip(ca, cb)) for ca, cb in cols]
        for c in range(9):
            print("%s column %d: device vs host, worst printed difference %.3e (own unit %.1e, bound %.1e)" % (fn, c + 1, worst[c], unit[c], bound[c]))
        for c in range(9):
            assert worst[c] <= bound[c] * (1 + 1e-9), (fn, c, worst[c], bound[c])


def test_zero_edit_dropin_forms_no_g0_after_the_scf_loop(dropin_runs):
    """The reference's own main program calls calculate_orbital_quadrupoles after the SCF loop (calculation.f90:621); on the device route it
    no longer fetches g0: no Green region outside `calculation-of-DOS`; <sym>_orbquadene.out (quad_columns) and the two log lines of a
    host-moments run.  (The spin and orbital files of the two tails are compared in test_device_tail_against_host_tail; their comparison
    with a host-moments run is tests/test_spectra_dropin.py's.)"""
    if dropin_runs is None:
        return
    dev_work, dev_log, host_work, host_log = dropin_runs
    assert "moment-integrals-gpu" in dev_log and "moment-integrals-host" not in dev_log, dev_log[-3000:]
    stray = [p for p in report_paths(dev_log) if p[-1] in GREEN_REGIONS and "calculation-of-DOS" not in p]
    assert not stray, stray
    assert any(p[-1] in GREEN_REGIONS for p in report_paths(host_log)) and "moment-integrals-gpu" not in host_log, host_log[-3000:]
    quad_columns(dev_work, host_work)
    qa, qb = quad_lines(dev_log), quad_lines(host_log)
    assert set(qa) == set(qb) and len(qa) >= 2
    for k in qa:
        assert len(qa[k]) == len(qb[k]) == (6 if k[0].startswith("Orbital") else 2), (k, qa[k], qb[k])
        print("%s of atom %d: device %r host %r" % (k + (qa[k], qb[k])))
        assert max(abs(x - y) for x, y in zip(qa[k], qb[k])) <= 2.0e-6 * (1 + 1e-9), (k, qa[k], qb[k])
