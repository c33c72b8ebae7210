"""The Chebyshev SCF case of the manifest through both Fortran builds with the LDOS stage of `bands%calculate_fermi` on the device
(fortran/bands_gpu.f90 -> rsrec_chebyshev_ldos on the moments chebyshev_recur left there), against the case's expected values and
against the same run with the inherited host reduction over a downloaded g0 (RSREC_HOST_LDOS).

Like its neighbours (test_fortran_dropin.py) the test needs the programs build() links where the reference sources are readable; a
tree without them returns early."""
import os
import shutil

import pytest

from helpers import program_built
from oracle.make_fixtures import patch_namelist
from rslmtoasa_amd._proc import run_with_unlimited_stack
from test_fortran_dropin import DROPIN, EXE, MANIFEST, SCF, close, fortran_float, read_nml_value

pytestmark = pytest.mark.gpu

CASE = "Example_bulk_bccFe_nsp2_chebyshev"


def expected_misses(case, work):
    """The case's expected values (manifest) against the files of a run, by the reference's own rule (tests/run_test.py:201-219)."""
    at, rt = case["abs_tol"], case["rel_tol"]
    bad = []
    for fn, keys in case["expected"].get("nml", {}).items():
        for key, exp in keys.items():
            for idx, e in (exp.items() if isinstance(exp, dict) else [(None, exp)]):
                got = read_nml_value(work / fn, key, None if idx is None else int(idx))
                if not close(got, e, at, rt):
                    bad.append((fn, key, idx, got, e))
    for fn, rows in case["expected"].get("text", {}).items():
        lines = (work / fn).read_text().splitlines()
        for row, cols in rows.items():
            vals = lines[int(row) - 1].split()
            for col, e in cols.items():
                got = fortran_float(vals[int(col) - 1])
                if not close(got, e, at, rt):
                    bad.append((fn, row, col, got, e))
    return bad


def dos_files(work):
    return {fn: [[fortran_float(v) for v in line.split()] for line in (work / fn).read_text().splitlines()]
            for fn in sorted(os.listdir(work)) if fn == "totaldos.out" or fn.endswith("_dos.out")}


@pytest.mark.parametrize("build", ["dropin", "driver"])
def test_chebyshev_scf_with_device_ldos(build, tmp_path):
    exe = DROPIN if build == "dropin" else EXE
    if not program_built(exe):
        return
    case = MANIFEST[CASE]
    assert "'chebyshev'" in str(case["patch"])
    outs = {}
    for mode, env in (("device", {}), ("host", {"RSREC_HOST_LDOS": "1"})):
        work = tmp_path / mode
        shutil.copytree(os.path.join(SCF, case["inputs"]), work)
        inp = work / "input.nml"
        inp.write_text(patch_namelist(inp.read_text(), case["patch"]))
        # every child drives the GPU itself under its own time limit; a failing run ends the test (the asserts below)
        r = run_with_unlimited_stack([exe], cwd=work, env=dict(env, OMP_NUM_THREADS="8", RSREC_REPORT="1"), timeout=900, scrub=False)
        log = r.stdout + r.stderr
        assert r.returncode == 0, (mode, log[-3000:])
        assert "fatal" not in log.lower(), (mode, log[-3000:])
        # an SCF iteration still fetches g0 for its moment integrals: the Green stage runs in both modes
        assert "chebyshev-green-gpu" in log, (mode, log[-3000:])
        assert ("ldos-gpu" in log) == (mode == "device"), (mode, log[-3000:])
        assert ("device_ldos_calls=0" in log) == (mode == "host"), (mode, log[-1500:])
        bad = expected_misses(case, work)
        assert not bad, (mode, bad)
        outs[mode] = dos_files(work)
    assert set(outs["device"]) == set(outs["host"]) and len(outs["device"]) >= 3          # totaldos, <sym>_dos, <sym>_orbital_dos
    for fn, rows in outs["device"].items():
        ref = outs["host"][fn]
        assert len(rows) == len(ref) > 1000, fn
        worst = max(abs(a - b) for ra, rb in zip(rows, ref) for a, b in zip(ra, rb))
        print("%s %s: device vs host reduction, worst printed difference %.3e" % (build, fn, worst))
        assert worst <= 1.0e-5 + 1e-12, (fn, worst)                                      # files carry 5 decimals: last-digit rounding at most
