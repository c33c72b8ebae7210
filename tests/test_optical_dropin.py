"""optical_cond.out of the zero-edit drop-in (oracle/_ref/rslmto_dropin.x; tests/test_fortran_dropin.py and
tests/test_cond_tensor_dropin.py have the machinery): with RSREC_KUBO_OPTICAL=<nw> in the environment the conductivity shim
(fortran/conductivity_gpu.f90) calls rsrec_kubo_optical after the DC tensor, at energy%fermi, on the orbital diagonals of the run's
moments, and writes omega_k, Re and Im of the sum over orbitals and vectors divided by loop_over, 7 significant digits each.

The case Generated_conductivity_fccPt_spin ('per_type', one type).  RSREC_KUBO_OPTICAL_MOMENTS=<file> makes the shim write the
diagonals it handed to the call; the file must equal Conductivity.optical on those moments and the run's mesh within the print error,
5e-7 relative per number.  Without RSREC_KUBO_OPTICAL no such file appears, no such timer region, and cond_total.out is byte for byte
the same."""
import numpy as np
import pytest

import optical_reference as O
from helpers import program_built
from rslmtoasa_amd.conductivity import Conductivity
from rslmtoasa_amd.recursion import Energy
from test_cond_tensor_dropin import namelist_value, table
from test_conductivity_dropin import run_case
from test_fortran_dropin import DROPIN

pytestmark = pytest.mark.gpu


class BareHandle:
    """A handle with no lattice and no Hamiltonian: the call needs neither (tools/time_cond_tensor.py)."""

    def __init__(self, en):
        import ctypes as C
        from rslmtoasa_amd import _lib
        from rslmtoasa_amd.recursion import Recursion
        self.en, self._L, self._h = en, _lib.lib(), C.c_void_p()
        self._check, self.timing = Recursion._check.__get__(self), Recursion.timing.__get__(self)
        self._check(self._L.rsrec_create(C.byref(self._h), 0))

    def close(self):
        self._L.rsrec_destroy(self._h)


CASE = "Generated_conductivity_fccPt_spin"
NW = 64


def run_mesh(work):
    """energy%ene of the run as energy%e_mesh forms it (energy.f90:174-207), its window and its Fermi level, from input.nml."""
    text = (work / "input.nml").read_text()
    emin, emax, fermi = (float(namelist_value(text, k)) for k in ("energy_min", "energy_max", "fermi"))
    ch = int(namelist_value(text, "channels_ldos"))
    ch = ch if ch % 2 == 0 else ch - 1
    edel = (emax - emin) / ch
    edel = (fermi - emin) / round((fermi - emin) / edel)
    return emin + edel * np.arange(ch + 10), emin, emax, fermi


def test_drop_in_writes_the_optical_conductivity(tmp_path, monkeypatch):
    if not program_built(DROPIN):               # (warns: the program holds reference object code, test_fortran_dropin.py)
        return
    monkeypatch.delenv("RSREC_HOST_COND_TAIL", raising=False)
    monkeypatch.delenv("RSREC_KUBO_OPTICAL", raising=False)
    plain = tmp_path / "plain"
    _, log0 = run_case(DROPIN, CASE, plain)
    assert not (plain / "optical_cond.out").exists() and "conductivity-optical-gpu" not in log0

    monkeypatch.setenv("RSREC_KUBO_OPTICAL", str(NW))                  # (run_case hands the environment on to the program)
    monkeypatch.setenv("RSREC_KUBO_OPTICAL_MOMENTS", "optical_moments.bin")
    work = tmp_path / "optical"
    _, log = run_case(DROPIN, CASE, work)
    assert "conductivity-optical-gpu" in log, log[-3000:]
    assert (work / "cond_total.out").read_bytes() == (plain / "cond_total.out").read_bytes()
    got = table(work / "optical_cond.out")
    assert got.shape == (NW, 3) and np.isfinite(got).all()

    ene, emin, emax, fermi = run_mesh(work)
    assert namelist_value((work / "input.nml").read_text(), "cond_calctype") == "per_type"      # one type: loop_over = 1
    L = int(namelist_value((work / "input.nml").read_text(), "cond_ll"))
    mu = np.fromfile(work / "optical_moments.bin", dtype=np.complex128).reshape((18, L, L, 1), order="F")
    assert np.abs(mu).max() > 0
    rec = BareHandle(Energy(emin, emax))
    try:
        opt = Conductivity(rec).optical(mu, ene, fermi, NW)
    finally:
        rec.close()
    assert O.orbital_err(opt, O.optical_dense(mu, ene, emin, emax, fermi, NW)) <= 1e-12
    want = np.zeros(NW, np.complex128)
    for v in range(mu.shape[3]):                                       # (the shim's sum: orbitals fastest, one term after the other)
        for l in range(18):
            want += opt[l, :, 0, v]
    want /= mu.shape[3]
    want = np.stack([(ene[1] - ene[0]) * np.arange(1, NW + 1), want.real, want.imag], axis=1)
    err = np.abs(got - want) / np.abs(want)
    print("optical_cond.out against the Python call: max relative difference %.2e, |sigma| %.2e .. %.2e" % (err.max(), np.abs(want[:, 1:]).min(), np.abs(want[:, 1:]).max()))
    assert (np.abs(want) > 0).all() and (err <= 5e-7).all(), np.argwhere(err > 5e-7)[:5]
