"""The LDOS stage behind the Chebyshev recursion, on the device (rsrec_chebyshev_ldos, Green.chebyshev_ldos): the moments
rsrec_chebyshev left on the GPU -> the diagonal of green%chebyshev_green (green.f90:1030-1108) -> the reduction of
bands%calculate_fermi (bands.f90:258-268), without a g0 and without moving the moments.

Checker: the compiled reference's g0 of the same runs (tests/golden/*_cheb_green.npz, every 40th energy of its 2510-point mesh),
reduced with the expressions of bands.f90:258-268 (test_gpu_ldos.ldos_from_g0).  Tolerances are those of the block stage's tests
(test_gpu_ldos.py): 1e-10 of the largest LDOS against the reference run (the device's acos / sin / cos differ from the host's in the
last bits), 1e-12 against the library's own g0 route (device against device)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import load_golden, objects_from, problem_dict
from rslmtoasa_amd import _lib
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.recursion import Recursion, chebyshev_scaling
from test_gpu_green import load_green
from test_gpu_ldos import ldos_from_g0

pytestmark = pytest.mark.gpu

CHEB_CASES = ["bccFe_nsp2_cheb", "fccCu001_cheb"]


def make_rec(g, irec=None):
    irec = g["irec"] if irec is None else irec
    return Recursion(*objects_from(problem_dict(g), irec, g["lld"], nsp=g["nsp"], emin=g["emin"], emax=g["emax"]), device=0)


def full_mesh(g, z):
    """The reference's mesh of the run, energy%ene(i + 1) = energy_min + edel i for i = 0 .. channels_ldos + 9 (energy.f90:198-207).
    edel is (energy_max - energy_min) / channels_ldos snapped so that the Fermi level falls on a mesh point (:201-203); the fixture
    holds every 40th energy of that mesh, which fixes edel."""
    nen, idx = int(z["nen_full"]), z["ene_idx"]
    edel = (float(z["ene"][-1]) - float(z["ene"][0])) / float(idx[-1] - idx[0])
    ene = float(g["emin"]) + edel * np.arange(nen)
    assert np.allclose(ene[idx], z["ene"], rtol=0, atol=1e-12)
    return ene


@pytest.mark.parametrize("name", CHEB_CASES)
def test_cheb_ldos_against_reference_run(name):
    """chebyshev_recur on the GPU (moments equal to the reference's to rounding: test_chebyshev_green part (b)), then ONE call for the
    LDOS stage from the moments left on the device, against the reduction of the reference run's g0.  Every sampled energy of the
    fixture is compared."""
    z, g = load_green(name), load_golden(name)
    rec = make_rec(g)
    rec.chebyshev_recur()
    n = int(z["nrec"])
    r = Green(rec, z["ene"]).chebyshev_ldos()
    rec.close()
    dtot, dosia, dosial = ldos_from_g0(z["g0"])
    assert r["dosial"].shape == dosial.shape == (n, 18, len(z["ene"])) and r["dosia"].shape == dosia.shape and r["dtot"].shape == dtot.shape
    scale = np.abs(dosial).max()
    e_l, e_a, e_t = np.abs(r["dosial"] - dosial).max(), np.abs(r["dosia"] - dosia).max(), np.abs(r["dtot"] - dtot).max()
    print("%s: |dosial - ref| %.3e  |dosia - ref| %.3e  |dtot - ref| %.3e  scale %.3e" % (name, e_l, e_a, e_t, scale))
    assert np.isfinite(dosial).all() and np.isfinite(r["dosial"]).all()
    assert e_l <= 1e-10 * scale
    assert e_a <= 1e-10 * scale
    assert e_t <= 1e-10 * n * scale


@pytest.mark.parametrize("name", CHEB_CASES)
def test_cheb_ldos_equals_g0_route(name):
    """The same numbers as the library's own g0 route (rsrec_chebyshev_green on the moments the same recursion returned, reduced on
    the host): device against device."""
    z, g = load_green(name), load_golden(name)
    rec = make_rec(g)
    rec.chebyshev_recur()
    n = int(z["nrec"])
    gr = Green(rec, z["ene"])
    r = gr.chebyshev_ldos()
    dt2, da2, dl2 = ldos_from_g0(gr.chebyshev_green(nsites=n))
    rec.close()
    e_l, e_t = np.abs(r["dosial"] - dl2).max(), np.abs(r["dtot"] - dt2).max()
    print("%s: |dosial - g0 route| %.3e of %.3e  |dtot - g0 route| %.3e of %.3e" % (name, e_l, np.abs(dl2).max(), e_t, np.abs(dt2).max()))
    assert e_l <= 1e-12 * np.abs(dl2).max()
    assert e_t <= 1e-12 * np.abs(dt2).max()


def test_cheb_ldos_images_are_zero_padded():
    """The images the ranks all-reduce (bands.f90:271-274): this rank's sites at their global positions, zeros elsewhere."""
    name = "fccCu001_cheb"                                                               # two sites
    z, g = load_green(name), load_golden(name)
    rec = make_rec(g)
    rec.chebyshev_recur()
    gr = Green(rec, z["ene"])
    n, ntot, off = 2, 5, 2
    host = gr.chebyshev_ldos(site_offset=off, nsites_total=ntot)
    local = gr.chebyshev_ldos()
    rec.close()
    assert host["dosial"].shape == (ntot, 18, len(z["ene"])) and np.abs(local["dosial"]).max() > 0
    assert np.array_equal(host["dosial"][off:off + n], local["dosial"]) and np.array_equal(host["dosia"][off:off + n], local["dosia"])
    assert np.array_equal(host["dtot"], local["dtot"])
    mask = np.ones(ntot, bool); mask[off:off + n] = False
    assert np.all(host["dosial"][mask] == 0) and np.all(host["dosia"][mask] == 0)


DEVICE_OUTPUT_SCRIPT = r"""
import sys, numpy as np, torch
torch.cuda.init(); torch.cuda.set_device(0)          # torch's HIP runtime first, as in bench.py
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import load_golden, objects_from, problem_dict
from test_gpu_green import load_green
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.recursion import Recursion
name = "fccCu001_cheb"
z, g = load_green(name), load_golden(name)
rec = Recursion(*objects_from(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"], emin=g["emin"], emax=g["emax"]), device=0)
rec.chebyshev_recur()
gr = Green(rec, z["ene"])
n, nen, ntot, off = 2, len(z["ene"]), 5, 2
host = gr.chebyshev_ldos(site_offset=off, nsites_total=ntot)
t_tot = torch.full((nen,), -1.0, dtype=torch.float64, device="cuda")
t_ia = torch.full((nen, ntot), -1.0, dtype=torch.float64, device="cuda")              # Fortran (ntot, nen)
t_ial = torch.full((nen, 18, ntot), -1.0, dtype=torch.float64, device="cuda")         # Fortran (ntot, 18, nen)
torch.cuda.synchronize()
r = gr.chebyshev_ldos(site_offset=off, nsites_total=ntot, out=(t_tot.data_ptr(), t_ia.data_ptr(), t_ial.data_ptr()))
assert r["dtot"] is None and np.abs(host["dosial"]).max() > 0
assert np.array_equal(t_tot.cpu().numpy(), host["dtot"])
assert np.array_equal(t_ia.cpu().numpy().T, host["dosia"])
assert np.array_equal(t_ial.cpu().numpy().transpose(2, 1, 0), host["dosial"])
rec.close()
print("DEVICE_OUTPUT_OK")
"""


def test_cheb_ldos_device_outputs_match_host_outputs():
    """Outputs handed over as DEVICE buffers (the tensors a collective would reduce) receive the same bits as host arrays.
    Own process: torch's HIP runtime has to be initialised before librsrec's (as in bench.py)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", DEVICE_OUTPUT_SCRIPT, root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE_OUTPUT_OK" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_cheb_ldos_residency_rules():
    """The stage takes the moments of the LAST chebyshev_recur call and nothing else, and leaves them as they are."""
    name = "fccCu001_cheb"
    z, g = load_green(name), load_golden(name)
    rec = make_rec(g)
    gr = Green(rec, z["ene"])
    n, nm = int(z["nrec"]), 2 * int(g["lld"]) + 2
    with pytest.raises(_lib.RsrecError, match="no Chebyshev moments resident"):          # fresh handle
        gr.chebyshev_ldos()
    rec.recur_b()
    with pytest.raises(_lib.RsrecError, match="no Chebyshev moments resident"):          # block coefficients are not moments
        gr.chebyshev_ldos()
    rec.chebyshev_recur()
    with pytest.raises(_lib.RsrecError):                                                 # ... and moments are not block coefficients
        gr.block_ldos()
    before = np.zeros((18, 18, nm, n), np.complex128, order="F")
    rec.pack_moments(0, n, before)
    assert np.array_equal(before, rec.mu_n[:, :, :, :n]) and np.abs(before).max() > 0
    r1 = gr.chebyshev_ldos()
    after = np.zeros_like(before)
    rec.pack_moments(0, n, after)
    assert np.array_equal(after, before)
    r2 = gr.chebyshev_ldos()
    for k in ("dtot", "dosia", "dosial"):
        assert np.array_equal(r1[k], r2[k]), k
    with pytest.raises(_lib.RsrecError):                                                 # images too small for the rank's sites
        gr.chebyshev_ldos(site_offset=1, nsites_total=n)
    rec.close()


def test_cheb_ldos_full_mesh():
    """The reference's full 2510-point mesh of the bcc Fe run, energy_min + (i - 1) edel (full_mesh): it lies inside the open interval
    (b - a, b + a) where acos and the square root are real (on or outside it the reference gives NaN as well), so every value must be
    finite -- nothing is masked.  Two calls repeat bit for bit, and each of 64 repeated sites of one call equals the one-site call bit
    for bit (a site's numbers do not depend on which other sites share the launch)."""
    name = "bccFe_nsp2_cheb"
    z, g = load_green(name), load_golden(name)
    ene = full_mesh(g, z)
    a, b = chebyshev_scaling(g["emin"], g["emax"])
    assert len(ene) == 2510 and b - a < ene.min() and ene.max() < b + a
    nm = 2 * int(g["lld"]) + 2
    rec = make_rec(g)
    # The RECURSION splits its reductions over workgroups by the size of the batch (1 chain: 256 per chain, 64 chains: 8), so its
    # moments differ in the last bits between a one-site and a 64-site call.  `nblk` fixes that split; with it the two calls below
    # hand the LDOS stage the same bits (asserted), and any difference in the densities of states would be the stage's own.
    rec.set_option("nblk", 4)
    rec.chebyshev_recur()
    mu1 = np.zeros((18, 18, nm, 1), np.complex128, order="F")
    rec.pack_moments(0, 1, mu1)
    gr = Green(rec, ene)
    one, again = gr.chebyshev_ldos(), gr.chebyshev_ldos()
    rec.close()
    assert one["dosial"].shape == (1, 18, 2510)
    for k in ("dtot", "dosia", "dosial"):
        assert np.isfinite(one[k]).all() and np.array_equal(one[k], again[k]), k
    assert np.abs(one["dosial"]).max() > 0
    # the sub-sampled energies of the fixture are reproduced by the full-mesh run
    ref = ldos_from_g0(z["g0"])[2]
    assert np.abs(one["dosial"][:, :, z["ene_idx"]] - ref).max() <= 1e-10 * np.abs(ref).max()
    ns = 64
    rec = make_rec(g, np.repeat(g["irec"], ns))
    rec.set_option("nblk", 4)
    rec.chebyshev_recur()
    mu = np.zeros((18, 18, nm, ns), np.complex128, order="F")
    rec.pack_moments(0, ns, mu)
    many = Green(rec, ene).chebyshev_ldos()
    rec.close()
    assert many["dosial"].shape == (ns, 18, 2510) and np.isfinite(many["dosial"]).all()
    # (the stage's input: the recursion gives a repeated site the moments of the one-site call, bit for bit)
    assert all(np.array_equal(mu[:, :, :, s], mu1[:, :, :, 0]) for s in range(ns))
    for s in range(ns):
        assert np.array_equal(many["dosial"][s], one["dosial"][0]) and np.array_equal(many["dosia"][s], one["dosia"][0]), s
