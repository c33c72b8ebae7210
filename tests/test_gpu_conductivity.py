"""The conductivity integrand on the GPU (rsrec_kubo_integrand, rslmtoasa_amd.conductivity) against the numpy restatement of
calculate_gamma_nm + calculate_conductivity_tensor (tests/cond_reference.py, itself pinned to the compiled reference by
tests/test_conductivity_oracle.py).  Error measure: max |integrand - restatement| of an orbital over all energies and vectors,
divided by the largest |restatement| of that orbital."""
import ctypes as C

import numpy as np
import pytest

import cond_reference as R
from helpers import load_golden
from rslmtoasa_amd import _lib
from rslmtoasa_amd.conductivity import Conductivity
from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion

pytestmark = pytest.mark.gpu
TOL = 1e-12


def make_rec(z, energy):
    p = {k: z[k] for k in ("nn", "iz", "ee", "lsham", "eeo", "enim") if k in z}
    ham = Hamiltonian(ee=p["ee"], lsham=p["lsham"], eeo=p.get("eeo"), enim=p.get("enim"), hoh=bool(int(z["hoh"])))
    lat = Lattice(nn=p["nn"], iz=p["iz"], irec=np.asarray(z["atlist"], np.int32), nmax=0, ntype=p["ee"].shape[3])
    return Recursion(ham, lat, Control(lld=int(z["cond_ll"]), nsp=int(z["nsp"])), energy, device=0)


def window(z):
    """energy_min / energy_max whose Chebyshev scaling is the fixture's a, b (chebyshev_scaling inverted)."""
    a, b = float(z["acheb"]), float(z["bcheb"])
    half = a * float(np.float32(2) - np.float32(0.3)) / 2
    return b - half, b + half


def same_bits(a, b):
    return np.array_equal(np.ravel(a, order="K").view(np.float64), np.ravel(b, order="K").view(np.float64))


@pytest.fixture(scope="module")
def cond():
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's (as bench.py does)
    torch.cuda.set_device(0)
    rec = make_rec(load_golden("fccPt_kubo"), Energy(-0.8, 0.6))
    yield Conductivity(rec)
    rec.close()


def orbital_err(x, ref):
    return max(np.abs(x[l] - ref[l]).max() / np.abs(ref[l]).max() for l in range(18))


def device_moments(d, seed=0):
    """mu_nm (18, 18, L, L, nvec) on the GPU as a C-order tensor (nvec, L, L, 18, 18): off-diagonal entries random (the integrand
    must not read them), orbital diagonals = d(l, n, m, v)."""
    import torch
    nvec, L = d.shape[3], d.shape[1]
    g = torch.Generator(device="cuda").manual_seed(seed)
    mu = torch.randn((nvec, L, L, 18, 18), dtype=torch.complex128, device="cuda", generator=g)
    mu.diagonal(dim1=3, dim2=4).copy_(torch.from_numpy(np.ascontiguousarray(d.transpose(3, 2, 1, 0))).cuda())
    return mu


def random_diagonals(L, nvec, seed):
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    decay = 1.0 / (1.0 + 0.05 * (n[:, None] + n[None, :]))
    return (rng.standard_normal((18, L, L, nvec)) + 1j * rng.standard_normal((18, L, L, nvec))) * decay[None, :, :, None]


def mesh(nen, emin, emax):
    """nen energies: the reference's mesh for nen = 2510 (channels_ldos = 2500); otherwise nen points inside the window (a reference
    mesh of few channels puts its 10 extra points past |x| = 1, where the integrand is NaN in the reference too)."""
    if nen == 2510:
        return R.energy_mesh(emin, emax, 2500)
    return np.linspace(emin, emax, nen + 2)[1:-1]


@pytest.mark.parametrize("name", ["fccPt_kubo", "fccPt_kubo_hoh", "fccPt_kubo_random"])
def test_integrand_on_reference_moments(name, cond):
    z = load_golden(name)
    mu = z["mu_nm"]
    ene = R.energy_mesh(cond.en.energy_min, cond.en.energy_max, 2500)
    got = cond.integrand(mu, ene)
    ref = R.integrand_factorised(mu, ene, cond.en.energy_min, cond.en.energy_max)
    assert got.shape == (18, 2510, mu.shape[4])
    assert orbital_err(got, ref) <= TOL


CASES = [(1, 1, 1), (1, 3, 37), (2, 8, 2510), (17, 3, 37), (17, 1, 2510), (50, 8, 2510), (50, 1, 1), (131, 3, 2510), (131, 8, 37),
         (500, 1, 2510), (500, 3, 37)]


@pytest.mark.parametrize("L,nvec,nen", CASES)
def test_integrand_random_moments(L, nvec, nen, cond):
    d = random_diagonals(L, nvec, 100 * L + nvec)
    ene = mesh(nen, cond.en.energy_min, cond.en.energy_max)
    got = cond.integrand(device_moments(d, seed=L), ene)
    ref = R.integrand_from_diagonals(d, ene, cond.en.energy_min, cond.en.energy_max)
    assert got.shape == (18, nen, nvec)
    assert orbital_err(got, ref) <= TOL


def test_two_calls_same_bits(cond):
    d = random_diagonals(131, 3, 5)
    mu = device_moments(d)
    ene = R.energy_mesh(cond.en.energy_min, cond.en.energy_max, 2500)
    a, b = cond.integrand(mu, ene), cond.integrand(mu, ene)
    assert same_bits(a, b)


def test_host_and_device_moments_same_bits(cond):
    d = random_diagonals(17, 3, 9)
    mu_dev = device_moments(d, seed=3)
    mu_host = np.asfortranarray(mu_dev.cpu().numpy().transpose(4, 3, 2, 1, 0))      # the same Fortran array in host memory
    ene = mesh(37, cond.en.energy_min, cond.en.energy_max)
    a, b = cond.integrand(mu_host, ene), cond.integrand(mu_dev, ene)
    assert same_bits(a, b)
    assert orbital_err(a, R.integrand_from_diagonals(d, ene, cond.en.energy_min, cond.en.energy_max)) <= TOL


def test_bad_arguments_give_errors(cond):
    rec = cond.recursion
    L = _lib.lib()
    mu = np.zeros((18, 18, 4, 4, 1), np.complex128, order="F")
    ene = np.linspace(-0.5, 0.5, 9)
    out = np.zeros((18, 9, 1), np.complex128, order="F")
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    good = (rec._h, 1, 4, p(mu), 9, p(ene), -0.8, 0.6, p(out))
    bad = [(None,) + good[1:], good[:1] + (0,) + good[2:], good[:2] + (0,) + good[3:], good[:2] + (100000,) + good[3:],
           good[:3] + (None,) + good[4:], good[:4] + (0,) + good[5:], good[:5] + (None,) + good[6:], good[:6] + (0.6, 0.6) + good[8:],
           good[:6] + (0.6, -0.8) + good[8:], good[:6] + (float("nan"), 0.6) + good[8:], good[:8] + (None,)]
    for args in bad:
        assert L.rsrec_kubo_integrand(*args) == _lib.ERR_ARG
    buf = C.create_string_buffer(512)
    L.rsrec_last_error(rec._h, buf, 512)
    assert b"rsrec_kubo_integrand" in buf.value
    assert L.rsrec_kubo_integrand(*good) == 0                          # the handle is still usable
    with pytest.raises(ValueError):
        cond.integrand(np.zeros((18, 18, 4, 5, 1), np.complex128), ene)


def test_end_to_end_gpu_moments_then_integrand(cond):
    """GPU moments from the fccPt_kubo inputs, then the GPU integrand, against the restatement on the reference's own mu_nm."""
    import rslmtoasa_amd.recursion as Rm
    z = load_golden("fccPt_kubo")
    emin, emax = window(z)
    rec = make_rec(z, Energy(emin, emax))
    orig = Rm.chebyshev_scaling
    Rm.chebyshev_scaling = lambda e0, e1: (float(z["acheb"]), float(z["bcheb"]))     # the fixture's a, b to the last bit
    try:
        mu = rec.compute_moments_stochastic(z["v_a"], z["v_b"], int(z["cond_ll"]), atlist=z["atlist"])
    finally:
        Rm.chebyshev_scaling = orig
    ene = R.energy_mesh(emin, emax, 2500)
    got = Conductivity(rec).integrand(mu, ene)
    rec.close()
    ref = R.integrand_factorised(z["mu_nm"], ene, emin, emax)
    assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max()
