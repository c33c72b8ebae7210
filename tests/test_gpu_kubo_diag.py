"""The orbital-diagonal Kubo moments (rsrec_kubo_moments_diag, k_kubo_gram_diag) and the integrand from them
(rsrec_kubo_integrand_diag).  conductivity.f90:289 and :292 read mu_nm_stochastic(l, l, n, m, v) and nothing else reads the array, so
the diagonal route forms mu_diag(l, n, m, v) = mu_nm(l, l, n, m, v) alone.  Checked against the compiled reference's moments
(tests/golden/fccPt_kubo*.npz), against the full route on the same handle, for bitwise repeatability and independence of the vectors
in flight, and -- the integrand -- bitwise against rsrec_kubo_integrand on the full array built from the same diagonals.
Error measure and tolerance of the moments: those of tests/test_gpu_kubo.py (max |mu - ref| of a vector over its largest |ref|, RTOL)."""
import numpy as np
import pytest

import cond_reference as R
from helpers import RTOL, load_golden
from kubo_cases import DIAG, KK_ODD, golden_case, integrand_call, ragged_case, same_bits, vec_err
from kubo_cases import torch_first  # noqa: F401 (autouse)
from rslmtoasa_amd import _lib
from rslmtoasa_amd.conductivity import Conductivity
from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ragged():
    cases = {hoh: ragged_case(hoh) for hoh in (False, True)}
    yield cases
    for c in cases.values():
        c.rec.close()


@pytest.fixture(scope="module")
def ragged_full(ragged):
    """The full route's moments on the ragged lattices, computed once per (hoh, cond_ll) at the default options and left unchanged."""
    cache = {}

    def get(hoh, cond_ll):
        if (hoh, cond_ll) not in cache:
            c = ragged[hoh]
            c.rec.set_option("kubo_lchunk", 0)
            mu = c.full(cond_ll)
            mu.setflags(write=False)
            cache[(hoh, cond_ll)] = mu
        return cache[(hoh, cond_ll)]
    return get


# ---- 1. against the compiled reference ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fccPt_kubo", "fccPt_kubo_hoh", "fccPt_kubo_random"])
def test_diagonal_moments_match_reference(name):
    z, c = golden_case(name)
    try:
        mu = c.diag(int(z["cond_ll"]))
    finally:
        c.rec.close()
    ref = z["mu_nm"][DIAG, DIAG]
    assert mu.shape == ref.shape
    err = vec_err(mu, ref)
    print("diag vs reference", name, err)
    assert err < RTOL


# ---- 2. against the full route on the same handle ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("lchunk", [0, 3, 32])
@pytest.mark.parametrize("cond_ll", [1, 2, 3, 17, 49, 65])
@pytest.mark.parametrize("hoh", [False, True])
def test_diagonal_moments_match_full_route(hoh, cond_ll, lchunk, ragged, ragged_full):
    """cond_ll: the m = 0 copy, the first-order step, a tile border (16), a block border of the full kernel (48), the border of a
    block of right vectors (64); kubo_lchunk: left-chunk borders, with one or two vectors in the last chunk."""
    full = ragged_full(hoh, cond_ll)
    c = ragged[hoh]
    c.rec.set_option("kubo_lchunk", lchunk)
    try:
        mu = c.diag(cond_ll)
    finally:
        c.rec.set_option("kubo_lchunk", 0)
    assert np.isfinite(full).all() and np.abs(full[DIAG, DIAG]).max() > 0
    err = vec_err(mu, full[DIAG, DIAG])
    print("diag vs full", hoh, cond_ll, lchunk, err)
    assert err < RTOL


@pytest.mark.parametrize("hoh", [False, True])
def test_small_lattice_diagonals_have_the_full_route_bits(hoh, ragged, ragged_full):
    """On this lattice (338 k-steps) both contractions take 8 slices of the row index on any device, sum a slice in the same k order
    and a k-step in the same order of the four real MFMAs: the diagonal route gives the very bits of the full route's diagonals."""
    assert same_bits(ragged[hoh].diag(49), np.asfortranarray(ragged_full(hoh, 49)[DIAG, DIAG]))


# ---- 3. independence and repeatability, bitwise ------------------------------------------------------------------------------------------

def test_two_calls_same_bits(ragged):
    c = ragged[False]
    assert same_bits(c.diag(17), c.diag(17))


def test_host_and_device_output_same_bits(ragged):
    import torch
    c = ragged[True]
    L, nvec = 17, len(c.seeds)
    host = c.diag(L)
    dev = torch.zeros((nvec, L, L, 18), dtype=torch.complex128, device="cuda")      # the Fortran array (18, L, L, nvec) seen from C
    c.rec._check(c.call("rsrec_kubo_moments_diag", L, dev))
    torch.cuda.synchronize()
    assert same_bits(host, np.asfortranarray(dev.cpu().numpy().transpose(3, 2, 1, 0)))


def test_vectors_in_flight_do_not_change_a_vector(ragged):
    c = ragged[False]
    try:
        c.rec.set_option("kubo_vbatch", 3)
        three = c.diag(19)
        c.rec.set_option("kubo_vbatch", 1)
        for v in range(3):
            assert same_bits(c.diag(19, vecs=slice(v, v + 1))[..., 0], three[..., v])
    finally:
        c.rec.set_option("kubo_vbatch", 0)


def test_resident_only_then_download_same_bits(ragged):
    c = ragged[True]
    first = c.diag(17)
    c.rec._check(c.call("rsrec_kubo_moments_diag", 17, None))
    assert same_bits(c.diag(17), first)


# ---- 4. the integrand -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cond_rec():
    z, c = golden_case("fccPt_kubo")
    yield z, c
    c.rec.close()


@pytest.mark.parametrize("name", ["cond_integrand_L7", "cond_integrand_L24"])
def test_integrand_from_diagonals(name, cond_rec):
    import torch
    _, c = cond_rec
    z = load_golden(name)
    L, nvec = int(z["cond_ll"]), int(z["nvec"])
    d = np.asfortranarray(z["mu_diag"])
    full = np.zeros((18, 18, L, L, nvec), np.complex128, order="F")
    full[DIAG, DIAG] = d
    rc, ref = integrand_call(c, "rsrec_kubo_integrand", nvec, L, full, z)
    assert rc == 0
    rc, host = integrand_call(c, "rsrec_kubo_integrand_diag", nvec, L, d, z)
    assert rc == 0 and same_bits(host, ref)
    d_dev = torch.from_numpy(np.ascontiguousarray(d.transpose(3, 2, 1, 0))).cuda()
    torch.cuda.synchronize()
    rc, dev = integrand_call(c, "rsrec_kubo_integrand_diag", nvec, L, d_dev, z)
    assert rc == 0 and same_bits(dev, ref)
    # the restatement, at the tolerance of tests/test_gpu_conductivity.py, and the compiled reference's fort.123 as
    # tests/test_conductivity_oracle.py compares it (es16.6: within half a unit of the seventh digit)
    emin, emax = float(z["energy_min"]), float(z["energy_max"])
    want = R.integrand_from_diagonals(d, z["ene"], emin, emax)
    assert max(np.abs(host[l] - want[l]).max() / np.abs(want[l]).max() for l in range(18)) <= 1e-12
    mine = R.fort123(host, z["ene"], emin, emax, float(z["fermi"]))
    for calctype in ("per_type", "random_vec"):
        f = z["fort123_" + calctype]
        ulp = 10.0 ** np.floor(np.log10(np.maximum(np.abs(f), 1e-300))) * 1e-6
        assert np.all(np.abs(mine - f) <= 0.5 * ulp * 1.02 + 1e-300)


def test_resident_integrand_equals_downloaded(ragged):
    c = ragged[False]
    L, nvec = 17, len(c.seeds)
    d = c.diag(L)
    z = dict(ene=np.linspace(-0.7, 0.5, 37), energy_min=-0.8, energy_max=0.6)
    rc, res = integrand_call(c, "rsrec_kubo_integrand_diag", nvec, L, None, z)
    assert rc == 0, c.last_error()
    rc, down = integrand_call(c, "rsrec_kubo_integrand_diag", nvec, L, d, z)
    assert rc == 0 and np.isfinite(res).all() and np.abs(res).max() > 0
    assert same_bits(res, down)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_usable():
    c = ragged_case(False)
    try:
        L, nvec = 5, len(c.seeds)
        z = dict(ene=np.linspace(-0.7, 0.5, 9), energy_min=-0.8, energy_max=0.6)

        def refused(nv, ll):
            rc, _ = integrand_call(c, "rsrec_kubo_integrand_diag", nv, ll, None, z)
            assert rc == _lib.ERR_ARG and len(c.last_error()) > 0

        refused(nvec, L)                                               # nothing resident yet
        d = c.diag(L)
        assert integrand_call(c, "rsrec_kubo_integrand_diag", nvec, L, None, z)[0] == 0
        refused(nvec, L + 1)                                           # another cond_ll
        refused(nvec - 1, L)                                           # another nvec
        refused(nvec, 100000)                                          # cond_ll out of range
        rc, _ = integrand_call(c, "rsrec_kubo_integrand_diag", nvec, 100000, d, z)
        assert rc == _lib.ERR_ARG and len(c.last_error()) > 0
        assert c.call("rsrec_kubo_moments_diag", 100000, None) == _lib.ERR_ARG and len(c.last_error()) > 0
        assert integrand_call(c, "rsrec_kubo_integrand_diag", nvec, L, None, z)[0] == 0   # the refusals dropped nothing
        c.rec.update_hamiltonian()
        refused(nvec, L)                                               # rsrec_set_hamiltonian dropped the resident moments
        assert same_bits(c.diag(L), d)                                 # ... and a valid call works, with the same bits
        assert integrand_call(c, "rsrec_kubo_integrand_diag", nvec, L, None, z)[0] == 0
        nn = np.array(c.rec.lattice.nn, order="F")
        nn[1, 1] = nn[1, 1] % KK_ODD + 1                               # another neighbour in one slot: a changed lattice
        c.rec.lattice.nn = nn
        c.rec.update_lattice()
        refused(nvec, L)                                               # rsrec_set_lattice dropped them too, before any new Hamiltonian
        c.rec.update_hamiltonian()
        refused(nvec, L)
        assert np.isfinite(c.diag(L)).all()
        assert integrand_call(c, "rsrec_kubo_integrand_diag", nvec, L, None, z)[0] == 0
    finally:
        c.rec.close()


# ---- 6. the full route is untouched -----------------------------------------------------------------------------------------------------------

def test_full_route_after_diagonal_call_same_bits(ragged):
    c = ragged[True]
    c.diag(19)
    after = c.full(19)
    fresh = ragged_case(True)
    try:
        assert same_bits(after, fresh.full(19))
    finally:
        fresh.rec.close()


# ---- the Python mirror ---------------------------------------------------------------------------------------------------------------------------

def test_python_mirror_diag_and_resident_integrand():
    import rslmtoasa_amd.recursion as Rm
    z = load_golden("fccPt_kubo")
    a, b = float(z["acheb"]), float(z["bcheb"])
    half = a * float(np.float32(2) - np.float32(0.3)) / 2
    ham = Hamiltonian(ee=z["ee"], lsham=z["lsham"], hoh=False)
    lat = Lattice(nn=z["nn"], iz=z["iz"], irec=np.asarray(z["atlist"], np.int32), nmax=0, ntype=z["ee"].shape[3])
    rec = Recursion(ham, lat, Control(lld=int(z["cond_ll"]), nsp=int(z["nsp"])), Energy(b - half, b + half), device=0)
    orig = Rm.chebyshev_scaling
    Rm.chebyshev_scaling = lambda e0, e1: (a, b)
    try:
        L = int(z["cond_ll"])
        mu = rec.compute_moments_stochastic(z["v_a"], z["v_b"], L, atlist=z["atlist"], diag=True)
        assert mu.shape == (18, L, L, 1) and mu.dtype == np.complex128 and mu.flags.f_contiguous
        assert vec_err(mu, z["mu_nm"][DIAG, DIAG]) < RTOL
        cond = Conductivity(rec)
        ene = R.energy_mesh(b - half, b + half, 300)
        res = cond.integrand(None, ene)
        assert res.shape == (18, ene.size, 1) and same_bits(res, cond.integrand(mu, ene))
        assert rec.compute_moments_stochastic(z["v_a"], z["v_b"], L, atlist=z["atlist"], diag=True, resident_only=True) is None
        assert same_bits(cond.integrand(None, ene), res)
    finally:
        Rm.chebyshev_scaling = orig
        rec.close()
