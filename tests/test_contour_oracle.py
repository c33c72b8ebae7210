"""The numpy restatement of the Gauss-Legendre contour stages (contour_reference.py) against the compiled reference's own routines
(tests/golden/contour_block.npz, contour_cheb.npz, written by tools/contour_fixture): gij_eta / gji_eta, T_comm_xc and the occupations
from the stored diagonals, on the reference's coefficients.  Block g comes from the C oracle's block_green with eta, as
test_oracle_block_green_eta_pinned_by_reference uses it; Chebyshev g from chebyshev_green_ij_eta restated in numpy.

Bar: the rule of test_exchange_oracle.py, 1e-12 relative to the pair's scale; quantities that vanish by symmetry are judged on that
scale, and a contour sum on its largest |summand| (small values times weights of several thousand, and the sum can cancel).
Measured here (restatement vs compiled reference, CPU): xc 5e-15 or better, the diagonals 8e-16; the helpers' x, w and dmat equal the
reference's to the last bit.  eta = cmplx(0.0_rp, res) in the reference has no KIND: it is rounded to single precision, and so is
contour_eta (without that rounding the restatement is 4e-9 off)."""
import numpy as np
import pytest

from contour_reference import chebyshev_green_eta, contour_eta, contour_pair, gij_gji, occupation
from exchange_reference import PI
from helpers import load_golden
from rslmtoasa_amd.exchange import contour_dmat, gauss_legendre

TOL = 1e-12
NAMES = ("contour_block", "contour_cheb")


def chain_g(z, oracle_lib=None):
    """g (18, 18, 64, nchains) of the fixture's chains at the contour points."""
    e0 = float(z["ene"][int(z["fermi_point"]) - 1])
    eta = contour_eta(z["x"])
    if int(z["kind"]) == 1:
        return chebyshev_green_eta(z["mu_n"], e0, eta, float(z["emin"]), float(z["emax"]))
    n = z["a_b"].shape[3]
    g = np.zeros((18, 18, 64, n), np.complex128)
    for s in range(n):
        for k in range(64):
            g[:, :, k, s] = oracle_lib.block_green(z["a_b"][:, :, :, s], z["b_sqrt"][:, :, :, s], np.array([e0]), z["a_inf"][:, :, s], z["b_inf"][:, :, s],
                                                   eta=1j * eta[k])[:, :, 0]
    return g


G_CACHE = {}


def fixture(name, oracle_lib):
    if name not in G_CACHE:
        z = load_golden(name)
        G_CACHE[name] = (z, chain_g(z, oracle_lib))
    return G_CACHE[name]


@pytest.mark.parametrize("name", NAMES)
def test_helpers_reproduce_the_reference_inputs(name, oracle_lib):
    z, _ = fixture(name, oracle_lib)
    x, w = gauss_legendre(64)
    assert np.array_equal(x, z["x"]) and np.array_equal(w, z["w"])             # the same operations in the same order
    assert np.array_equal(contour_dmat(z["ee"], [1, 2], np.array([(1, 2)] * z["dmat"].shape[3])), z["dmat"])
    assert abs(z["ene"][int(z["fermi_point"]) - 1] - float(z["fermi"])) <= 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_intersite_gf_eta(name, oracle_lib):
    z, g = fixture(name, oracle_lib)
    pts = np.asarray(z["eta_points"])
    for q in range(z["xc"].shape[1]):
        gij, gji = gij_gji(g[..., 4 * q:4 * q + 4], False)
        for mine, ref in ((gij[pts], z["gij_eta"][..., q]), (gji[pts], z["gji_eta"][..., q])):
            scale = np.abs(ref).max()                                          # the pair's scale: at large eta gij is the small
            dev = np.abs(mine - ref).max() / scale                             # difference of four chains' g ~ 1 / z
            print("%s pair %d: worst deviation / the pair's largest element %.2e" % (name, q, dev))
            assert dev <= TOL


@pytest.mark.parametrize("name", NAMES)
def test_t_comm_xc(name, oracle_lib):
    z, g = fixture(name, oracle_lib)
    for q in range(z["xc"].shape[1]):
        xc, rows = contour_pair(g[..., 4 * q:4 * q + 4], False, z["dmat"][..., q], z["x"], z["w"])
        scale = max(np.abs(z["xc"][:, q]).max(), np.abs(rows).max() * 1.0e3 / 4.0 / PI)
        dev = np.abs(xc - z["xc"][:, q]).max() / scale
        print("%s pair %d: |xc| max %.3e, largest summand %.3e, deviation / scale %.2e" % (name, q, np.abs(z["xc"][:, q]).max(), np.abs(rows).max() * 1.0e3 / 4.0 / PI, dev))
        assert dev <= TOL
        assert np.abs(z["xc"][0, q]) > 0


@pytest.mark.parametrize("name", NAMES)
def test_occupation_from_the_stored_diagonals(name, oracle_lib):
    z, g = fixture(name, oracle_lib)
    d = np.arange(18)
    for q in range(z["xc"].shape[1]):
        ref = z["gdiag"][..., q]                                               # (18, 64, 4): the pair's chains as four sites
        mine = g[..., 4 * q:4 * q + 4][d, d]
        dev = np.abs(mine - ref).max() / np.abs(ref).max()
        print("%s pair %d: diagonal deviation / scale %.2e" % (name, q, dev))
        assert dev <= TOL
        y = (ref.real * z["w"][None, :, None]) / (z["x"] * z["x"])[None, :, None]
        assert np.abs(occupation(mine, z["x"], z["w"]) - occupation(ref, z["x"], z["w"])).max() <= TOL * max(np.abs(y).max() / PI, 1.0)
