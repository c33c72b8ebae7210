"""The stages on resident chains after a local-axis recursion (hamiltonian%local_axis = T, recursion.f90:1830-1832).

rsrec_block_lanczos_local_axis runs every site's chain on the global-frame blocks and conjugates the coefficients with the site's
rotation ON THE DEVICE, A' = R^H A R, B'^2 = R^H B^2 R: the arrays it returns and the chains it leaves resident are one set of bits, in
each site's local frame.  The continued fraction, zsqr, get_terminf and every epilogue are covariant under that transform, so
block_ldos / block_spectra / contour_occupation(resident=True) / pack_diag follow as after recur_b.

Fixtures: Pt2MnGa_nsp4_local_axis and _hoh -- four sites (Mn, Ga, Pt1, Pt2) with four moment directions, the compiled reference's
local-frame a_b, b2_b and its rotation matrices; 63 energies across the band (the mesh of bccFe_nsp2_block_green).
Bounds: those of the collinear tests of the same stages (tests/test_gpu_ldos.py test_resident_ldos_pipeline, tests/test_gpu_spectra.py
check (1), tests/test_gpu_contour.py resident = caller arrays bit for bit); RTOL of the parity tests for coefficients against the CPU
oracle.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from helpers import RTOL, load_golden, objects_from, problem_dict, rel_err, supercell_problem
from rslmtoasa_amd.exchange import gauss_legendre
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.recursion import Recursion
from test_gpu_green import load_green
from test_gpu_ldos import ldos_from_g0
from test_gpu_spectra import OPS21, check as check_spectra

pytestmark = pytest.mark.gpu

CASES = ["Pt2MnGa_nsp4_local_axis", "Pt2MnGa_nsp4_local_axis_hoh"]
ENE = load_green("bccFe_nsp2_block")["ene"]
E0 = float(ENE[31])
D = np.arange(18)


def make_rec(g, sites=None, lld=None):
    irec = g["irec"] if sites is None else np.asarray(g["irec"])[list(sites)]
    return Recursion(*objects_from(problem_dict(g), irec, g["lld"] if lld is None else lld, nsp=g["nsp"]), device=0)


_runs = {}


def run(name):
    """One local-axis recursion per fixture, shared and left unchanged: the returned arrays, every stage on the resident chains, the
    host path on the returned arrays, and the global-frame run of the same sites."""
    if name in _runs:
        return _runs[name]
    g = load_golden(name)
    n, lld = int(g["nrec"]), int(g["lld"])
    rec = make_rec(g)
    rec.recur_b_local_axis(g["rot"])
    a_b, b2_b = rec.a_b[:, :, :, :n].copy(), rec.b2_b[:, :, :, :n].copy()
    gr = Green(rec, ENE)
    ldos = gr.block_ldos()
    spec = gr.block_spectra(OPS21)
    x, w = gauss_legendre(8)
    occ_res = gr.contour_occupation(x, w, E0, resident=True)
    a_img, b_img = np.zeros((lld, 18, n), order="F"), np.zeros((lld, 18, n), order="F")
    rec.pack_diag(0, n, a_img, b_img)
    ldos_again = gr.block_ldos()                               # after spectra, contour and pack_diag: the chains are still B^2, untouched
    rec.zsqr()                                                 # the host path on the returned arrays
    b_sqrt = rec.b2_b[:, :, :, :n].copy()
    occ_coef = gr.contour_occupation(x, w, E0, coef=(a_b, b_sqrt))
    g0 = gr.block_green(ldos["a_inf"], ldos["b_inf"], nsites=n).copy()
    rec.recur_b()                                              # the same sites in the global frame
    ldos_glob = gr.block_ldos()
    rec.close()
    _runs[name] = dict(g=g, n=n, lld=lld, a_b=a_b, b2_b=b2_b, ldos=ldos, ldos_again=ldos_again, spec=spec, occ_res=occ_res, occ_coef=occ_coef,
                       a_img=a_img, b_img=b_img, g0=g0, ldos_glob=ldos_glob)
    return _runs[name]


@pytest.mark.parametrize("name", CASES)
def test_ldos_in_the_local_frame(name, oracle_lib):
    """block_ldos after recur_b_local_axis against bands.f90:258-268 on the CPU oracle's g0 of the REFERENCE's local-frame coefficients
    (oracle.zsqr, oracle.terminator, oracle.block_green), and against the library's host path on the returned arrays.  dosial proves the
    frame (dtot is a trace): the global-frame run of the same sites differs on a tilted site."""
    r = run(name)
    g, n = r["g"], r["n"]
    b_sqrt = oracle_lib.zsqr(g["b2_b"])
    a_inf, b_inf, _, _ = oracle_lib.terminator(g["a_b"], b_sqrt)
    g0_ref = np.stack([oracle_lib.block_green(g["a_b"][:, :, :, s], b_sqrt[:, :, :, s], ENE, a_inf[:, :, s], b_inf[:, :, s]) for s in range(n)], axis=3)
    dtot, dosia, dosial = ldos_from_g0(g0_ref)
    scale = np.abs(dosial).max()
    e = {k: np.abs(r["ldos"][k] - v).max() for k, v in (("dosial", dosial), ("dosia", dosia), ("dtot", dtot))}
    print("%s: largest LDOS %.3e; vs oracle on the reference's coefficients: dosial %.2e dosia %.2e dtot %.2e (of scale)"
          % (name, scale, e["dosial"] / scale, e["dosia"] / scale, e["dtot"] / scale))
    assert scale > 1.0                                         # states / Ry per orbital inside the band: not a comparison of noise
    assert e["dosial"] <= 1e-10 * scale and e["dosia"] <= 1e-10 * scale and e["dtot"] <= 1e-10 * n * scale
    dt2, da2, dl2 = ldos_from_g0(r["g0"])
    e2 = (np.abs(r["ldos"]["dosial"] - dl2).max() / np.abs(dl2).max(), np.abs(r["ldos"]["dtot"] - dt2).max() / np.abs(dt2).max())
    print("%s: vs the host path on the returned arrays: dosial %.2e dtot %.2e" % (name, e2[0], e2[1]))
    assert e2[0] <= 1e-12 and e2[1] <= 1e-12
    diff = np.abs(r["ldos_glob"]["dosial"][0] - r["ldos"]["dosial"][0]).max()
    print("%s: dosial of site 1, global frame against local frame: %.3e of scale" % (name, diff / scale))
    assert diff > 1e-6 * scale
    for k in ("dtot", "dosia", "dosial", "a_inf", "b_inf"):
        assert np.array_equal(r["ldos"][k], r["ldos_again"][k]), k


@pytest.mark.parametrize("name", CASES)
def test_spectra_in_the_local_frame(name):
    """block_spectra of the 21 named operators against Im Tr(O g0) of the host-path g0 (tests/test_gpu_spectra.py check, bound (1))."""
    r = run(name)
    check_spectra(r["spec"], OPS21, r["g0"], None, name)
    assert np.abs(r["spec"]).max() > 1.0


@pytest.mark.parametrize("name", CASES)
def test_contour_occupation_on_resident_local_chains(name):
    """8 Gauss-Legendre points: the resident chains give the bits of the same call on the returned arrays (b2_b after zsqr)."""
    r = run(name)
    print("%s: occ resident against caller arrays: %.3e" % (name, np.abs(r["occ_res"] - r["occ_coef"]).max()))
    assert np.isfinite(r["occ_res"]).all() and np.abs(r["occ_res"]).max() > 0
    assert np.array_equal(r["occ_res"], r["occ_coef"])


@pytest.mark.parametrize("name", CASES)
def test_resident_chains_are_the_returned_arrays(name):
    """One source of truth: pack_diag's images are the real diagonals of the returned arrays, bit for bit; b2 of level 1 is exactly 1
    and a of level lld exactly 0 (recursion.f90:1836-1837), and the returned arrays are the reference's local-frame coefficients."""
    r = run(name)
    assert np.array_equal(r["a_img"], r["a_b"][D, D].real.transpose(1, 0, 2))
    assert np.array_equal(r["b_img"], r["b2_b"][D, D].real.transpose(1, 0, 2))
    assert np.all(r["b_img"][0] == 1.0) and np.all(r["a_img"][-1] == 0.0)
    assert np.all(r["a_b"][:, :, -1] == 0) and all(np.array_equal(r["b2_b"][:, :, 0, s], np.eye(18)) for s in range(r["n"]))
    assert rel_err(r["a_b"], r["g"]["a_b"]) < RTOL and rel_err(r["b2_b"], r["g"]["b2_b"]) < RTOL


def test_one_site_alone_equals_its_column():
    """Site 3 of the four in a call of its own: the same bits, in the returned arrays and in the LDOS of the resident chain."""
    name = CASES[0]
    r = run(name)
    g, s = r["g"], 2
    rec = make_rec(g, sites=[s])
    rec.recur_b_local_axis(g["rot"][:, :, s:s + 1])
    assert np.array_equal(rec.a_b[:, :, :, 0], r["a_b"][:, :, :, s]) and np.array_equal(rec.b2_b[:, :, :, 0], r["b2_b"][:, :, :, s])
    one = Green(rec, ENE).block_ldos()
    rec.close()
    assert np.array_equal(one["dosial"][0], r["ldos"]["dosial"][s]) and np.array_equal(one["a_inf"][:, :, 0], r["ldos"]["a_inf"][:, :, s])


def su2(rng):
    q = rng.standard_normal(4); q /= np.linalg.norm(q)
    u = np.array([[q[0] + 1j * q[3], q[2] + 1j * q[1]], [-q[2] + 1j * q[1], q[0] - 1j * q[3]]])
    return np.kron(u, np.eye(9))                               # spin-major 18 x 18: orbitals 1-9 up, 10-18 down


@pytest.mark.parametrize("hoh", [False, True])
@pytest.mark.parametrize("lld", [2, 5])
def test_random_rotations_on_a_supercell(lld, hoh, oracle_lib):
    """Random SU(2) x 1 rotations per site on a 128-atom bcc cell (nothing leans on the physical rot), lld = 2 (one a and one b2 matrix per
    site are rotated) and 5; the spin-orbit term of the nsp = 4 iron fixture, so that the per-chain on-site term R l.s R^H is there.
    Reference: the CPU oracle on blocks rotated as rotate_to_local_axis does (hamiltonian.f90:2442-2465: ee, eeo, enim, not lsham).  The
    stages on the resident chains then give what the host path gives on the returned arrays."""
    rng = np.random.default_rng(7 + lld + 10 * hoh)
    p = supercell_problem((4, 4, 4), hoh=hoh)
    p["lsham"] = load_golden("bccFe_nsp4_block")["lsham"]
    assert p["lsham"].shape == (18, 18, 1) and np.abs(p["lsham"]).max() > 0
    irec = np.array([1, 30, 64], np.int32)
    n = len(irec)
    rot = np.stack([su2(rng) for _ in range(n)], axis=2)
    rec = Recursion(*objects_from(p, irec, lld, nsp=4), device=0)
    rec.recur_b_local_axis(rot)
    worst = 0.0
    for s in range(n):
        R = rot[:, :, s]
        q = dict(p)
        for k in ("ee", "eeo", "enim"):
            if k in p:
                q[k] = np.asfortranarray(np.einsum("ji,jk...,kl->il...", R.conj(), p[k], R))
        a_o, b_o = oracle_lib.Oracle(q).block_lanczos(irec[s:s + 1], lld)
        worst = max(worst, rel_err(rec.a_b[:, :, :, s:s + 1], a_o), rel_err(rec.b2_b[:, :, :, s:s + 1], b_o))
    print("lld %d hoh %d: coefficients against the oracle on rotated blocks %.2e" % (lld, hoh, worst))
    assert worst < RTOL
    assert np.all(rec.a_b[:, :, -1] == 0) and all(np.array_equal(rec.b2_b[:, :, 0, s], np.eye(18)) for s in range(n))
    a_b, b2_b = rec.a_b[:, :, :, :n].copy(), rec.b2_b[:, :, :, :n].copy()
    a_img, b_img = np.zeros((lld, 18, n), order="F"), np.zeros((lld, 18, n), order="F")
    rec.pack_diag(0, n, a_img, b_img)
    assert np.array_equal(a_img, a_b[D, D].real.transpose(1, 0, 2)) and np.array_equal(b_img, b2_b[D, D].real.transpose(1, 0, 2))
    ene = np.linspace(-0.6, 0.2, 9)
    gr = Green(rec, ene)
    ldos = gr.block_ldos(eta=5e-3j)
    rec.zsqr()
    dt, da, dl = ldos_from_g0(gr.block_green(ldos["a_inf"], ldos["b_inf"], eta=5e-3j, nsites=n))
    rec.close()
    err = np.abs(ldos["dosial"] - dl).max() / np.abs(dl).max()
    print("lld %d hoh %d: dosial of the resident chains against the host path %.2e, largest %.3e" % (lld, hoh, err, np.abs(dl).max()))
    assert np.abs(dl).max() > 0.1 and err <= 1e-12


def test_repeatable_and_last_call_stays_resident():
    """Two local-axis calls give the same bits.  A recur_b after a local-axis call, and a local-axis call after a recur_b, leave the
    chains of the LAST call resident: the stages give the bits of a fresh handle that made that call alone.  No tolerance."""
    name = CASES[0]
    r = run(name)
    g, n = r["g"], r["n"]
    rec = make_rec(g)
    gr = Green(rec, ENE)
    rec.recur_b()
    rec.recur_b_local_axis(g["rot"])
    assert np.array_equal(rec.a_b[:, :, :, :n], r["a_b"]) and np.array_equal(rec.b2_b[:, :, :, :n], r["b2_b"])
    l1, s1 = gr.block_ldos(), gr.block_spectra(OPS21)
    rec.recur_b_local_axis(g["rot"])
    assert np.array_equal(rec.a_b[:, :, :, :n], r["a_b"]) and np.array_equal(rec.b2_b[:, :, :, :n], r["b2_b"])
    l2 = gr.block_ldos()
    rec.recur_b()
    lg = gr.block_ldos()
    rec.close()
    for k in ("dtot", "dosia", "dosial", "a_inf", "b_inf"):
        assert np.array_equal(l1[k], r["ldos"][k]) and np.array_equal(l2[k], r["ldos"][k]), k
        assert np.array_equal(lg[k], r["ldos_glob"][k]), k
    assert np.array_equal(s1, r["spec"])
