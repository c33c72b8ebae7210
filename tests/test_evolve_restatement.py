"""The numpy restatement the GPU tests of rsrec_chebyshev_evolve compare with (tests/evolve_reference.py), held to references of its own,
and the host-side front ends (evolution_weights, evolution_order, position_commutator, Conductivity.spreading).  No GPU.

dense_operator against the C oracle: r^H V_a V_b r (and r^H V_a H~ V_b r) from the dense matrices against Oracle.kubo_moments at
cond_ll = 1 (2) on the ragged 75-atom lattice, at helpers.RTOL of the largest element.

The recurrence against exact_step (eigh and divided differences) on the periodic bcc Fe 2 x 2 x 2 cell with D from position_commutator
and the golden slot_vec, a tau = 24.9.  Bound: 100 x the sum of |w_n| over the neglected orders, from a table twice as long (the factor
covers ||D|| tau and the length of the sums).  Both sides get the Hermitian part of the fixture's H, whose blocks are adjoint pairs to
1e-13 only.  Measured with korder = evolution_order(tau, a) = 56 (bound 5.6e-13): one step psi 3.0e-15, chi 2.3e-15; two steps against
one of 2 tau psi 6.1e-15, chi 5.0e-15.  With korder 36, 20 short, the deviation is 9.7e-5 (psi) and 7.6e-5 (chi) after one step, far
above 1e-12: the bound is not vacuous."""
import numpy as np
import pytest

import evolve_reference as E
from bloch_reference import fixture_case
from helpers import RTOL, load_golden, supercell_problem
from pair_direct_reference import dense_h
from rslmtoasa_amd.conductivity import Conductivity
from rslmtoasa_amd.recursion import evolution_order, evolution_weights, kubo_greenwood_weights, position_commutator, chebyshev_scaling

DIMS = (2, 2, 2)
A_TAU = 24.9


@pytest.mark.parametrize("hoh", [False, True])
def test_dense_operator_matches_the_oracle(hoh, oracle_lib):
    p, (v_a, v_b, vo_a, vo_b), seeds, coefs = E.ragged_problem(hoh)
    a, b = 60.0, 0.1
    mu = oracle_lib.Oracle(p).kubo_moments(seeds, coefs, 2, a, b, v_a, v_b, vo_a, vo_b)
    H = dense_h(p)
    Ht = (H - b * np.eye(H.shape[0])) / a
    Va, Vb = E.dense_operator(p, v_a, vo_a), E.dense_operator(p, v_b, vo_b)
    for v in range(len(seeds)):
        r = E.seed_vector(E.KK_ODD, seeds[v], coefs[v])
        for what, mine, ref in (("cond_ll = 1", r.conj().T @ (Va @ (Vb @ r)), mu[:, :, 0, 0, v]),
                                ("H~ in between", r.conj().T @ (Va @ (Ht @ (Vb @ r))), mu[:, :, 1, 0, v])):
            dev = np.abs(mine - ref).max() / np.abs(ref).max()
            print("hoh=%d vector %d %s: %.2e" % (hoh, v, what, dev))
            assert dev <= RTOL, (what, v, dev)


@pytest.fixture(scope="module")
def fe_cell():
    """H, D, a, b, a seed vector and chi = a second random vector on the periodic bcc Fe cell"""
    _, _, _, a, b, _, _, _, _, _ = fixture_case(False)
    p = supercell_problem(DIMS)
    H = dense_h(p)
    assert np.abs(H - H.conj().T).max() <= 1e-12 * np.abs(H).max()             # the fixture's blocks are adjoint pairs to 1e-13, as the reference
    H = 0.5 * (H + H.conj().T)                                                  # assembled them; eigh wants the Hermitian part, and so both sides get it
    d_op = position_commutator(p["ee"], load_golden("bccFe_nsp2_block")["slot_vec"], (1.0, 0.0, 0.0))
    assert np.all(d_op[:, :, 0] == 0)
    Dm = E.dense_operator(p, d_op)
    kk = H.shape[0] // 18
    rng = np.random.default_rng(5)
    seeds = np.arange(1, kk + 1, dtype=np.int32)
    psi = E.seed_vector(kk, seeds, np.exp(2j * np.pi * rng.random(kk)) / np.sqrt(kk))
    chi = E.seed_vector(kk, seeds, np.exp(2j * np.pi * rng.random(kk)) / np.sqrt(kk)) @ (rng.standard_normal((18, 18)) / 4)
    return H, Dm, a, b, psi, chi


def deviations(fe_cell, korder, steps):
    H, Dm, a, b, psi, chi = fe_cell
    tau = A_TAU / a
    w = evolution_weights(tau, korder, a, b)
    Ht = (H - b * np.eye(H.shape[0])) / a
    p, c = psi, chi
    for _ in range(steps):
        p, c = E.step(Ht, Dm / a, w, p, c)
    U, L = E.exact_step(H, Dm, steps * tau)
    table = np.abs(evolution_weights(tau, 2 * korder, a, b))
    return np.abs(p - U @ psi).max(), np.abs(c - (L @ psi + U @ chi)).max(), 100.0 * table[korder:].sum()


@pytest.mark.parametrize("steps", [1, 2])
def test_step_matches_the_eigen_decomposition(steps, fe_cell):
    a = fe_cell[2]
    korder = evolution_order(A_TAU / a, a)
    assert A_TAU + 20 < korder < A_TAU + 60
    dpsi, dchi, bound = deviations(fe_cell, korder, steps)
    print("korder %d, %d step(s): psi %.2e, chi %.2e, bound %.2e" % (korder, steps, dpsi, dchi, bound))
    assert bound < 1e-11 and dpsi <= bound and dchi <= bound
    dpsi, dchi, _ = deviations(fe_cell, korder - 20, steps)
    print("korder %d: psi %.2e, chi %.2e" % (korder - 20, dpsi, dchi))
    assert dpsi > 1e-12 and dchi > 1e-12


def test_commutator_is_the_position_commutator():
    """on a cell large enough that no two slots of an atom reach the same neighbour, D = X H - H X block by block for unwrapped
    displacements: checked through the identity D_ij = (r_i - r_j) H_ij on the bonds"""
    p = supercell_problem((4, 4, 4))
    sv = load_golden("bccFe_nsp2_block")["slot_vec"]
    d = np.array([0.3, -1.0, 2.0])
    d_op = position_commutator(p["ee"], sv, d, alat=2.5)
    Dm, H = E.dense_operator(p, d_op), dense_h(dict(p, lsham=np.zeros_like(p["lsham"])))
    nn = p["nn"]
    for i in (0, 17, 63):
        for m in range(1, int(nn[i, 0])):
            j = int(nn[i, m]) - 1
            want = -2.5 * float(sv[m] @ d) / np.linalg.norm(d) * H[18 * i:18 * i + 18, 18 * j:18 * j + 18]
            assert np.abs(Dm[18 * i:18 * i + 18, 18 * j:18 * j + 18] - want).max() <= 1e-15 * max(1.0, np.abs(want).max())
    assert np.abs(Dm + Dm.conj().T).max() <= 1e-11 * np.abs(Dm).max()          # [X, H] is anti-Hermitian (the fixture's blocks are adjoint pairs to 1e-13 absolute)
    ob = np.random.default_rng(1).standard_normal((18, 18)) + 0j
    d2, do = position_commutator(p["ee"], sv, d, alat=2.5, eeo_factor=ob)
    assert np.array_equal(d2, d_op) and np.allclose(do[:, :, 3, 0], d_op[:, :, 3, 0] @ ob, rtol=0, atol=1e-15)


def test_weights_are_the_bessel_coefficients():
    jv = pytest.importorskip("scipy.special").jv
    for tau, korder, a, b in ((0.41, 66, 60.0, 0.1), (1.7, 140, 51.3, -0.4), (0.01, 12, 3.0, 0.0)):
        n = np.arange(korder)
        want = (2.0 - (n == 0)) * (-1j) ** n * jv(n, a * tau) * np.exp(-1j * b * tau)
        dev = np.abs(evolution_weights(tau, korder, a, b) - want).max()
        print("a tau = %.3g: %.2e" % (a * tau, dev))
        assert dev <= 1e-15, (tau, korder, a, b)


def test_evolution_order_bounds_the_first_neglected_coefficient():
    for tau, a in ((0.41, 60.0), (0.05, 60.0), (2.0, 51.3)):
        k = evolution_order(tau, a)
        mag = np.abs(evolution_weights(tau, 2 * k + 8, a, 0.0))
        assert np.all(mag[k:] < 1e-14) and mag[k - 1] >= 1e-14, (tau, a, k)
        assert evolution_order(tau, a, tol=1e-6) < k


def test_spreading_from_the_restatement():
    """Conductivity.spreading on the restated call: the axes it sums, t and D = DX^2 / t (against kubo_greenwood_weights, which shares
    its formula: plumbing only), and a state that has not moved has not spread.  The expansion itself is held to an eigen-decomposition
    by test_spreading_dos_is_the_broadened_spectrum."""
    _, _, _, a, b, _, emin, emax, _, _ = fixture_case(False)
    a, b = chebyshev_scaling(emin, emax)
    p = supercell_problem(DIMS)
    H = dense_h(p)
    Dm = E.dense_operator(p, position_commutator(p["ee"], load_golden("bccFe_nsp2_block")["slot_vec"], (0, 0, 1)))
    kk = H.shape[0] // 18
    rng = np.random.default_rng(9)
    seeds = np.tile(np.arange(1, kk + 1, dtype=np.int32), (2, 1))
    coefs = np.exp(2j * np.pi * rng.random((2, kk))) / np.sqrt(kk)
    tau, mom, nt, stride = 6.0 / a, 24, 3, 2
    w = evolution_weights(tau, evolution_order(tau, a), a, b)
    ref = E.evolve(H, Dm, a, b, seeds, coefs, w, nt, stride, mom)
    idx = np.arange(18)
    evo = {"m_diag": ref["m_full"][idx, idx], "m0_diag": ref["m0_full"][idx, idx]}
    ene = np.linspace(emin + 0.2 * (emax - emin), emax - 0.2 * (emax - emin), 5)
    got = Conductivity.spreading(None, evo, ene, emin, emax, tau, stride)
    d = kubo_greenwood_weights(ene, mom, emin, emax)[0].real
    dos = d.T @ evo["m0_diag"].real.sum(axis=(0, 2))
    num = d.T @ evo["m_diag"].real.sum(axis=(0, 3))
    assert np.allclose(got["t"], tau * stride * np.arange(1, nt + 1), rtol=1e-15)
    assert np.allclose(got["dos"], dos, rtol=1e-12) and np.all(dos > 0)
    assert np.allclose(got["dx2"], num / dos[:, None], rtol=1e-10) and np.all(got["dx2"] > 0)
    assert np.allclose(got["diffusion"], got["dx2"] / got["t"][None, :], rtol=1e-15)
    still = E.evolve(H, 0.0 * Dm, a, b, seeds, coefs, w, 1, 1, mom)
    assert not still["m_full"].any()


def test_spreading_dos_is_the_broadened_spectrum():
    """With one-atom seeds on every atom the m0 moments sum to Tr T_n(H~) exactly, so the DOS spreading divides by must be the spectrum
    of H from eigh with every level broadened by the Jackson kernel, sum_k sum_n g_n (2 - delta_n0) cos(n acos x) cos(n acos x_k) /
    (pi a sqrt(1 - x^2)) -- closed forms on the eigenvalues, no recurrence and no moments -- and DX^2 with chi = psi is then exactly 1."""
    _, _, _, _, _, _, emin, emax, _, _ = fixture_case(False)
    a, b = chebyshev_scaling(emin, emax)
    H = dense_h(supercell_problem(DIMS))
    H = 0.5 * (H + H.conj().T)
    kk, mom = H.shape[0] // 18, 40
    seeds = np.arange(1, kk + 1, dtype=np.int32)[:, None]
    ref = E.evolve(H, np.zeros_like(H), a, b, seeds, np.ones((kk, 1), np.complex128), np.array([1.0, 0.0]), 1, 1, mom)
    idx = np.arange(18)
    m0 = ref["m0_full"][idx, idx]
    ene = np.linspace(emin + 0.1 * (emax - emin), emax - 0.1 * (emax - emin), 7)
    got = Conductivity.spreading(None, {"m_diag": m0[:, :, None, :], "m0_diag": m0}, ene, emin, emax, 0.3, 2)
    xk = (np.linalg.eigvalsh(H) - b) / a
    assert np.abs(xk).max() < 1
    n = np.arange(mom)
    g = ((mom - n + 1) * np.cos(np.pi * n / (mom + 1)) + np.sin(np.pi * n / (mom + 1)) / np.tan(np.pi / (mom + 1))) / (mom + 1)
    g[1:] *= 2
    x = (ene - b) / a
    dos = np.einsum("n,ne,nk->e", g, np.cos(np.outer(n, np.arccos(x))), np.cos(np.outer(n, np.arccos(xk)))) / (np.pi * a * np.sqrt(1 - x ** 2))
    dev = np.abs(got["dos"] - dos).max() / np.abs(dos).max()
    print("DOS against the broadened spectrum: %.2e" % dev)
    assert dev <= 1e-11 and np.all(dos > 0)
    assert np.abs(got["dx2"] - 1.0).max() <= 1e-12 and np.allclose(got["t"], [0.6]) and np.allclose(got["diffusion"], got["dx2"] / 0.6)
