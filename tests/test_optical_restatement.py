"""The numpy restatement of the optical conductivity (tests/optical_reference.py) against what it restates, without a GPU:
  * the density J(i,j) = sum D(i,n) mu(n,m) D(j,m) of moments built from a dense Hermitian H equals the eigen-decomposition
    sum_{alpha beta} <r|beta> K(x_j, eps_beta) <beta|v_a|alpha> K(x_i, eps_alpha) <alpha|v_b r>,  K(x, eps) = sum_n D(x,n) T_n(eps);
  * the factorised, tiled form the kernels compute equals the literal formula at the shapes the GPU test runs;
  * Fermi levels do not see each other;
  * at T = 0 and a Fermi level between mesh points only the terms x_i <= x_F < x_{i+k} contribute."""
import numpy as np
import pytest

import optical_reference as O


def chebyshev_of_matrix(H, L):
    T = [np.eye(H.shape[0], dtype=np.complex128), H.astype(np.complex128)]
    for _ in range(2, L):
        T.append(2.0 * H @ T[-1] - T[-2])
    return T[:L]


def test_density_is_the_eigen_decomposition():
    rng = np.random.default_rng(7)
    N, L, nen = 40, 24, 61
    A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    H = (A + A.conj().T) / 2
    H = 0.9 * H / np.abs(np.linalg.eigvalsh(H)).max()                  # spectrum inside (-1, 1): H is the scaled H~
    va, vb = (rng.standard_normal((2, N, N)) + 1j * rng.standard_normal((2, N, N)))
    r = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    T = chebyshev_of_matrix(H, L)
    # mu(n, m) = [T_m(H) r]^H [v_a T_n(H) v_b r]
    right = np.stack([va @ (Tn @ (vb @ r)) for Tn in T])               # (n, N)
    left = np.stack([Tm @ r for Tm in T])                              # (m, N)
    mu = np.einsum("mk,nk->nm", left.conj(), right)
    emin, emax = -1.0, 1.0
    a, b = O.R.scaling(emin, emax)
    ene = b + a * np.linspace(-0.95, 0.95, nen)
    D = O.basis_table(ene, emin, emax, L)
    J = O.density(D, mu)
    x = (ene - b) / a
    eps, U = np.linalg.eigh(H)
    Te = np.empty((L, N))
    Te[0], Te[1] = 1.0, eps
    for n in range(2, L):
        Te[n] = 2.0 * eps * Te[n - 1] - Te[n - 2]
    K = D @ Te                                                         # K(x_i, eps_alpha)
    rb = U.conj().T @ r                                                # <beta|r>
    Va = U.conj().T @ va @ U                                           # <beta|v_a|alpha>
    cb = U.conj().T @ (vb @ r)                                         # <alpha|v_b r>
    want = np.einsum("b,jb,ba,ia,a->ij", rb.conj(), K, Va, K, cb)
    assert x.size == nen
    err = np.abs(J - want).max() / np.abs(want).max()
    print("eigen-decomposition identity: %.1e of max|J|" % err)
    assert err <= 1e-12


@pytest.mark.parametrize("L,nset,nen,nw,nfermi", O.CASES)
def test_factorised_is_the_formula(L, nset, nen, nw, nfermi):
    d = O.random_diagonals(L, nset, 1000 * L + nen)
    ene = O.inner_mesh(nen, *O.WINDOW)
    fermi = O.case_fermi(ene, nfermi)
    dense = O.optical_dense(d, ene, *O.WINDOW, fermi, nw)
    fact = O.optical_factorised(d, ene, *O.WINDOW, fermi, nw)
    assert dense.shape == fact.shape == (18, nw, nfermi, nset)
    assert np.abs(dense).max() > 0
    err = O.orbital_err(fact, dense)
    print("factorised against dense: %.1e" % err)
    assert err <= 1e-13


def test_factorised_is_the_formula_at_finite_temperature_and_past_the_band():
    d = O.random_diagonals(17, 2, 3)
    ene = np.linspace(-0.75, 0.75, 70)                                 # the last points have |x| >= 1: rows of zeros
    x = O.scaled_axis(ene, *O.WINDOW)[0]
    assert (np.abs(x) >= 1).any() and (np.abs(x) < 1).sum() > 40
    a = O.R.scaling(*O.WINDOW)[0]
    T = 3 * (ene[1] - ene[0]) / 0.633362019e-5                         # kT = 3 steps of the mesh
    fermi = [0.01, ene[20]]
    dense = O.optical_dense(d, ene, *O.WINDOW, fermi, 50, T)
    fact = O.optical_factorised(d, ene, *O.WINDOW, fermi, 50, T)
    F = O.fermi_table(ene, *O.WINDOW, fermi, T)
    assert ((F > 1e-3) & (F < 1 - 1e-3)).sum() > 10 and a > 0          # the levels are really smeared
    assert O.orbital_err(fact, dense) <= 1e-13


def test_fermi_levels_do_not_see_each_other():
    d = O.random_diagonals(24, 2, 11)
    ene = O.inner_mesh(61, *O.WINDOW)
    f2 = np.array([0.5 * (ene[30] + ene[31]), ene[12]])
    for fn in (O.optical_dense, O.optical_factorised):
        both = fn(d, ene, *O.WINDOW, f2, 40)
        for f in range(2):
            one = fn(d, ene, *O.WINDOW, f2[f:f + 1], 40)
            assert np.array_equal(both[:, :, f], one[:, :, 0])


def test_zero_temperature_takes_only_pairs_across_the_fermi_level():
    L, nen, nw = 24, 61, 60
    d = O.random_diagonals(L, 1, 5)
    ene = O.inner_mesh(nen, *O.WINDOW)
    x, a, b = O.scaled_axis(ene, *O.WINDOW)
    fermi = np.array([0.5 * (ene[25] + ene[26])])
    xf = (fermi[0] - b) / a
    F = O.fermi_table(ene, *O.WINDOW, fermi)
    assert set(np.unique(F)) == {0.0, 1.0}
    D = O.basis_table(ene, *O.WINDOW, L)
    across = (x[:, None] <= xf) & (xf < x[None, :])                    # x_i <= x_F < x_j
    want = O.optical_dense(d, ene, *O.WINDOW, fermi, nw)
    for l in (0, 7, 17):
        J = O.density(D, d[l, :, :, 0])
        kept = O.frequency_sum(np.where(across, J, 0.0), F, nw, a)
        assert np.array_equal(kept, want[l, :, :, 0])
        only_w = np.array([[np.pi / a ** 2 / k * np.diagonal(np.where(across, J, 0.0), offset=k).sum()] for k in range(1, nw + 1)])
        assert np.abs(only_w - want[l, :, :, 0]).max() <= 1e-13 * np.abs(want[l]).max()      # weight 1 on every kept term
