"""The identity rsrec_chebyshev_bloch_map rests on, on the CPU: everything the Bloch call does is linear, so the energy sum can be taken
before the lattice Fourier sum,
    G_i(k, e) = sum_n w(n, e) S_i(k, n) = sum_j exp(-i k.d(j, i)) Y_e[j],    Y_e = sum_n w(n, e) psi_{n-1}.
The energy-first restatement (bloch_map_reference.bloch_map) against the weights applied to the moments of bloch_reference.bloch_sums and of
the chain-free oracle bloch_hamiltonian_moments, on both 4x4x8 fixtures.  Bounds: 1e-12 of the largest element of the image, that of
tests/test_bloch_restatement.py on the same sums (measured 2.4e-15 / 1.5e-15 against bloch_sums, 1.5e-15 / 2.9e-15 against the oracle,
without / with hoh)."""
import functools

import numpy as np
import pytest

from bloch_map_reference import bloch_map, green_weights, weighted_moments
from bloch_reference import bloch_hamiltonian_moments, bloch_sums, commensurate_k, fixture_case, image_errors
from rslmtoasa_amd.recursion import chebyshev_green_weights

K_TRIPLES = [(0, 0, 0), (2, 0, 0), (1, 2, 3), (3, 1, 7), (2, 2, 4), (1, 1, 1)]
SOURCES = (1, 37)


def energies(emin, emax):
    return np.array([emin + 0.4, 0.5 * (emin + emax), -0.1, emax - 0.4])


@functools.lru_cache(maxsize=None)
def case(hoh):
    dims, _, H, a, b, lld, emin, emax, cr, cell = fixture_case(hoh)
    k = commensurate_k(dims, K_TRIPLES)
    w = green_weights(2 * lld + 2, a, b, energies(emin, emax))
    g = bloch_map(H, a, b, SOURCES, lld, cr, cell, k, w)
    g.setflags(write=False)
    return H, a, b, lld, cr, cell, k, w, g


@pytest.mark.parametrize("hoh", [False, True])
def test_energy_first_against_the_weighted_bloch_sums(hoh):
    H, a, b, lld, cr, cell, k, w, g = case(hoh)
    assert lld == 12 and g.shape == (18, 18, 4, 6, 1, 2)
    ref = weighted_moments(bloch_sums(H, a, b, SOURCES, lld, cr, cell, k), w)
    err = max(max(row) for row in image_errors(g, ref))
    print("hoh %s: energy-first against the weighted Bloch sums %.2e" % (hoh, err))
    assert err <= 1e-12


@pytest.mark.parametrize("hoh", [False, True])
def test_energy_first_against_the_bloch_hamiltonian(hoh):
    H, a, b, lld, cr, cell, k, w, g = case(hoh)
    for s, src in enumerate(SOURCES):
        ref = weighted_moments(bloch_hamiltonian_moments(H, a, b, src, lld, cr, cell, k), w)
        err = np.abs(g[..., 0, s] - ref).max() / np.abs(ref).max()
        print("hoh %s source %d: energy-first against the weights on T_n(H~(k)) %.2e" % (hoh, src, err))
        assert err <= 1e-12


@pytest.mark.parametrize("hoh", [False, True])
def test_spectral_matrix_is_non_negative(hoh):
    """Green weights, the full group: (G - G^H) / (-2 pi i) of every (k, E) has no negative eigenvalue -- the positivity of the Jackson kernel."""
    g = case(hoh)[-1]
    low = np.inf
    for s in range(g.shape[5]):
        for q in range(g.shape[3]):
            for e in range(g.shape[2]):
                G = g[:, :, e, q, 0, s]
                low = min(low, np.linalg.eigvalsh((G - G.conj().T) / (-2j * np.pi)).min())
    print("hoh %s: smallest eigenvalue of the spectral matrix %.2e" % (hoh, low))
    assert low >= 0.0


@pytest.mark.parametrize("hoh", [False, True])
def test_group_images_add_up(hoh):
    H, a, b, lld, cr, cell, k, w, g = case(hoh)
    group = (np.arange(H.shape[0] // 18) % 3 + 1).astype(np.int32)
    parts = bloch_map(H, a, b, SOURCES, lld, cr, cell, k, w, group, 3)
    assert np.abs(parts.sum(axis=4) - g[..., 0, :]).max() <= 1e-12 * np.abs(g).max()
    assert min(np.abs(parts[..., q, :]).max() for q in range(3)) > 0


@pytest.mark.parametrize("hoh", [False, True])
def test_package_weights_are_the_reference_weights(hoh):
    """A few ulps of the largest weight: the same formula written twice (vectorised in the package, element by element here)."""
    _, _, _, a, b, lld, emin, emax, _, _ = fixture_case(hoh)
    ene = energies(emin, emax)
    mine, ref = chebyshev_green_weights(ene, lld, emin, emax), green_weights(2 * lld + 2, a, b, ene)
    assert mine.shape == ref.shape == (2 * lld + 2, 4)
    assert np.abs(mine - ref).max() <= 1e-14 * np.abs(ref).max()
    for bad in (emin, emax, emax + 0.1):
        with pytest.raises(ValueError):
            chebyshev_green_weights([0.0, bad], lld, emin, emax)
