"""The identity rsrec_chebyshev_bloch rests on, on the CPU: the lattice Fourier sum of the Chebyshev vector started at atom i,
S_i(k, n) = sum_j exp(-i k.(r_j - r_i)) <j|T_n(H~)|i>, is T_n of the 18x18 H~(k) on a periodic one-atom cell at supercell-commensurate k.
The dense restatement (bloch_reference.bloch_sums) against the oracle that never forms a chain (bloch_hamiltonian_moments).
Bound: 1e-12 of max|T_n| (measured 5.5e-15 at 14 moments, 8.2e-14 at 102 moments, worst case)."""
import numpy as np
import pytest

from bloch_reference import bloch_hamiltonian_moments, bloch_sums, commensurate_k, fixture_case, stencil_column

K_TRIPLES = [(0, 0, 0), (1, 0, 0), (1, 2, 3), (3, 1, 7), (2, 2, 4)]
SOURCE = 37


@pytest.mark.parametrize("hoh", [False, True])
def test_restatement_against_the_bloch_hamiltonian(hoh):
    dims, _, H, a, b, lld, _, _, cr, cell = fixture_case(hoh)
    assert lld == 12
    k = commensurate_k(dims, K_TRIPLES)
    s = bloch_sums(H, a, b, [SOURCE], lld, cr, cell, k)[..., 0, 0]
    t = bloch_hamiltonian_moments(H, a, b, SOURCE, lld, cr, cell, k)
    err = np.abs(s - t).max() / np.abs(t).max()
    print("hoh %s: %.2e of max|T_n| = %.3f" % (hoh, err, np.abs(t).max()))
    assert err <= 1e-12
    assert np.array_equal(s[:, :, 0, :], np.repeat(np.eye(18)[:, :, None], len(K_TRIPLES), axis=2))


@pytest.mark.parametrize("hoh", [False, True])
def test_group_sums_add_up(hoh):
    dims, _, H, a, b, lld, _, _, cr, cell = fixture_case(hoh)
    k = commensurate_k(dims, K_TRIPLES)
    kk = H.shape[0] // 18
    group = (np.arange(kk) % 3 + 1).astype(np.int32)
    whole = bloch_sums(H, a, b, [SOURCE], lld, cr, cell, k)
    parts = bloch_sums(H, a, b, [SOURCE], lld, cr, cell, k, group, 3)
    assert np.abs(parts.sum(axis=4) - whole[..., 0, :]).max() <= 1e-12 * np.abs(whole).max()
    left_out = group.copy()
    left_out[::5] = 0
    fewer = bloch_sums(H, a, b, [SOURCE], lld, cr, cell, k, left_out, 3)
    assert np.abs(fewer - parts).max() > 1e-3                    # the atoms left out carry weight


@pytest.mark.parametrize("hoh", [False, True])
def test_cell_does_not_matter_for_commensurate_k(hoh):
    dims, _, H, a, b, lld, _, _, cr, cell = fixture_case(hoh)
    k = commensurate_k(dims, K_TRIPLES)
    with_cell = bloch_sums(H, a, b, [SOURCE], lld, cr, cell, k)
    without = bloch_sums(H, a, b, [SOURCE], lld, cr, None, k)
    assert np.abs(with_cell - without).max() <= 1e-12 * np.abs(with_cell).max()


def test_stencil_column_is_the_dense_column():
    """The column the large-cell GPU test builds without a dense matrix."""
    _, p, H, *_ = fixture_case(False)
    for src in (1, SOURCE, 128):
        assert np.array_equal(stencil_column(p, src), H[:, 18 * (src - 1):18 * src].reshape(-1, 18, 18))
