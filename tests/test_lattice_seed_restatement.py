"""The dense restatement of rsrec_chebyshev_lattice (lattice_seed_reference.lattice_moments) against what it has to reduce to (CPU only):
plane-wave seeds give the source average of the Bloch sums, on a one-type cell T_n(H~(k)) itself, and a one-atom seed the chain's own block."""
import numpy as np

from bloch_reference import bloch_hamiltonian_moments, bloch_sums, commensurate_k, fixture_case
from lattice_seed_reference import ALLOY_K, ALLOY_LLD, alloy_case, lattice_moments, plane_wave_seeds
from pair_direct_reference import chain_blocks


def test_plane_wave_seeds_give_the_source_average_of_the_bloch_sums():
    """Two-type random 4x4x8 cell, lld 5, three commensurate k, grouped by type: M_g(n) at k equals the mean over all 128 sources of
    bloch_sums.  Bound: 1e-13 of the largest element -- both sides are sums of 128 x 128 products of magnitude <= 1 in float64."""
    dims, p, H, a, b, _, _, cr, cell = alloy_case(False)
    kk = H.shape[0] // 18
    k = commensurate_k(dims, ALLOY_K)
    group = p["iz"]
    assert kk == 128 and 0 < (group == 1).sum() < kk
    mean = bloch_sums(H, a, b, np.arange(1, kk + 1), ALLOY_LLD, cr, cell, k, group, 2).mean(axis=5)      # (18,18,nmom,nk,2)
    mine = lattice_moments(H, a, b, *plane_wave_seeds(k, cr), ALLOY_LLD, group, 2)                       # (18,18,nmom,2,nk)
    err, scale = np.abs(mine - mean.transpose(0, 1, 2, 4, 3)).max(), np.abs(mean).max()
    print("source average: %.2e at scale %.3f" % (err, scale))
    assert scale > 0.1 and err <= 1e-13 * scale
    # the first moment is the group's share of the identity
    for g in (1, 2):
        assert np.allclose(mine[:, :, 0, g - 1, :], ((group == g).sum() / kk * np.eye(18))[:, :, None], rtol=0, atol=1e-14)


def test_one_type_cell_gives_the_bloch_hamiltonian_moments():
    dims, _, H, a, b, lld, _, _, cr, cell = fixture_case(False)
    k = commensurate_k(dims, ALLOY_K)
    ref = bloch_hamiltonian_moments(H, a, b, 1, 4, cr, cell, k)                                          # (18,18,nmom,nk)
    mine = lattice_moments(H, a, b, *plane_wave_seeds(k, cr), 4)[:, :, :, 0, :]
    err = np.abs(mine - ref).max() / np.abs(ref).max()
    print("T_n(H~(k)): %.2e" % err)
    assert err <= 1e-13


def test_one_atom_seed_gives_the_chains_own_block():
    dims, _, H, a, b, lld, _, _, cr, cell = fixture_case(False)
    ref = chain_blocks(H, a, b, 37, 10)[36]                                                              # (18,18,nmom)
    mine = lattice_moments(H, a, b, [[37, 0]], [[1.0, 5.0]], 4)[:, :, :, 0, 0]
    assert np.abs(mine - ref).max() <= 1e-14 * np.abs(ref).max()
    # a later entry on the same atom overwrites, and the weight is the conjugate of what was placed
    twice = lattice_moments(H, a, b, [[37, 37]], [[3.0, 0.5j]], 4)[:, :, :, 0, 0]
    assert np.abs(twice - 0.25 * ref).max() <= 1e-14 * np.abs(ref).max()
