"""The definition of rsrec_chebyshev_site_map as dense double-precision identities on at most 128 atoms (site_map_reference.site_map), the
weights and seeds of its Python front ends, and the colouring that makes probing exact.  No GPU.

Identities are asserted at 1e-12 of the largest element and the measured value is printed: the sibling restatement tests record 1e-15 to
7e-15 for identities of this kind, and 1e-12 leaves room for the longer sums and no more."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb

from contour_reference import jackson_kernel
from helpers import random_vec_coefficients
from lattice_seed_reference import alloy_case, lattice_moments
from rslmtoasa_amd.lattice import active_region_sizes, supercell_colouring
from rslmtoasa_amd.recursion import chebyshev_fermi_weights, chebyshev_scaling, probing_seeds
from site_map_reference import onsite_function, site_map, worst

TOL = 1e-12


def random_weights(rng, lld, ne):
    return np.asfortranarray(rng.standard_normal((2 * lld + 2, ne)) + 1j * rng.standard_normal((2 * lld + 2, ne)))


def test_one_atom_seeds_give_the_onsite_blocks():
    """Case 1: one vector per atom, coefficient 1: D(:,:,e,j) = sum_n w(n,e) [T_{n-1}(H~)]_jj, and cnorm = 1."""
    dims, p, H, a, b, *_ = alloy_case()
    kk, lld = 128, 2
    w = random_weights(np.random.default_rng(3), lld, 2)
    seeds = np.arange(1, kk + 1, dtype=np.int32)[:, None]
    d_full, d_diag, cnorm = site_map(H, a, b, seeds, np.ones((kk, 1)), lld, w)
    ref = onsite_function(H, a, b, lld, w)
    err = worst(d_full, ref)
    print("one-atom seeds against the on-site blocks: %.2e" % err)
    assert err <= TOL and np.array_equal(cnorm, np.ones(kk))
    assert np.array_equal(d_diag, np.einsum("aaej->aej", d_full))


def test_probing_is_exact_below_the_colour_distance():
    """Case 2: 4x4x8 alloy, stride 4: 64 colours of 2 atoms, at least 4 hops apart (checked by breadth-first search), lld = 1 (degree <= 3):
    D / cnorm equals the on-site blocks for all 128 atoms, with random signs."""
    dims, p, H, a, b, *_ = alloy_case()
    colour = supercell_colouring(dims, 4)
    assert colour.shape == (128,) and sorted(np.bincount(colour)) == [2] * 64
    for c in range(64):
        i, j = np.flatnonzero(colour == c)
        # three hops from i do not reach j: same-coloured atoms are at least 4 hops apart
        reach = np.zeros(129, bool)
        reach[i + 1] = True
        for _ in range(3):
            reach[1:] |= reach[p["nn"][:, 1:int(p["nn"][:, 0].max())]].any(axis=1)
            reach[0] = False
        assert not reach[j + 1], (c, i, j)
        if i == 0:
            assert int(reach.sum()) == active_region_sizes(p["nn"], 1, 3)[-1]             # (the same search as the library's region growth)
    lld = 1
    w = random_weights(np.random.default_rng(5), lld, 3)
    seeds, coefs = probing_seeds(colour, np.random.default_rng(6))
    assert set(np.unique(coefs[seeds > 0].real)) == {-1.0, 1.0}
    d_full, _, cnorm = site_map(H, a, b, seeds, coefs, lld, w)
    ref = onsite_function(H, a, b, lld, w)
    err = worst(d_full / cnorm[None, None, None, :], ref)
    print("exact probing, 64 colours, degree 3: %.2e" % err)
    assert err <= TOL and np.array_equal(cnorm, np.ones(128))


def test_group_sums_are_the_lattice_moments():
    """Case 3: three random-phase vectors, groups by type: sum_{j in g} D(:,:,e,j) = sum_v sum_n w(n,e) M_g^v(n)."""
    dims, p, H, a, b, *_ = alloy_case()
    lld = 3
    rng = np.random.default_rng(8)
    w = random_weights(rng, lld, 2)
    seeds, coefs = random_vec_coefficients(rng.random((128, 3)))
    group = p["iz"].astype(np.int32)
    d_full, _, _ = site_map(H, a, b, seeds, coefs, lld, w)
    m_g = lattice_moments(H, a, b, seeds, coefs, lld, group, 2)             # (18,18,nmom,2,3)
    for g in (1, 2):
        ref = np.einsum("ne,abnv->abe", w, m_g[:, :, :, g - 1, :])
        err = worst(d_full[..., group == g].sum(axis=3), ref)
        print("sum rule, group %d: %.2e" % (g, err))
        assert err <= TOL


def test_fermi_weights_are_the_chebyshev_interpolant():
    """Case 4: against numpy's chebinterpolate of the same function at degree 2 lld + 1 (same coefficients, another algorithm); the
    Jackson columns are the undamped ones times the kernel's damping factors (jackson_kernel folds the doubling of n > 1 in, the
    coefficients carry it already: it is divided out)."""
    lld, emin, emax = 50, -1.1, 0.9
    a, b = chebyshev_scaling(emin, emax)
    fermi, kT, powers = 0.07, 0.1 * a, (0, 1, 2)
    w = chebyshev_fermi_weights(fermi, kT, lld, emin, emax, powers)
    assert w.shape == (2 * lld + 2, 3) and w.flags.f_contiguous and np.all(w.imag == 0)
    for col, q in enumerate(powers):
        ref = npcheb.chebinterpolate(lambda x: (a * x + b) ** q / (1.0 + np.exp((a * x + b - fermi) / kT)), 2 * lld + 1)
        err = np.abs(w[:, col].real - ref).max() / np.abs(ref).max()
        print("fermi weights, power %d: %.2e" % (q, err))
        assert err <= TOL
    g = jackson_kernel(2 * lld + 2)
    g[1:] /= 2.0
    wj = chebyshev_fermi_weights(fermi, kT, lld, emin, emax, powers, jackson=True)
    assert np.abs(wj - w * g[:, None]).max() <= TOL * np.abs(w).max()
    assert chebyshev_fermi_weights(fermi, kT, 4, emin, emax, powers=(0,)).shape == (10, 1)


def test_colouring_probing_seeds_and_cnorm():
    """Case 5: a stride that does not divide is refused; shapes of probing_seeds; cnorm counts the vectors seeding each atom."""
    with pytest.raises(ValueError):
        supercell_colouring((4, 4, 8), 3)
    with pytest.raises(ValueError):
        supercell_colouring((4, 6, 8), 4)
    colour = supercell_colouring((4, 4, 8), 2)
    assert colour.dtype == np.int32 and colour.min() == 0 and colour.max() == 7
    # bcc_supercell's numbering: the first cell index fastest
    assert list(colour[:5]) == [0, 1, 0, 1, 2] and colour[16] == 4
    seeds, coefs = probing_seeds(colour)
    assert seeds.shape == coefs.shape == (8, 128) and seeds.dtype == np.int32 and coefs.dtype == np.complex128
    for c in range(8):
        assert np.array_equal(np.flatnonzero(seeds[c]), np.flatnonzero(colour == c))
        assert np.array_equal(seeds[c][seeds[c] > 0], np.flatnonzero(colour == c) + 1) and np.all(coefs[c][seeds[c] > 0] == 1)
    dims, p, H, a, b, *_ = alloy_case()
    # unit coefficients: atom j is seeded by vector c if colour j = c, and by the two extra vectors if j < 10 or j is even
    extra = np.zeros((2, 128), np.int32)
    extra[0, :10] = np.arange(1, 11)
    extra[1, ::2] = np.arange(1, 129, 2)
    all_seeds = np.concatenate([seeds, extra])
    all_coefs = np.concatenate([coefs, (extra > 0).astype(np.complex128)])
    _, _, cnorm = site_map(H, a, b, all_seeds, all_coefs, 1, np.ones((4, 1)))
    want = 1.0 + (np.arange(128) < 10) + (np.arange(128) % 2 == 0)
    assert np.array_equal(cnorm, want)
