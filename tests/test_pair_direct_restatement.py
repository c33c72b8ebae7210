"""The identity rsrec_chebyshev_pairs_direct rests on, on the CPU: the four moment sets chebyshev_recur_ij computes per pair
(recursion.f90:2376-2487) are combinations of M_ij(n) = <i|T_n(H~)|j> and M_ji(n), and M_ji(n) is the block at atom j of the Chebyshev
vector started at atom i.  The dense numpy restatement (pair_direct_reference.py) against the compiled reference's moments."""
import numpy as np

from helpers import RTOL
from pair_direct_reference import consumer_sensitivity, fixture_dense, gij_gji, pair_scale


def test_both_form_reproduces_the_reference_slots():
    g, (mu, m_pair), _ = fixture_dense()
    ref = g["mu_n"]
    assert mu.shape == ref.shape and [tuple(p) for p in g["pairs"]] == [(1, 2), (7, 7), (5, 40)]
    for q in range(3):                                           # slot by slot, the (7,7) pair with M_ii / 2 in all four
        for r in range(4):
            err = np.abs(mu[..., 4 * q + r] - ref[..., 4 * q + r]).max() / pair_scale(ref, q)
            print("pair %d slot %d: %.2e" % (q, r, err))
            assert err <= RTOL, (q, r, err)
    # M_ij = M_ji^H to the Hermiticity of the fixture's H
    for q in range(3):
        assert np.abs(m_pair[:, :, :, 0, q] - np.conj(m_pair[:, :, :, 1, q].transpose(1, 0, 2))).max() <= 1e-11


def test_both_form_reproduces_the_reference_slots_with_hoh():
    g, (mu, _), (mu_c, _) = fixture_dense("sc_4x4x8_cheb_ij_hoh")
    ref = g["mu_n"]
    for q in range(len(g["pairs"])):
        err = np.abs(mu[..., 4 * q:4 * q + 4] - ref[..., 4 * q:4 * q + 4]).max() / pair_scale(ref, q)
        print("pair %d: %.2e" % (q, err))
        assert err <= RTOL, (q, err)
        for mine, want in zip(gij_gji(mu_c, q), gij_gji(ref, q)):
            assert np.abs(mine - want).max() / pair_scale(ref, q) <= RTOL, q


def test_cancelling_form_reproduces_the_reference_combinations():
    g, (mu_b, _), (mu, m_pair) = fixture_dense()
    ref = g["mu_n"]
    for q, (i, j) in enumerate(g["pairs"]):
        if i == j:
            assert np.array_equal(mu[..., 4 * q:4 * q + 4], mu_b[..., 4 * q:4 * q + 4])
            continue
        for mine, want, direct in zip(gij_gji(mu, q), gij_gji(ref, q), (m_pair[:, :, :, 0, q], m_pair[:, :, :, 1, q])):
            err = np.abs(mine - want).max() / pair_scale(ref, q)
            print("pair %d: %.2e" % (q, err))
            assert err <= RTOL, (q, err)
            assert np.abs(direct - want).max() / pair_scale(ref, q) <= RTOL
        assert np.array_equal(mu[..., 4 * q + 1], -mu[..., 4 * q]) and np.array_equal(mu[..., 4 * q + 3], -mu[..., 4 * q + 2])


def test_orders_before_first_contact_are_exact_zeros():
    g, (_, m_both), (mu, m_pair) = fixture_dense()
    q = 2                                                        # (5, 40): three hops apart
    assert np.all(m_pair[:, :, :3, :, q] == 0) and np.all(m_both[:, :, :3, :, q] == 0) and np.all(mu[:, :, :3, 4 * q:4 * q + 4] == 0)
    assert np.abs(m_pair[:, :, 3, :, q]).max() > 0


def test_consumer_sensitivity_of_the_exchange_values(oracle_lib):
    """The figure the GPU comparison of the consumers' values between the two routes is judged on (10 x this): moments right to 1e-12
    move xc / fo / parts of exchange_cheb.npz by this fraction of the call's largest value."""
    s = consumer_sensitivity()
    print("largest deviation of xc / fo / parts over the call's largest value: %.2e" % s)
    assert 0.0 < s < 1e-6
