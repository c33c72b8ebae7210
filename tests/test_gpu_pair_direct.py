"""rsrec_chebyshev_pairs_direct (kernels_fan.hpp): the pair moments of chebyshev_recur_ij from one Chebyshev chain per atom.

References: the compiled reference's four-chain moments (tests/golden/sc_4x4x8_cheb_ij*.npz), the library's own four-chain call on a
multi-class cluster, the dense numpy restatement (pair_direct_reference.py) on a ragged lattice, and the consumers' values of the
four-chain route.  Tolerances: helpers.RTOL (1e-10) of a pair's largest slot magnitude for moments; for the consumers' values 10 x the
deviation the CPU restatement measures on exchange_cheb.npz (pair_direct_reference.consumer_sensitivity: 1.5e-13 of the call's largest
value when this was written), because the summation order on the device differs."""
import ctypes as C

import numpy as np
import pytest

from helpers import RTOL, load_golden, objects_from, problem_dict, supercell_problem
from pair_cases import mesh, pair_list, random_contour_dmat, random_tmat
from pair_direct_reference import consumer_sensitivity, dense_h, gij_gji, pair_moments, pair_scale
from rslmtoasa_amd import _lib
from rslmtoasa_amd.exchange import Exchange, exchange_dpar, gauss_legendre
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.recursion import Recursion, chebyshev_scaling

pytestmark = pytest.mark.gpu

KERNEL_SETS = [1, 2]            # VALU kernels on the reference's layout; matrix-core kernels (k_spmm5 on CI vectors)


def recursion(p, pairs, lld, emin, emax, kernels=None):
    ham, lat, ctl, en = objects_from(p, [1], lld, emin=emin, emax=emax)
    lat.ijpair = np.asarray(pairs, np.int32).reshape(-1, 2)
    rec = Recursion(ham, lat, ctl, en, device=0)
    if kernels is not None:
        rec.set_option("kernels", kernels)
    return rec


def direct(rec, both_ends):
    """(mu (18,18,nmom,4 npairs), m_pair) of one direct call, copies."""
    m_pair = rec.chebyshev_recur_ij_direct(both_ends=both_ends)
    return rec.mu_n[:, :, :, :4 * len(rec.lattice.ijpair)].copy(), m_pair


def slot_errors(mu, ref):
    return [np.abs(mu[..., 4 * q:4 * q + 4] - ref[..., 4 * q:4 * q + 4]).max() / pair_scale(ref, q) for q in range(ref.shape[3] // 4)]


def combination_errors(mu, m_pair, ref, pairs):
    """gij / gji formed from the slots, and m_pair itself, against the combinations of the reference's slots; i == j pairs slot by slot."""
    out = []
    for q, (i, j) in enumerate(pairs):
        if i == j:
            out.append(np.abs(mu[..., 4 * q:4 * q + 4] - ref[..., 4 * q:4 * q + 4]).max() / pair_scale(ref, q))
            continue
        e = 0.0
        for k, (mine, want) in enumerate(zip(gij_gji(mu, q), gij_gji(ref, q))):
            e = max(e, np.abs(mine - want).max(), np.abs(m_pair[:, :, :, k, q] - want).max())
        out.append(e / pair_scale(ref, q))
    return out


@pytest.mark.parametrize("kernels", KERNEL_SETS)
@pytest.mark.parametrize("name", ["sc_4x4x8_cheb_ij", "sc_4x4x8_cheb_ij_hoh"])
def test_fixture_parity(name, kernels):
    g = load_golden(name)
    p = supercell_problem(g["dims"], hoh=bool(g["hoh"]))
    rec = recursion(p, g["pairs"], int(g["lld"]), float(g["emin"]), float(g["emax"]), kernels)
    ref = g["mu_n"]
    mu_b, mp_b = direct(rec, True)
    eb = slot_errors(mu_b, ref)
    mu_c, mp_c = direct(rec, False)
    ec = combination_errors(mu_c, mp_c, ref, g["pairs"])
    print(name, kernels, "both: slots", eb, "first-atom mode: combinations", ec)
    assert max(eb) <= RTOL and max(ec) <= RTOL
    assert max(combination_errors(mu_b, mp_b, ref, g["pairs"])) <= RTOL
    # the two modes agree with each other
    for q in range(len(g["pairs"])):
        for k in range(2):
            assert np.abs(mp_b[:, :, :, k, q] - mp_c[:, :, :, k, q]).max() <= RTOL * pair_scale(ref, q), (q, k)
        assert np.array_equal(mu_c[..., 4 * q + 1], -mu_c[..., 4 * q]) or g["pairs"][q][0] == g["pairs"][q][1]
        assert np.array_equal(mu_c[..., 4 * q + 3], -mu_c[..., 4 * q + 2]) or g["pairs"][q][0] == g["pairs"][q][1]
    # orders before the first contact of a distant pair: exact zeros, in m_pair and in all four slots of the first-atom mode
    for q, (i, j) in enumerate(g["pairs"]):
        if (i, j) == (5, 40):
            first = 2 if g["hoh"] else 3                        # three hops apart; with hoh an application reaches two hops
            assert np.all(mp_c[:, :, :first, :, q] == 0) and np.all(mp_b[:, :, :first, :, q] == 0) and np.all(mu_c[:, :, :first, 4 * q:4 * q + 4] == 0)
            assert np.abs(mp_c[:, :, first, :, q]).max() > 0
    rec.close()


def awkward_pairs(kk, seed):
    """pair_list's pairs (the first an i == j pair) plus: a reversed pair beside its original, a duplicated pair, an i == j pair in the
    middle, and a pair whose first atom occurs elsewhere only as a second atom."""
    base = [tuple(int(v) for v in p) for p in pair_list(kk, 4, np.random.default_rng(seed))]
    i, j = next(p for p in base if p[0] != p[1])
    lone = next(a for a in range(kk, 0, -1) if all(a not in p for p in base))
    pairs = base[:2] + [(j, i), (3, 3)] + base[2:] + [(i, j), (2, lone), (lone, 4)]
    assert [p for p in pairs if p[0] == lone] == [(lone, 4)] and sum(p[1] == lone for p in pairs) == 1
    return np.array(pairs, np.int32)


@pytest.mark.parametrize("kernels", KERNEL_SETS)
def test_multi_class_cluster_against_the_four_chain_call(kernels):
    """B2FeCo: three atom types and 15 atoms with their own operator blocks; the pairs lie in and around that region."""
    g = load_golden("B2FeCo_block")
    pairs = awkward_pairs(40, 5)
    rec = recursion(problem_dict(g), pairs, 6, float(g["emin"]), float(g["emax"]), kernels)
    rec.chebyshev_recur_ij()
    ref = rec.mu_n.copy()
    mu_b, mp_b = direct(rec, True)
    mu_c, mp_c = direct(rec, False)
    eb, ec = slot_errors(mu_b, ref), combination_errors(mu_c, mp_c, ref, pairs)
    print(kernels, pairs.tolist(), "both", eb, "first-atom mode", ec)
    assert max(eb) <= RTOL and max(ec) <= RTOL
    assert min(pair_scale(ref, q) for q in range(len(pairs))) > 0
    # a duplicated pair carries the same bits twice
    first_of = {tuple(pairs[q]): q for q in reversed(range(len(pairs)))}
    for q in range(len(pairs)):
        f = first_of[tuple(pairs[q])]
        assert np.array_equal(mu_c[..., 4 * q:4 * q + 4], mu_c[..., 4 * f:4 * f + 4]) and np.array_equal(mu_b[..., 4 * q:4 * q + 4], mu_b[..., 4 * f:4 * f + 4])
    assert len(first_of) < len(pairs)
    rec.close()


@pytest.mark.parametrize("kernels", KERNEL_SETS)
def test_ragged_lattice(kernels):
    """fuzz_seed_1766: a ragged lattice of two atom types with hoh.  Its random operator is NOT Hermitian, so the four-chain call's
    doubled moments (mu_{2n+1} = 2 psi_n^H psi_n - mu_1) are no moments of T_n beyond the first two: the four-chain call pins moments 1 and
    2 of the `both` form, and every order of both forms is held to the dense restatement of the same operator."""
    z = load_golden("fuzz_seed_1766")
    p = problem_dict(z)
    pairs = awkward_pairs(int(z["kk"]), 9)
    lld, emin, emax = 5, -4.0, 4.0
    rec = recursion(p, pairs, lld, emin, emax, kernels)
    rec.chebyshev_recur_ij()
    four = rec.mu_n.copy()
    mu_b, mp_b = direct(rec, True)
    mu_c, mp_c = direct(rec, False)
    a, b = chebyshev_scaling(emin, emax)
    H = dense_h(p)
    for both, mu, mp in ((True, mu_b, mp_b), (False, mu_c, mp_c)):
        ref_mu, ref_mp = pair_moments(H, a, b, pairs, lld, both)
        for q in range(len(pairs)):
            scale = max(pair_scale(ref_mu, q), np.abs(ref_mp[..., q]).max())
            if scale == 0:                                      # a pair the region never joins
                assert np.all(mu[..., 4 * q:4 * q + 4] == 0) and np.all(mp[..., q] == 0)
                continue
            err = max(np.abs(mu[..., 4 * q:4 * q + 4] - ref_mu[..., 4 * q:4 * q + 4]).max(), np.abs(mp[..., q] - ref_mp[..., q]).max()) / scale
            print(kernels, both, tuple(pairs[q]), "%.2e" % err)
            assert err <= RTOL, (both, q, err)
            # exact zeros in the orders at which the dense product has not reached the block
            assert np.array_equal(np.abs(mp[..., q]).max(axis=(0, 1)) == 0, np.abs(ref_mp[..., q]).max(axis=(0, 1)) == 0)
    for q in range(len(pairs)):
        scale = pair_scale(four[:, :, :2], q)
        assert np.abs(mu_b[:, :, :2, 4 * q:4 * q + 4] - four[:, :, :2, 4 * q:4 * q + 4]).max() <= RTOL * scale, q
    # M_ji comes from the same chain in both modes
    assert np.array_equal(mp_b[:, :, :, 1, :], mp_c[:, :, :, 1, :])
    rec.close()


def fixture_case(kernels=None, pairs=None, lld=12):
    g = load_golden("sc_4x4x8_cheb_ij")
    pairs = g["pairs"] if pairs is None else pairs
    return recursion(supercell_problem(g["dims"]), pairs, lld, float(g["emin"]), float(g["emax"]), kernels), np.asarray(pairs, np.int32)


@pytest.mark.parametrize("both_ends", [False, True])
def test_stale_work_buffers_do_not_show(both_ends):
    """A block-Lanczos call and a four-chain call first on the same handle: the direct call then gives the bits of a fresh handle."""
    pairs = np.array([(1, 2), (7, 7), (5, 40), (40, 9)], np.int32)
    rec, _ = fixture_case(pairs=pairs, lld=6)
    fresh = direct(rec, both_ends)
    rec.close()
    rec, _ = fixture_case(pairs=pairs, lld=6)
    rec.recur_b_ij()
    rec.chebyshev_recur_ij()
    used = direct(rec, both_ends)
    assert np.array_equal(fresh[0], used[0]) and np.array_equal(fresh[1], used[1]) and np.abs(fresh[0]).max() > 0
    rec.close()


@pytest.mark.parametrize("kernels", KERNEL_SETS)
@pytest.mark.parametrize("both_ends", [False, True])
def test_determinism_and_independence(both_ends, kernels):
    pairs = np.array([(1, 2), (7, 7), (5, 40), (40, 9), (9, 1), (2, 1)], np.int32)
    rec, _ = fixture_case(kernels, pairs, lld=6)
    mu, mp = direct(rec, both_ends)
    t = rec.timing()
    assert t["hop_launches"] == 2 * 6 + 1 and t["total_ms"] > 0 and t["hop_ms"] > 0      # one batch: one H|psi> launch per application
    mu2, mp2 = direct(rec, both_ends)
    assert np.array_equal(mu, mu2) and np.array_equal(mp, mp2)
    # one chain at a time (at least 3 sources)
    rec.set_option("batch", 1)
    mu1, mp1 = direct(rec, both_ends)
    assert np.array_equal(mu, mu1) and np.array_equal(mp, mp1)
    rec.set_option("batch", 0)
    # every pair alone
    for q in range(len(pairs)):
        rec.lattice.ijpair = pairs[q:q + 1]
        mq, mpq = direct(rec, both_ends)
        assert np.array_equal(mq, mu[..., 4 * q:4 * q + 4]) and np.array_equal(mpq[..., 0], mp[..., q]), q
    rec.close()


def test_pack_moments_reads_the_resident_image():
    rec, pairs = fixture_case(lld=6)
    mu, _ = direct(rec, False)
    n = 4 * len(pairs)
    img = np.full((18, 18, 14, n + 3), 7.0 + 0j, order="F")
    rec.pack_moments(2, n + 3, img)
    assert np.array_equal(img[..., 2:2 + n], mu) and np.all(img[..., :2] == 0) and np.all(img[..., 2 + n:] == 0)
    rec.close()


def consumers(rec, ene, nv1, dpar, tmat, dmat, x, w, **kw):
    ex = Exchange(rec, Green(rec, ene))
    return (ex.compute(-0.0517, nv1, dpar, kind="chebyshev", integrand=True, cumulative=True, **kw)
            + ex.damping(tmat, 61, kind="chebyshev", rows=True, **kw) + ex.contour(x, w, float(ene[50]), dmat, kind="chebyshev", rows=True, **kw))


@pytest.mark.parametrize("both_ends", [False, True])
def test_consumers_behind_the_direct_call(both_ends, oracle_lib):
    """Exchange, damping and contour on the resident image are bitwise what they give on the returned array, and agree with the
    four-chain route's values to 10 x the CPU-measured sensitivity, every pair judged on the largest |value| of the call."""
    rec, pairs = fixture_case()
    ene, nv1 = mesh(100, fermi=-0.0517)
    c = np.array([[[-0.02, 0.05], [0.31, 0.36], [-0.12, 0.01]]])
    dele = np.array([[[0.21, 0.20], [0.12, 0.11], [0.045, 0.052]]])
    dpar = exchange_dpar(c, dele, np.array([0.013]), np.ones(128, np.int32), pairs)
    tmat, dmat = random_tmat(len(pairs)), random_contour_dmat(len(pairs))
    x, w = gauss_legendre(8)
    rec.chebyshev_recur_ij()
    four = consumers(rec, ene, nv1, dpar, tmat, dmat, x, w, resident=True)
    mu, _ = direct(rec, both_ends)
    resident = consumers(rec, ene, nv1, dpar, tmat, dmat, x, w, resident=True)
    mu_after, _ = direct(rec, both_ends)                        # (the consumers left the image alone; a second call restores it anyway)
    from_array = consumers(rec, ene, nv1, dpar, tmat, dmat, x, w, coef=(mu,))
    assert np.array_equal(mu, mu_after)
    bound = 10.0 * consumer_sensitivity()
    assert len(four) == len(resident) == len(from_array) == 11
    for k, (f, r, h) in enumerate(zip(four, resident, from_array)):
        assert np.array_equal(r, h), k
        dev = np.abs(r - f).max() / max(np.abs(f).max(), 1e-300)
        print("both_ends %s output %d: deviation / largest value of the call %.2e (bound %.2e)" % (both_ends, k, dev, bound))
        assert dev <= bound, (k, dev, bound)
    assert all(np.abs(four[k]).max() > 0 for k in (0, 5, 8, 10))
    rec.close()


def test_errors_leave_the_handle_usable():
    rec, pairs = fixture_case(lld=6)
    good, _ = direct(rec, False)
    L, h = rec._L, rec._h
    a, b = chebyshev_scaling(rec.en.energy_min, rec.en.energy_max)
    mu = np.zeros((18, 18, 14, 4 * len(pairs)), np.complex128, order="F")
    P = lambda arr: None if arr is None else arr.ctypes.data_as(C.c_void_p)

    def call(pr=pairs, lld=6, a_=a, out=mu, both=0):
        pr = np.ascontiguousarray(pr, np.int32)
        return L.rsrec_chebyshev_pairs_direct(h, len(pr), P(pr), lld, a_, b, both, P(out), None)
    assert call() == 0 and np.array_equal(mu, good)
    for bad in ([(0, 2)], [(1, 129)], [(129, 1)], [(1, 2), (3, 0)]):
        assert call(pr=np.array(bad, np.int32)) == _lib.ERR_ARG, bad
        assert call(pr=np.array(bad, np.int32), both=1) == _lib.ERR_ARG, bad
    assert call(lld=0) == _lib.ERR_ARG
    assert call(a_=0.0) == _lib.ERR_ARG
    assert call(out=None) == _lib.ERR_ARG
    assert L.rsrec_chebyshev_pairs_direct(h, 0, None, 6, a, b, 0, None, None) == 0          # npairs = 0
    mu[:] = 0
    assert call() == 0 and np.array_equal(mu, good)              # the handle still works
    rec.close()


@pytest.mark.parametrize("both_ends", [False, True])
def test_a_window_too_narrow_diverges(both_ends):
    g = load_golden("sc_4x4x8_cheb_ij")
    rec = recursion(supercell_problem(g["dims"]), g["pairs"], 12, -0.3, 0.3)
    with pytest.raises(_lib.RsrecError) as ei:
        rec.chebyshev_recur_ij_direct(both_ends=both_ends)
    assert ei.value.code == _lib.ERR_DIVERGED
    rec.en.energy_min, rec.en.energy_max = float(g["emin"]), float(g["emax"])
    mu, _ = direct(rec, True)
    assert max(slot_errors(mu, g["mu_n"])) <= RTOL               # the handle still works
    rec.close()
