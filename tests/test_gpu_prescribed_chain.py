"""B = S^{1/2} AND B^-1 = S^{-1/2} of the device eigen-solver inside the recursion, against KNOWN answers: recur_b on the chains of
eig18_cases.prescribed_chain, whose hops are P diag(sigma) Q^H, so that in exact arithmetic eig(b2_b[n]) = sigma_n^2 and
eig(a_b[n]) = eig(E_{n+1}).  B^-1 is only ever used to form the next level's vectors: a wrong S^{-1/2} shows in the next A_n and B_n^2.

Three kernel sets, as tests/test_gpu_spmm_random.py runs them: kernels = 1 (k_reduce_b_eig, k_update), kernels = 2 with spmm5 = 1 and
with spmm5 = 2 (k_reduce_b_u and its tables, the orth3 kernels), on lattices of 6 and 3 atoms.

  * well-conditioned, 3 x 6-fold degenerate and all-equal singular values, two chains (seeded at either end of the chain): within RTOL
    of the CPU oracle and within 1e-13 (450 eps) of the prescribed spectra at every level (the oracle alone: <= 42 eps on b2_b,
    <= 29 eps on a_b); a_b[lld - 1] exactly zero;
  * one ill-conditioned level (kappa(B_1^2) = 1e4, 1e8, or one sigma = 1e-4): rounding is amplified by about sqrt(kappa) at that level
    and by kappa per further level IN THE ORACLE TOO, so the bars are 16 x the oracle's own distance to the prescribed spectrum on the
    same input (oracle: eig(b2_b[1]) 6 / 2 / 7.6 eps, eig(a_b[1]) 184 / 1.8e6 / 3.2e5 eps, eig(b2_b[2]) 137 / 1.8e6 / 6.3e5 eps);
  * every kernel set gives the same bits with batch = 1 and with the side stream off.

Measured on an MI355X (the tests print every figure): well-conditioned chains, all kernel sets: eig(b2_b) <= 49 eps, eig(a_b) <= 54 eps.
One ill-conditioned level, device / oracle ratio (kernels 1 | kernels 2 spmm5 1 | kernels 2 spmm5 2):
    kappa 1e4    eig(b2_b[1]) 0.83 | 0.83 | 0.83 (5 eps)   eig(a_b[1]) 0.43 | 0.72 | 0.68 (79 .. 133 eps)     eig(b2_b[2]) 0.99 | 0.87 | 0.86
    kappa 1e8    eig(b2_b[1]) 2.0 | 1.5 | 1.5 (3 .. 4 eps) eig(a_b[1]) 0.39 | 0.73 | 0.72 (0.7 .. 1.3e6 eps)  eig(b2_b[2]) 0.26 | 0.33 | 0.33
    one 1e-4     eig(b2_b[1]) 0.82 | 0.71 | 0.71 (6 eps)   eig(a_b[1]) 0.43 | 1.49 | 1.24 (1.4 .. 4.8e5 eps)  eig(b2_b[2]) 0.42 | 0.85 | 0.85"""
import numpy as np
import pytest

import eig18_cases as EC
from helpers import RTOL, objects_from, rel_err
from rslmtoasa_amd.recursion import Recursion

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
VARIANTS = {"valu": {"kernels": 1, "spmm5": 1}, "mfma_small": {"kernels": 2, "spmm5": 1}, "mfma_ci": {"kernels": 2, "spmm5": 2}}
CHAIN_BAR = 1e-13
NATOMS = 6


@pytest.fixture(scope="module")
def chains(oracle_lib):
    """kind -> (problem, seeds, lld, sigma^2 per level, eig E per atom, oracle a_b, oracle b2_b), built once and left unchanged."""
    cache = {}

    def get(kind):
        if kind not in cache:
            if kind in ("uniform", "deg3x6", "equal"):
                p, sig2, E = EC.prescribed_chain(EC.chain_sigmas(kind, NATOMS - 1, 7), 11)
                seeds = np.array([1, NATOMS], np.int32)
            else:
                p, sig2, E = EC.prescribed_chain(EC.graded_sigmas(kind, 8), 12)
                seeds = np.array([1], np.int32)
            lld = len(E)
            a_o, b_o = oracle_lib.Oracle(p).block_lanczos(seeds, lld)
            a_o.setflags(write=False)
            b_o.setflags(write=False)
            cache[kind] = (p, seeds, lld, sig2, E, a_o, b_o)
        return cache[kind]
    return get


def recursion(p, seeds, lld, variant):
    rec = Recursion(*objects_from(p, seeds, lld), device=0)
    for k, v in VARIANTS[variant].items():
        rec.set_option(k, v)
    return rec


def spectra_of(chain, sig2, E):
    """Chain 0 starts at atom 1, chain 1 at the last atom and meets the hops and atoms in reverse order (T T^H has the spectrum of T^H T)."""
    return (sig2, E) if chain == 0 else (sig2[::-1], E[::-1])


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["uniform", "deg3x6", "equal"])
def test_prescribed_spectra_at_every_level(kind, variant, chains):
    p, seeds, lld, sig2, E, a_o, b_o = chains(kind)
    rec = recursion(p, seeds, lld, variant)
    rec.recur_b()
    a_b, b2_b = rec.a_b.copy(), rec.b2_b.copy()
    assert np.isfinite(a_b).all() and np.isfinite(b2_b).all()
    assert rel_err(a_b, a_o) < RTOL and rel_err(b2_b, b_o) < RTOL
    assert not a_b[:, :, lld - 1, :].any()
    for c in range(len(seeds)):
        s2, e = spectra_of(c, sig2, E)
        eb, ea = EC.chain_spectrum_errors(a_b[:, :, :, c], b2_b[:, :, :, c], s2, e)
        ob, oa = EC.chain_spectrum_errors(a_o[:, :, :, c], b_o[:, :, :, c], s2, e)
        print("chain %-7s %-10s seed %d: eig(b2_b) %s eps (oracle %s), eig(a_b) %s eps (oracle %s)"
              % (kind, variant, seeds[c], np.round(eb / EPS, 1), np.round(ob / EPS, 1), np.round(ea / EPS, 1), np.round(oa / EPS, 1)))
        assert (ob <= CHAIN_BAR).all() and (oa <= CHAIN_BAR).all()
        assert (eb <= CHAIN_BAR).all() and (ea <= CHAIN_BAR).all()
    # scheduling options must not change a bit
    for key, val in (("batch", 1), ("side_stream", 0)):
        rec.set_option(key, val)
        rec.recur_b()
        assert np.array_equal(rec.a_b, a_b) and np.array_equal(rec.b2_b, b2_b), (key, val)
    rec.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["kappa1e4", "kappa1e8", "one_small"])
def test_one_ill_conditioned_level(kind, variant, chains):
    p, seeds, lld, sig2, E, a_o, b_o = chains(kind)
    rec = recursion(p, seeds, lld, variant)
    rec.recur_b()
    a_b, b2_b = rec.a_b.copy(), rec.b2_b.copy()
    assert np.isfinite(a_b).all() and np.isfinite(b2_b).all() and not a_b[:, :, lld - 1, :].any()
    eb, ea = EC.chain_spectrum_errors(a_b[:, :, :, 0], b2_b[:, :, :, 0], sig2, E)
    ob, oa = EC.chain_spectrum_errors(a_o[:, :, :, 0], b_o[:, :, :, 0], sig2, E)
    rows = (("eig(b2_b[1])", eb[0], ob[0]), ("eig(a_b[1])", ea[1], oa[1]), ("eig(b2_b[2])", eb[1], ob[1]))
    for what, dev, orc in rows:
        print("chain %-9s %-10s %-12s device %.3g eps, oracle %.3g eps, ratio %.2f" % (kind, variant, what, dev / EPS, orc / EPS, dev / orc))
    for what, dev, orc in rows:
        assert np.isfinite(orc) and orc > 0
        assert dev <= 16.0 * orc, (what, dev / EPS, orc / EPS)
    assert ea[0] <= CHAIN_BAR                              # A_0 = E_1: nothing ill-conditioned has happened yet
    for key, val in (("batch", 1), ("side_stream", 0)):
        rec.set_option(key, val)
        rec.recur_b()
        assert np.array_equal(rec.a_b, a_b) and np.array_equal(rec.b2_b, b2_b), (key, val)
    rec.close()
