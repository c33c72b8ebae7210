"""Every form of the block-Lanczos post-hop pass (rsrec.hip, run_block_lanczos) at the group counts where it can go wrong:
  oop      k_mfma_orth3 writing u_{n+1} into a third vector (the default: orth3 = 1, orth_oop = 1),
  inplace  k_mfma_orth3 writing over u_{n-1} (orth_oop = 0: another vector count, another buffer rotation),
  lds      k_mfma_orth3w (orth3 = 2: tables in LDS, two waves per SIMD, a two-tile pipeline).
For every case and form: finite results, within RTOL of the CPU oracle, a_b(:,:,lld) exactly zero -- and ALL THREE FORMS THE SAME BITS: they do
the same MFMAs in the same order (T1, T2, T3 per tile; tiles in walk order per wave; the same Gram accumulators and the same sums over the waves)
and differ only in where the tables live and where the rows are stored.

The lattices are those of tests/piece_lattices.py (conditions: tests/test_piece_lattices.py), the random ragged lattices of
tests/test_gpu_spmm_random.py and the prescribed chains of tests/test_gpu_prescribed_chain.py.  Also here: s5_spin_xcd (placement only: same
bits) and sat_pct (another list of atoms: another summation order, so held to the oracle, not to bits)."""
import numpy as np
import pytest

import eig18_cases as EC
import piece_lattices as PL
from helpers import RTOL, objects_from, rel_err
from rslmtoasa_amd.recursion import Recursion

pytestmark = pytest.mark.gpu

FORMS = {"oop": {"orth3": 1, "orth_oop": 1}, "inplace": {"orth3": 1, "orth_oop": 0}, "lds": {"orth3": 2}}
CI = {"kernels": 2, "spmm5": 2}


@pytest.fixture(scope="module")
def oracle_of(oracle_lib):
    """label -> oracle (a_b, b2_b) of a problem's chains, computed once per module and left unchanged."""
    cache = {}

    def get(label, p, seeds, lld):
        if label not in cache:
            a_o, b_o = oracle_lib.Oracle(p).block_lanczos(np.asarray(seeds, np.int32), lld)
            a_o.setflags(write=False)
            b_o.setflags(write=False)
            cache[label] = (a_o, b_o)
        return cache[label]
    return get


def run_forms(p, seeds, lld, options, emin=PL.EMIN, emax=PL.EMAX, forms=FORMS, refresh=False):
    """recur_b once per form, each on a handle of its own: {form: (a_b, b2_b, timing)}."""
    out = {}
    for form, fopts in forms.items():
        rec = Recursion(*objects_from(p, seeds, lld, emin=emin, emax=emax), device=0)
        for k, v in dict(options, **fopts).items():
            rec.set_option(k, v)
        if refresh:
            rec.update_hamiltonian()           # options that shape the operator tables apply from the next hand-over
        rec.recur_b()
        out[form] = (rec.a_b.copy(), rec.b2_b.copy(), rec.timing())
        rec.close()
    return out


def check_forms(res, oracle, lld, what):
    a_o, b_o = oracle
    for form, (a, b, _) in res.items():
        assert np.isfinite(a).all() and np.isfinite(b).all(), (what, form)
        ea, eb = rel_err(a, a_o), rel_err(b, b_o)
        print("%s %-7s a_b %.1e b2_b %.1e" % (what, form, ea, eb))
        assert ea < RTOL and eb < RTOL, (what, form, ea, eb)
        assert not a[:, :, lld - 1, :].any(), (what, form)
        assert np.abs(a[:, :, :lld - 1, :]).max() > 0
    first = next(iter(res))
    for form in res:
        assert np.array_equal(res[form][0], res[first][0]) and np.array_equal(res[form][1], res[first][1]), (what, first, form)


# ---- 1. one-piece lattices: 1 partial group .. 138 groups -------------------------------------------------------------------------
ONE_PIECE = [(kk, hoh, lld) for kk in PL.ONE_PIECE_KK for hoh in (False, True) for lld in PL.one_piece_llds(kk, hoh)]


@pytest.mark.parametrize("kk,hoh,lld", ONE_PIECE)
def test_forms_on_one_piece_lattices(kk, hoh, lld, oracle_of):
    p, seeds = PL.one_piece_problem(kk, hoh), PL.one_piece_seeds(kk)
    res = run_forms(p, seeds, lld, CI)
    check_forms(res, oracle_of(("piece", kk, hoh, lld), p, seeds, lld), lld, "piece %d hoh %d lld %d" % (kk, hoh, lld))


# ---- 2. random ragged lattices: several types, impurity atoms, spin-mixing, hoh; both settings of the fragment tables' ci flag ----------
def ragged_cases():
    from test_gpu_spmm_random import RECUR_CASES
    return RECUR_CASES


@pytest.mark.parametrize("spmm5", [1, 2])
@pytest.mark.parametrize("kk,nslots,ntype,nmax,hoh,collinear", ragged_cases())
def test_forms_on_random_ragged_lattices(kk, nslots, ntype, nmax, hoh, collinear, spmm5, oracle_of):
    from test_gpu_spmm_random import random_problem
    p = random_problem(np.random.default_rng(77 + kk + nslots), kk, nslots, ntype, nmax, hoh, collinear)
    seeds, lld = np.array([1, kk // 2, kk], np.int32), 6
    res = run_forms(p, seeds, lld, {"kernels": 2, "spmm5": spmm5})
    check_forms(res, oracle_of(("ragged", kk, nslots), p, seeds, lld), lld, "ragged %d/%d spmm5 %d" % (kk, nslots, spmm5))


# ---- 3. Hermitian rings: the Gram fold of the SpMM epilogue feeds k_reduce_a_u in front of each form --------------------------------
@pytest.mark.parametrize("name", sorted(PL.HERMITIAN_CASES))
def test_forms_behind_the_folded_gram(name, oracle_of):
    p, seeds, lld = PL.hermitian_problem(name), PL.hermitian_seeds(name), PL.HERMITIAN_LLD
    res = run_forms(p, seeds, lld, dict(CI, s5_gram_min=1, s5_queue=2), emin=-6.0, emax=6.0)
    for form, (_, _, t) in res.items():
        assert t["gram_folded_launches"] == lld - 1, (form, t["gram_folded_launches"])
    check_forms(res, oracle_of(("hermitian", name), p, seeds, lld), lld, name)


# ---- 4. prescribed chains: known spectra at every level, for the forms tests/test_gpu_prescribed_chain.py does not reach -----------------
@pytest.mark.parametrize("variant", ["mfma_small", "mfma_ci"])
@pytest.mark.parametrize("kind", ["uniform", "deg3x6"])
def test_forms_on_prescribed_chains(kind, variant, oracle_of):
    from test_gpu_prescribed_chain import CHAIN_BAR, NATOMS, VARIANTS, spectra_of
    p, sig2, E = EC.prescribed_chain(EC.chain_sigmas(kind, NATOMS - 1, 7), 11)
    seeds, lld = np.array([1, NATOMS], np.int32), len(E)
    res = run_forms(p, seeds, lld, VARIANTS[variant], emin=-1.0, emax=1.0)
    check_forms(res, oracle_of(("chain", kind), p, seeds, lld), lld, "chain %s %s" % (kind, variant))
    for form, (a_b, b2_b, _) in res.items():
        for c in range(len(seeds)):
            s2, e = spectra_of(c, sig2, E)
            eb, ea = EC.chain_spectrum_errors(a_b[:, :, :, c], b2_b[:, :, :, c], s2, e)
            print("chain %s %s %s seed %d: eig(b2_b) %.3g, eig(a_b) %.3g" % (kind, variant, form, seeds[c], eb.max(), ea.max()))
            assert (eb <= CHAIN_BAR).all() and (ea <= CHAIN_BAR).all(), (form, c)


# ---- 5. workgroup bands: nblk pinned, and one chain count in each of the three default bands ---------------------------------------------
BAND_LATTICES = [(260, PL.one_piece_lld(260))] + [(1100, lld) for lld in PL.one_piece_llds(1100, False)]   # 1100 atoms: 31 workgroups at lld 5, all 35 (two-stage sum) at lld 7


@pytest.mark.parametrize("band", ["nblk4", "nblk16", "nblk128", "chains2", "chains16", "chains32"])
@pytest.mark.parametrize("kk,lld", BAND_LATTICES)
def test_forms_in_every_workgroup_band(kk, lld, band, oracle_of):
    p, all_seeds = PL.one_piece_problem(kk), PL.round_robin_seeds(kk, 32)
    a_o, b_o = oracle_of(("bands", kk, lld), p, all_seeds, lld)
    nchains = int(band[6:]) if band.startswith("chains") else 2
    options = dict(CI, nblk=int(band[4:])) if band.startswith("nblk") else CI
    res = run_forms(p, all_seeds[:nchains], lld, options)
    check_forms(res, (a_o[..., :nchains], b_o[..., :nchains]), lld, "piece %d lld %d %s" % (kk, lld, band))


# ---- s5_spin_xcd: which XCD serves which output spin -- placement, never results ---------------------------------------------------------
def test_spin_by_xcd_placement_changes_no_bit(oracle_of):
    """A collinear operator (a spin-mixing one ignores the option) in the persistent form, the only one that reads it.  The library reports
    nothing that tells the two placements apart, so this holds the option to 'no bit changes, and the answer is the oracle's'; that the
    placement itself changed is not observable from here."""
    kk = 260
    lld = PL.one_piece_lld(kk)
    p, seeds = PL.one_piece_problem(kk), PL.one_piece_seeds(kk)
    plain = {"both": {"s5_spin_xcd": 0}, "by_xcd": {"s5_spin_xcd": 1}}
    res = run_forms(p, seeds, lld, dict(CI, s5_queue=2), forms=plain, refresh=True)
    check_forms(res, oracle_of(("piece", kk, False, lld), p, seeds, lld), lld, "spin_xcd piece %d" % kk)


# ---- sat_pct: a chain whose region holds that share of the lattice runs on the list of ALL atoms ------------------------------------------
@pytest.mark.parametrize("sat_pct", [40, 80, 100])
@pytest.mark.parametrize("lattice", ["piece260", "two_pieces"])
def test_saturation_share(lattice, sat_pct, oracle_of):
    """piece260: one piece, every chain ends on the list of all atoms, sooner the lower the share.  two_pieces (200 + 60 atoms): at 40 the chains
    of the larger piece (77 % of the lattice) take the list of all atoms although their region never reaches the other 60 -- the blocks outside a
    region are zero and must stay so --, the chain of the smaller piece never does; at 80 and 100 no chain does."""
    if lattice == "piece260":
        p, seeds, lld = PL.one_piece_problem(260), PL.one_piece_seeds(260), PL.one_piece_lld(260)
        label = ("piece", 260, False, lld)
    else:
        p, seeds, lld = PL.two_piece_problem(), PL.two_piece_seeds(), PL.TWO_PIECE_LLD
        label = ("two_pieces",)
    res = run_forms(p, seeds, lld, dict(CI, sat_pct=sat_pct))
    check_forms(res, oracle_of(label, p, seeds, lld), lld, "%s sat_pct %d" % (lattice, sat_pct))
