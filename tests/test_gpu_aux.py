"""rsrec_exchange_aux and rsrec_spin_lattice (kernels_auxgreen.hpp) against the numpy restatement of calculate_jij_auxgreen and
calculate_jijk (aux_reference.py, pinned to the compiled reference by test_aux_restatement), fed with g0 from the library's Green kernels."""
import ctypes as C

import numpy as np
import pytest

from pair_cases import (FERMI, TRIOS, aux_reference, chain_g0 as all_g0, check_aux as check, jijk_reference, random_apar,
                        random_trio_dmat as random_dmat, run_device_script, setup)
from rslmtoasa_amd import _lib
from rslmtoasa_amd.exchange import Exchange, trio_pairs

pytestmark = pytest.mark.gpu

PAIRS = np.array([(1, 1), (1, 2), (1, 9), (5, 60), (3, 3)], np.int32)


CASES = [("block", False), ("block", True), ("chebyshev", False)]


@pytest.mark.parametrize("kind,hoh", CASES)
def test_aux_matches_restatement(kind, hoh):
    rec, g, ene, nv1, _ = setup(PAIRS, lld=8, hoh=hoh, channels=100, kind=kind)
    apar = random_apar(len(PAIRS), 2, 21)
    g0 = all_g0(rec, g, kind, 4 * len(PAIRS))
    coef = (rec.a_b, rec.b2_b) if kind == "block" else None
    res = Exchange(rec, g).aux(FERMI, nv1, apar, kind=kind, rows=True, coef=coef)
    check(res, aux_reference(g0, PAIRS, apar, ene, nv1))
    same = PAIRS[:, 0] == PAIRS[:, 1]
    assert not res[0][1:, same].any() and not res[1][1:, :, same].any()          # an i == j pair: J00 in row 0, zeros below
    assert np.abs(res[0][1:, ~same]).max() > 0
    rec.close()


@pytest.mark.parametrize("kind,hoh", CASES)
def test_jijk_matches_restatement(kind, hoh):
    pairs = trio_pairs(TRIOS)
    rec, g, ene, nv1, _ = setup(pairs, lld=8, hoh=hoh, channels=100, kind=kind)
    apar, dmat = random_apar(len(TRIOS), 3, 22), random_dmat(len(TRIOS))
    g0 = all_g0(rec, g, kind, 4 * len(pairs))
    coef = (rec.a_b, rec.b2_b) if kind == "block" else None
    res = Exchange(rec, g).spin_lattice(FERMI, nv1, apar, dmat, kind=kind, rows=True, coef=coef)
    check(res, jijk_reference(g0, TRIOS, apar, dmat, ene, nv1))
    rec.close()


DEVICE_SCRIPT = r"""
from rslmtoasa_amd.exchange import Exchange, trio_pairs
pairs = trio_pairs(T.TRIOS)                          # (1,1) among them: the resident chains are compacted
rec, g, ene, nv1, _ = T.setup(pairs, lld=8, channels=100)
x = Exchange(rec, g)
aa, at, dm = T.random_apar(len(pairs), 2, 31), T.random_apar(len(T.TRIOS), 3, 32), T.random_trio_dmat(len(T.TRIOS))
calls = {"aux": lambda **kw: x.aux(T.FERMI, nv1, aa, rows=True, **kw), "jijk": lambda **kw: x.spin_lattice(T.FERMI, nv1, at, dm, rows=True, **kw)}
first = {k: f(resident=True) for k, f in calls.items()}
again = {k: f(resident=True) for k, f in calls.items()}
rec.zsqr()
a_inf, b_inf, _, _ = g.terminator(nsites=4 * len(pairs))
ta = torch.from_numpy(np.ascontiguousarray(rec.a_b.transpose(3, 2, 1, 0))).cuda()
tb = torch.from_numpy(np.ascontiguousarray(rec.b2_b.transpose(3, 2, 1, 0))).cuda()
for k, f in calls.items():
    for other in (again[k], f(), f(a_inf=a_inf, b_inf=b_inf), f(coef=(ta, tb))):
        for a, b in zip(first[k], other):
            assert np.array_equal(a, b), k
g0 = T.chain_g0(rec, g, "block", 4 * len(pairs), zsqr=False)
T.check_aux(first["aux"], T.aux_reference(g0, pairs, aa, ene, nv1))
T.check_aux(first["jijk"], T.jijk_reference(g0, T.TRIOS, at, dm, ene, nv1))
rec.close()
print("AUX_DEVICE_OK")
"""


def test_coefficient_sources_agree_bitwise():
    """Resident chains (compacted: the trio (1,2,1) holds the pair (1,1)), host arrays with device and with caller terminators, and
    device-pointer coefficients give the same bits; so do two calls.  Own process: torch's HIP runtime has to start before librsrec's."""
    run_device_script(DEVICE_SCRIPT, "sources", "AUX_DEVICE_OK")


def test_a_trio_does_not_depend_on_the_others_or_on_the_split():
    """Every trio alone (its own call: another chunking of the same work) gives the bits it has in the call of all trios, and the
    zero-padded images of a two-rank split (2 trios + 1 trio) sum to the single call.  Likewise the pairs of rsrec_exchange_aux."""
    pairs = trio_pairs(TRIOS)
    rec, g, ene, nv1, _ = setup(pairs, lld=8, channels=100)
    rec.zsqr()
    x = Exchange(rec, g)
    at, dm, aa = random_apar(len(TRIOS), 3, 41), random_dmat(len(TRIOS)), random_apar(len(pairs), 2, 42)
    whole, whole_rows = x.spin_lattice(FERMI, nv1, at, dm, rows=True)
    aux_whole, aux_rows = x.aux(FERMI, nv1, aa, rows=True)
    image = np.zeros_like(whole)
    aux_image = np.zeros_like(aux_whole)
    for n, (t0, t1) in enumerate(((0, 1), (1, 2), (2, 3), (0, 2), (2, 3))):          # every trio alone, then the two ranks of a split
        p0, p1 = 3 * t0, 3 * t1
        rec.lattice.ijpair = pairs[p0:p1]
        coef = (rec.a_b[..., 4 * p0:4 * p1], rec.b2_b[..., 4 * p0:4 * p1])
        part, rows = x.spin_lattice(FERMI, nv1, at[..., t0:t1], dm[..., t0:t1], rows=True, coef=coef, trio_offset=t0, ntrios_total=len(TRIOS))
        assert np.array_equal(rows, whole_rows[..., t0:t1]) and np.array_equal(part[:, t0:t1], whole[:, t0:t1])
        assert not np.delete(part, np.s_[t0:t1], axis=1).any()
        apart, arows = x.aux(FERMI, nv1, aa[..., p0:p1], rows=True, coef=coef, pair_offset=p0, npairs_total=len(pairs))
        assert np.array_equal(arows, aux_rows[..., p0:p1]) and np.array_equal(apart[:, p0:p1], aux_whole[:, p0:p1])
        if n >= 3:
            image += part
            aux_image += apart
    rec.lattice.ijpair = pairs
    assert np.array_equal(image, whole) and np.array_equal(aux_image, aux_whole)
    rec.close()


@pytest.mark.parametrize("cap", ["1", "3", "4", "7"])
def test_chunked_calls_give_the_same_bits(cap, monkeypatch):
    """RSREC_PAIR_CHUNK caps the pairs per chunk, so these small calls run the multi-chunk loop (rsrec_spin_lattice: whole trios, the cap
    rounded down to a multiple of 3 and at least 3; per-chunk staging of apar and dmat): the bits of the one-chunk call."""
    pairs = trio_pairs(TRIOS)
    rec, g, ene, nv1, _ = setup(pairs, lld=8, channels=100)
    x = Exchange(rec, g)
    at, dm, aa = random_apar(len(TRIOS), 3, 81), random_dmat(len(TRIOS)), random_apar(len(pairs), 2, 82)
    one = x.spin_lattice(FERMI, nv1, at, dm, rows=True, resident=True) + x.aux(FERMI, nv1, aa, rows=True, resident=True)
    rec.zsqr()
    one_host = x.spin_lattice(FERMI, nv1, at, dm, rows=True) + x.aux(FERMI, nv1, aa, rows=True)
    monkeypatch.setenv("RSREC_PAIR_CHUNK", cap)
    many = x.spin_lattice(FERMI, nv1, at, dm, rows=True, resident=True) + x.aux(FERMI, nv1, aa, rows=True, resident=True)
    many_host = x.spin_lattice(FERMI, nv1, at, dm, rows=True) + x.aux(FERMI, nv1, aa, rows=True)
    monkeypatch.delenv("RSREC_PAIR_CHUNK")
    for a, b, c, d in zip(one, many, one_host, many_host):
        assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)
    assert np.abs(one[0]).max() > 0 and np.abs(one[2]).max() > 0
    rec.close()


def test_bad_arguments_are_errors():
    pairs = trio_pairs(TRIOS[:1])
    rec, g, ene, nv1, _ = setup(pairs, lld=6, channels=40)
    L, h = rec._L, rec._h
    same = np.zeros(3, np.int32)
    aa, at, dm = random_apar(3, 2, 51), random_apar(1, 3, 52), random_dmat(1)
    ab = np.asfortranarray(rec.a_b[..., :12])
    bb = np.asfortranarray(rec.b2_b[..., :12])
    jaux, jijk = np.zeros((9, 3), order="F"), np.zeros((9, 1), order="F")
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def aux(kind=0, npairs=3, nen=len(ene), ap=aa, out=jaux, same_=same):
        jaux[:] = -7.0
        rc = L.rsrec_exchange_aux(h, kind, npairs, P(same_), 6, nen, P(ene), nv1, FERMI, 0, -0.6, 0.4, None, None, P(ab), P(bb), P(ap), 0, 3, P(out), None)
        assert rc == 0 or np.all(jaux == -7.0)              # nothing ran: the outputs are untouched
        return rc

    def jk(kind=0, npairs=3, nen=len(ene), ap=at, d=dm, out=jijk, same_=same):
        jijk[:] = -7.0
        rc = L.rsrec_spin_lattice(h, kind, npairs, P(same_), 6, nen, P(ene), nv1, FERMI, 0, -0.6, 0.4, None, None, P(ab), P(bb), P(ap), P(d), 0, 1,
                                  P(out), None)
        assert rc == 0 or np.all(jijk == -7.0)
        return rc
    assert aux() == 0 and jk() == 0
    for f in (aux, jk):
        assert f(npairs=0) == _lib.ERR_ARG
        assert f(kind=2) == _lib.ERR_ARG
        assert f(nen=nv1 + 8) == _lib.ERR_ARG
        assert f(ap=None) == _lib.ERR_ARG
        assert f(out=None) == _lib.ERR_ARG
        assert f(same_=None) == _lib.ERR_ARG
    assert jk(npairs=2) == _lib.ERR_ARG                                           # not a multiple of 3
    assert jk(npairs=4) == _lib.ERR_ARG
    assert jk(d=None) == _lib.ERR_ARG
    assert aux() == 0 and jk() == 0                                               # the handle still works
    rec.close()


def test_resident_compacted_chains_refuse_caller_terminators():
    pairs = trio_pairs(TRIOS[2:])                                                 # (1,2), (1,1), (2,1)
    rec, g, ene, nv1, _ = setup(pairs, lld=6, channels=40)
    ai = np.zeros((18, 18, 12), order="F")
    x = Exchange(rec, g)
    for call in (lambda **kw: x.aux(FERMI, nv1, random_apar(3, 2, 61), resident=True, **kw),
                 lambda **kw: x.spin_lattice(FERMI, nv1, random_apar(1, 3, 62), random_dmat(1), resident=True, **kw)):
        with pytest.raises(_lib.RsrecError) as ei:
            call(a_inf=ai, b_inf=ai)
        assert ei.value.code == _lib.ERR_ARG and "terminators" in str(ei.value)
        call()                                                                    # the handle still works, with the device terminator
    rec.close()


@pytest.mark.parametrize("kind", ["block", "chebyshev"])
def test_exchange_is_unchanged_by_the_new_calls(kind):
    """rsrec_exchange after rsrec_exchange_aux and rsrec_spin_lattice on the same handle gives the bits of a handle that never ran them."""
    pairs = trio_pairs(TRIOS)

    def exchange_only():
        rec, g, ene, nv1, dpar = setup(pairs, lld=8, channels=100, kind=kind)
        out = Exchange(rec, g).compute(FERMI, nv1, dpar, kind=kind, resident=True, integrand=True, cumulative=True)
        rec.close()
        return out
    rec, g, ene, nv1, dpar = setup(pairs, lld=8, channels=100, kind=kind)
    x = Exchange(rec, g)
    before = x.compute(FERMI, nv1, dpar, kind=kind, resident=True, integrand=True, cumulative=True)
    x.aux(FERMI, nv1, random_apar(len(pairs), 2, 71), kind=kind, resident=True, rows=True)
    x.spin_lattice(FERMI, nv1, random_apar(len(TRIOS), 3, 72), random_dmat(len(TRIOS)), kind=kind, resident=True, rows=True)
    after = x.compute(FERMI, nv1, dpar, kind=kind, resident=True, integrand=True, cumulative=True)
    rec.close()
    for a, b, c in zip(before, after, exchange_only()):
        assert np.array_equal(a, b) and np.array_equal(a, c)
