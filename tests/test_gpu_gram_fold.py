"""The A_n Gram  sum_i u_i^H (H u)_i  formed in k_spmm5's epilogue (option s5_gram_min; kernels_spmm5.hpp, S5Gram) instead of by k_mfma_adot's
pass over u and H u: per (group of 8 atoms, output spin) partials, summed in group order by k_gram_groupsum, which also completes the
Hermitian matrix from the rows the epilogue forms.  Smallest shapes that reach every branch: bcc 4x4x4 (64 atoms = eight full groups), bcc
5x4x3 (60 atoms: the last group carries four padding atoms), three sites with one repeated, LL = 8, every level folded (s5_gram_min = 0).
"""
import functools

import numpy as np
import pytest

from helpers import RTOL, objects_from, rel_err, supercell_problem
from rslmtoasa_amd.recursion import Recursion

pytestmark = pytest.mark.gpu

LLD = 8
NEVER = 1 << 40           # a group count no region reaches: the fold is off
FORMS = {"persistent": (("s5_queue", 2),), "global": (("s5_lds", 0),)}


def problem(name):
    """'fe444' / 'fe543': the bcc Fe stencil of tests/golden/bccFe_nsp2_block.npz (spin-diagonal hops, spin-mixing on-site block);
    'rnd444': the Hermitian full-complex operator of tests/test_gpu_random_operator.py."""
    if name == "rnd444":
        from test_gpu_random_operator import random_problem
        return random_problem(5, False)
    return supercell_problem({"fe444": (4, 4, 4), "fe543": (5, 4, 3)}[name])


def sites_of(p):
    kk = p["nn"].shape[0]
    return np.array([1, kk // 2 + 1, 1], dtype=np.int32)        # the third site repeats the first


@functools.lru_cache(maxsize=None)
def oracle_coefficients(oracle_lib, name):
    p = problem(name)
    a, b = oracle_lib.Oracle(p).block_lanczos(sites_of(p), LLD)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


def engine(p, options=(), sites=None, lld=LLD, gram_min=0):
    nsp = int(p.get("nsp", 2))
    rec = Recursion(*objects_from(p, sites_of(p) if sites is None else sites, lld, nsp=nsp, emin=-6.0, emax=6.0), device=0)
    for k, v in (("kernels", 2), ("spmm5", 2), ("s5_gram_min", gram_min)) + tuple(options):
        rec.set_option(k, v)
    return rec


def run(rec):
    rec.recur_b()
    return rec.a_b.copy(), rec.b2_b.copy(), rec.timing()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["fe444", "fe543", "rnd444"])
def test_folded_gram_against_the_oracle(name, form, oracle_lib):
    p = problem(name)
    rec = engine(p, FORMS[form])
    a, b, t = run(rec)
    rec.close()
    a_o, b_o = oracle_coefficients(oracle_lib, name)
    ea, eb = rel_err(a, a_o), rel_err(b, b_o)
    print(name, form, "a_b %.2e b2_b %.2e folded %d of %d" % (ea, eb, t["gram_folded_launches"], t["hop_launches"]))
    assert t["gram_folded_launches"] > 0
    assert ea < RTOL and eb < RTOL


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["fe543", "rnd444"])
def test_fold_on_against_fold_off_on_one_handle(name, form):
    rec = engine(problem(name), FORMS[form])
    a1, b1, t1 = run(rec)
    rec.set_option("s5_gram_min", NEVER)
    a0, b0, t0 = run(rec)
    rec.close()
    assert t1["gram_folded_launches"] == LLD - 1 and t1["hop_fuses_a"] == 1
    assert t0["gram_folded_launches"] == 0 and t0["hop_fuses_a"] == 0
    ea, eb = rel_err(a1, a0), rel_err(b1, b0)
    print(name, form, "on/off a_b %.2e b2_b %.2e" % (ea, eb))
    assert ea < RTOL and eb < RTOL
    eye = np.eye(18)
    for x in (b1, b0):
        assert all(np.array_equal(x[:, :, 0, s], eye) for s in range(x.shape[3]))      # b2_b(:,:,1) = I
    for x in (a1, a0):
        assert not x[:, :, -1, :].any()                                                # a_b(:,:,lld) = 0


@pytest.mark.parametrize("form", sorted(FORMS))
def test_folded_results_are_bitwise_reproducible(form):
    """Two calls; one chain at a time against the batch; the captured level loop (capture + two replays) against plain launches; the B
    reduction on the side stream against the main stream; and the repeated site against its first occurrence."""
    rec = engine(problem("fe543"), FORMS[form] + (("graph", 0),))
    a, b, t = run(rec)
    assert t["gram_folded_launches"] == LLD - 1 and np.isfinite(a).all() and np.abs(a[:, :, :-1, :]).max() > 0
    assert np.array_equal(a[..., 2], a[..., 0]) and np.array_equal(b[..., 2], b[..., 0])
    a2, b2, _ = run(rec)
    assert np.array_equal(a2, a) and np.array_equal(b2, b)
    rec.set_option("batch", 1)
    a2, b2, t2 = run(rec)
    assert t2["gram_folded_launches"] == 3 * (LLD - 1)
    assert np.array_equal(a2, a) and np.array_equal(b2, b)
    rec.set_option("batch", 0)
    rec.set_option("graph", 1)
    for _ in range(3):
        a2, b2, t2 = run(rec)
        assert t2["gram_folded_launches"] == LLD - 1
        assert np.array_equal(a2, a) and np.array_equal(b2, b)
    rec.set_option("graph", 0)
    rec.set_option("side_stream", 0)
    a2, b2, _ = run(rec)
    assert np.array_equal(a2, a) and np.array_equal(b2, b)
    rec.close()


def refusal_problem(kind):
    if kind == "nonhermitian":      # random blocks, one class: eligible in every respect but the operator
        from test_gpu_spmm_random import random_problem
        return random_problem(np.random.default_rng(31), 140, 14, 1, 0, False, True), np.array([1, 70, 140], np.int32)
    if kind == "hoh":
        return supercell_problem((4, 4, 4), hoh=True), np.array([1, 33, 1], np.int32)
    p = dict(supercell_problem((4, 4, 4)))      # nmax > 0: three atoms with blocks of their own
    p["nmax"] = 3
    p["hall"] = np.asfortranarray(p["ee"][:, :, :, :1] * np.array([1.0, 1.05, 0.95]))
    return p, np.array([1, 33, 1], np.int32)


@pytest.mark.parametrize("kind", ["nonhermitian", "hoh", "nmax"])
def test_operators_the_fold_refuses(kind):
    p, sites = refusal_problem(kind)
    rec = engine(p, (("s5_queue", 2),), sites=sites, lld=6)
    rec.recur_b()
    a1, b1, t1 = rec.a_b.copy(), rec.b2_b.copy(), rec.timing()
    rec.set_option("s5_gram_min", NEVER)
    rec.recur_b()
    a0, b0 = rec.a_b.copy(), rec.b2_b.copy()
    rec.close()
    assert t1["gram_folded_launches"] == 0 and t1["hop_fuses_a"] == 0
    assert np.isfinite(a1).all() and np.array_equal(a1, a0) and np.array_equal(b1, b0)


@pytest.mark.parametrize("name", ["fe444", "fe543"])
def test_folded_and_unfolded_levels_in_one_call(name, oracle_lib):
    """s5_gram_min = 5 groups lies between the region of the first application (the 15 atoms of the stencil: two groups) and the whole cell
    (eight groups): the first level keeps k_mfma_adot, the others fold."""
    p = problem(name)
    rec = engine(p, (("s5_queue", 2),), gram_min=5)
    a, b, t = run(rec)
    assert 0 < t["gram_folded_launches"] < LLD - 1 and t["hop_fuses_a"] == 0
    rec.set_option("batch", 1)
    a2, b2, _ = run(rec)
    rec.close()
    assert np.array_equal(a2, a) and np.array_equal(b2, b)
    a_o, b_o = oracle_coefficients(oracle_lib, name)
    ea, eb = rel_err(a, a_o), rel_err(b, b_o)
    print(name, "mixed a_b %.2e b2_b %.2e folded %d of %d" % (ea, eb, t["gram_folded_launches"], t["hop_launches"]))
    assert ea < RTOL and eb < RTOL
