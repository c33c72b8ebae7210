"""The strip operands of the folded A_n Gram (kernels_spmm5.hpp, the Gram epilogue of k_spmm5): columns 16, 17 of a tile's own-atom block are
not loaded per tile but taken, by a row broadcast, from the registers of the remainder tile, whose lane (l15, l4) holds them of atom
l15 >> 1 of the group.  What can go wrong is the lane a tile reads from, and a padding atom's zero block arriving in the wrong tile -- so
the shapes are the smallest that put padding into every lane pattern of the remainder tile: bcc 4x4x4 (64 atoms: full groups), 5x4x3
(60: the last group carries four padding entries), 3x3x7 (63: one) and 3x3x9 (81: seven), and the Hermitian full-complex random
operator, for which every strip element is non-zero.  Both forms of the kernel (persistent / LDS and global-load), every level folded
(s5_gram_min = 0), LL = 8, three sites with one repeated.  The 3-wide cells pass the opposite-slot check of rsrec_set_hamiltonian (each
slot's way back is unique), which `gram_folded_launches == LL - 1` asserts here: an operator that failed it would not fold.
"""
import functools

import numpy as np
import pytest

from helpers import RTOL, rel_err, supercell_problem
from test_gpu_gram_fold import FORMS, LLD, engine, run, sites_of

pytestmark = pytest.mark.gpu

CELLS = {"fe444": (4, 4, 4), "fe543": (5, 4, 3), "fe337": (3, 3, 7), "fe339": (3, 3, 9)}
NAMES = sorted(CELLS) + ["rnd444"]


@functools.lru_cache(maxsize=None)
def problem(name):
    if name == "rnd444":
        from test_gpu_random_operator import random_problem
        return random_problem(5, False)
    return supercell_problem(CELLS[name])


@functools.lru_cache(maxsize=None)
def oracle_coefficients(oracle_lib, name):
    p = problem(name)
    a, b = oracle_lib.Oracle(p).block_lanczos(sites_of(p), LLD)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_strips_from_the_remainder_tile(name, form, oracle_lib):
    p = problem(name)
    rec = engine(p, FORMS[form])
    a, b, t = run(rec)
    rec.set_option("batch", 1)
    a1, b1, t1 = run(rec)
    rec.close()
    a_o, b_o = oracle_coefficients(oracle_lib, name)
    ea, eb = rel_err(a, a_o), rel_err(b, b_o)
    print(name, form, "atoms %d a_b %.2e b2_b %.2e folded %d of %d" % (p["nn"].shape[0], ea, eb, t["gram_folded_launches"], t["hop_launches"]))
    assert t["gram_folded_launches"] == LLD - 1 and t1["gram_folded_launches"] == 3 * (LLD - 1)
    assert ea < RTOL and eb < RTOL
    assert np.array_equal(a1, a) and np.array_equal(b1, b)                                  # one chain at a time against the batch
    assert np.array_equal(a[..., 2], a[..., 0]) and np.array_equal(b[..., 2], b[..., 0])    # the repeated site against its first occurrence
