"""The conditions that tests/test_gpu_batch_composition.py and tests/test_gpu_post_hop_forms.py rely on, stated on the lattices of
tests/piece_lattices.py themselves (no GPU): symmetric tables, connected pieces, regions that fill their piece early enough, the intended
workgroup counts, and chains that the CPU oracle finds well enough conditioned to be compared (cond(B_n^2) <= 1e3 at every level, the
'comparable' rule of tools/fuzz_recursion.py).  Conditions, not measurements: a lattice that misses one gets another rng seed in
piece_lattices.py, never a wider bar."""
import numpy as np
import pytest

import piece_lattices as PL

COND_BAR = 1e3


def check_table(p, sizes, nslots=9):
    nn = p["nn"]
    kk = sum(sizes)
    assert nn.shape == (kk, nslots + 1) and p["nmax"] == 0 and p["ee"].shape == (18, 18, nslots, 1) and (p["iz"] == 1).all()
    assert nn[:, 0].min() >= 1 and nn[:, 0].max() <= nslots
    for k in range(1, kk + 1):
        nb = PL.neighbours(nn, k)
        assert len(set(nb)) == len(nb) and k not in nb
        assert not nn[k - 1, nn[k - 1, 0]:].any()                       # nothing behind the count
        for n in nb:
            assert k in PL.neighbours(nn, n), (k, n)                    # symmetric
    for lo, hi in PL.piece_bounds(sizes):
        assert PL.region_atoms(nn, lo) == list(range(lo, hi + 1))       # connected, and closed
        assert PL.region_atoms(nn, hi) == list(range(lo, hi + 1))


def saturation_level(nn, seed, size, nlevels):
    counts = PL.region_counts(nn, seed, nlevels)
    assert counts[0] == 1 and (np.diff(counts) >= 0).all() and counts[-1] == size, (seed, counts)
    return int(np.argmax(counts == size))


@pytest.mark.parametrize("hoh", [False, True])
def test_batch_lattice_regions_and_workgroups(hoh):
    p = PL.batch_problem(hoh)
    check_table(p, PL.BATCH_SIZES)
    assert sum(PL.BATCH_SIZES) == 3961
    assert [PL.workgroups(n) for n in PL.BATCH_SIZES] == [12, 25, 38, 51]
    assert PL.BATCH_WORKGROUPS == {n: PL.workgroups(n) for n in PL.BATCH_SIZES}
    assert sorted(PL.BATCH_SEEDS) == ["s12", "s25", "s38", "s51"]
    assert sum(n % 8 != 0 for n in PL.BATCH_SIZES) >= 2                # last groups with padding atoms
    assert (p["nn"][:, 1:9] == 0).sum(axis=1)[p["nn"][:, 0] == 9].max() >= 2      # absent neighbours in front of the count
    hops = PL.BATCH_LLD - 1                                             # H is applied lld - 1 times; with hoh every application is two hops
    for (lo, hi), size in zip(PL.piece_bounds(PL.BATCH_SIZES), PL.BATCH_SIZES):
        assert PL.BATCH_SEEDS["s%d" % PL.workgroups(size)] == lo
        L = saturation_level(p["nn"], lo, size, hops)
        assert L + 3 <= hops, (size, L)                                 # three further levels on the whole piece
        # 17 .. 32 workgroups alone, more than 32 beside a larger chain: the window of the single-stage against the two-stage sum
        if size == 771:
            assert 17 <= PL.workgroups(size) <= 32 < PL.workgroups(1603)


@pytest.mark.parametrize("kk", PL.ONE_PIECE_KK)
def test_one_piece_lattices(kk):
    """The group counts the sizes stand for are reached inside the depth the GPU tests run: 1 partial group, 1 group, 2 groups with one live atom
    in the second, 5 groups (wave 0 walks two tiles, the others one), 29 and 33 groups (8 and 9 workgroups: either side of the switch to
    per-XCD chunks), 138 groups (35 workgroups: the two-stage sum)."""
    groups = -(-kk // 8)
    assert {7: 1, 8: 1, 9: 2, 33: 5, 230: 29, 260: 33, 1100: 138}[kk] == groups
    for hoh in (False, True):
        p = PL.one_piece_problem(kk, hoh)
        check_table(p, (kk,))
        for lld in PL.one_piece_llds(kk, hoh):
            hops = (lld - 1) * (2 if hoh else 1)
            for s in PL.one_piece_seeds(kk):
                reached = int(PL.region_counts(p["nn"], int(s), hops)[-1])
                if kk == 1100 and not hoh and lld == PL.one_piece_lld(kk):
                    # four hops of at most eight neighbours do not fill 1100 atoms: this depth ends inside the single-stage window, the
                    # deeper run of one_piece_llds (and the hoh operator's eight hops) reach all 138 groups
                    assert 16 < PL.workgroups(reached) <= 32, reached
                else:
                    assert -(-reached // 8) == groups, (kk, hoh, lld, int(s), reached)
    assert PL.workgroups(230) == 8 and PL.workgroups(260) == 9 and PL.workgroups(1100) == 35


def test_hermitian_and_two_piece_lattices():
    for name, sizes in PL.HERMITIAN_CASES.items():
        p = PL.hermitian_problem(name)
        check_table(p, sizes)
        nn, ee = p["nn"], p["ee"]
        assert (nn[:, 1:9] == 0).any()                                  # cut bonds
        for k in range(1, sum(sizes) + 1):                              # slot s leads back through its partner slot
            for s in range(1, 9):
                n = nn[k - 1, s]
                if n:
                    assert nn[n - 1, s + 1 if s % 2 else s - 1] == k
        for s in range(1, 9, 2):
            assert np.array_equal(ee[:, :, s + 1, 0], ee[:, :, s, 0].conj().T)
        assert np.array_equal(ee[:, :, 0, 0], ee[:, :, 0, 0].conj().T) and np.array_equal(p["lsham"][:, :, 0], p["lsham"][:, :, 0].conj().T)
    p = PL.two_piece_problem()
    check_table(p, PL.TWO_PIECE_SIZES)
    assert 0.76 < PL.TWO_PIECE_SIZES[0] / sum(PL.TWO_PIECE_SIZES) < 0.78      # sat_pct 40: the larger piece saturates, 80: no chain does
    assert PL.TWO_PIECE_SIZES[1] / sum(PL.TWO_PIECE_SIZES) < 0.4                    # the smaller piece never does
    total, hops = sum(PL.TWO_PIECE_SIZES), PL.TWO_PIECE_LLD - 1
    reached = [int(PL.region_counts(p["nn"], int(s), hops)[-1]) for s in PL.two_piece_seeds()]
    in_large = [int(s) <= PL.TWO_PIECE_SIZES[0] for s in PL.two_piece_seeds()]
    assert sorted(in_large) == [False, True, True]
    for r, large in zip(reached, in_large):             # sat_pct 40: reached inside the depth by the chains of the larger piece only; 80: by none
        assert (r >= 0.4 * total) == large and r < 0.8 * total, (reached, in_large)
    for kk in (260,):                                    # the one-piece lattice of the sat_pct test: 40 and 80 % are reached before the last hop
        q = PL.one_piece_problem(kk)
        for s in PL.one_piece_seeds(kk):
            counts = PL.region_counts(q["nn"], int(s), PL.one_piece_lld(kk) - 1)
            assert counts[-2] >= 0.4 * kk and counts[-1] >= 0.8 * kk, counts


def chains_of_the_gpu_tests():
    """(label, problem, seeds, lld) of every block-Lanczos call whose result the GPU tests compare with the oracle."""
    for hoh in (False, True):
        yield "batch hoh=%d" % hoh, PL.batch_problem(hoh), np.array(sorted(PL.BATCH_SEEDS.values()), np.int32), PL.BATCH_LLD
        for kk in PL.ONE_PIECE_KK:
            yield "piece %d hoh=%d" % (kk, hoh), PL.one_piece_problem(kk, hoh), PL.one_piece_seeds(kk), max(PL.one_piece_llds(kk, hoh))
    for kk in (260, 1100):       # the workgroup bands: 32 chains, the 1100-atom piece also at the depth that fills it
        yield "bands %d" % kk, PL.one_piece_problem(kk), PL.round_robin_seeds(kk, 32), max(PL.one_piece_llds(kk, False))
    for name in PL.HERMITIAN_CASES:
        yield name, PL.hermitian_problem(name), PL.hermitian_seeds(name), PL.HERMITIAN_LLD
    yield "two pieces", PL.two_piece_problem(), PL.two_piece_seeds(), PL.TWO_PIECE_LLD


def test_every_chain_is_well_conditioned(oracle_lib):
    worst = {}
    for label, p, seeds, lld in chains_of_the_gpu_tests():
        a_o, b_o = oracle_lib.Oracle(p).block_lanczos(seeds, lld)
        assert np.isfinite(a_o).all() and np.isfinite(b_o).all(), label
        worst[label] = PL.max_condition(b_o)
    print({k: "%.1f" % v for k, v in worst.items()})
    assert all(v <= COND_BAR for v in worst.values()), worst
