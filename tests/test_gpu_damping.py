"""rsrec_damping (kernels_exchange.hpp) against the numpy restatement of exchange%calculate_gilbert_damping's traces
(damping_reference.py), fed with g0 from the library's own Green kernels, which test_gpu_green pins to the reference."""
import ctypes as C

import numpy as np
import pytest

from pair_cases import (chain_g0, check_damping as check_against, close, damping_restated as restated, ordered_total, random_tmat,
                        run_device_script, setup)
from rslmtoasa_amd import _lib
from rslmtoasa_amd.exchange import Exchange, damping_tmat

pytestmark = pytest.mark.gpu

PAIRS = np.array([(1, 1), (1, 2), (1, 9), (1, 17), (5, 60), (3, 3)], np.int32)


def angular_momentum():
    """Lx, Ly, Lz (9 x 9) on s, p, d in the complex spherical harmonics, m = -l..l within a shell."""
    Lz, Lp = np.zeros((9, 9), complex), np.zeros((9, 9), complex)
    for l in range(3):
        o = l * l
        for i, m in enumerate(range(-l, l + 1)):
            Lz[o + i, o + i] = m
            if m < l:
                Lp[o + i + 1, o + i] = np.sqrt(l * (l + 1) - m * (m + 1))
    Lm = Lp.conj().T
    return 0.5 * (Lp + Lm), -0.5j * (Lp - Lm), Lz


def physical_tmat(xi_p, xi_d):
    """hamiltonian%tmat (18, 18, 3) of one type as torque_operator_collinear builds it (hamiltonian.f90:1448-1472), `prefac` kept across
    the (i, j) loop as the reference keeps it."""
    Lx, Ly, Lz = angular_momentum()
    t = np.zeros((18, 18, 3), complex)
    sg = 0.5
    soc_p, soc_d = np.sqrt(xi_p[0] * xi_p[1]), np.sqrt(xi_d[0] * xi_d[1])
    prefac = 0.0
    for i in range(9):
        for j in range(9):
            if 1 <= i <= 3 and 1 <= j <= 3:
                prefac = sg * soc_p
            if 4 <= i <= 8 and 4 <= j <= 8:
                prefac = sg * soc_d
            t[j, i, 0] += prefac * 1j * Ly[j, i] * 2.0
            t[j, i + 9, 0] -= prefac * Lz[j, i] * 2.0
            t[j + 9, i, 0] += prefac * Lz[j, i] * 2.0
            t[j + 9, i + 9, 0] -= prefac * 1j * Ly[j, i] * 2.0
            t[j, i, 1] -= prefac * 1j * Lx[j, i] * 2.0
            t[j, i + 9, 1] += prefac * 1j * Lz[j, i] * 2.0
            t[j + 9, i, 1] += prefac * 1j * Lz[j, i] * 2.0
            t[j + 9, i + 9, 1] += prefac * 1j * Lx[j, i] * 2.0
            t[j, i + 9, 2] += prefac * (Lx[j, i] - 1j * Ly[j, i]) * 2.0
            t[j + 9, i, 2] += prefac * (Lx[j, i] + 1j * Ly[j, i]) * 2.0 * (-1.0)
    return t


def run_values(kind, hoh, tmat_of, lld=10):
    rec, g, ene, nv1, dpar = setup(PAIRS, hoh=hoh, kind=kind, lld=lld)
    tmat = tmat_of(len(PAIRS))
    g0 = chain_g0(rec, g, kind, 4 * len(PAIRS))
    ref = restated(g0, PAIRS, tmat)
    ief = 166
    coef = (rec.a_b, rec.b2_b) if kind == "block" else None
    res = Exchange(rec, g).damping(tmat, ief, kind=kind, rows=True, coef=coef)
    check_against(res, ref, ief)
    rec.close()


@pytest.mark.parametrize("hoh", [False, True])
def test_block_matches_restatement(hoh):
    run_values("block", hoh, random_tmat)


def test_chebyshev_matches_restatement():
    run_values("chebyshev", False, random_tmat, lld=12)


def two_type_tmat(npairs):
    """Physical torque matrices of two atom types with different spin-orbit parameters, the odd atoms of the cell of type 1 and the
    even ones of type 2: the pairs (1, 2) and (5, 60) have different matrices on their two sides, so a swap of the sides, in the kernel
    or in damping_tmat's gather by iz, changes the rows."""
    t = np.stack([physical_tmat((0.0045, 0.0038), (0.0041, 0.0033)), physical_tmat((0.0102, 0.0087), (0.0019, 0.0023))], axis=3)
    iz = 1 + (np.arange(64) + 1 + 1) % 2
    tm = damping_tmat(t, iz, PAIRS[:npairs])
    assert iz[0] == 1 and iz[1] == 2 and not np.array_equal(tm[:, :, :, 0, 1], tm[:, :, :, 1, 1])
    return tm


@pytest.mark.parametrize("kind,hoh", [("block", False), ("block", True), ("chebyshev", False)])
def test_physical_tmat_matches_restatement(kind, hoh):
    run_values(kind, hoh, two_type_tmat, lld=12 if kind == "chebyshev" else 10)


DEVICE_SCRIPT = r"""
from rslmtoasa_amd.exchange import Exchange
if mode == "sources":
    pairs = np.array([(1, 1), (1, 2), (7, 30), (2, 2), (9, 40)], np.int32)
    rec, g, ene, nv1, dpar = T.setup(pairs, lld=8)
    x = Exchange(rec, g)
    tmat, ief = T.random_tmat(len(pairs)), 120
    res_dev = x.damping(tmat, ief, rows=True, resident=True)
    res_dev2 = x.damping(tmat, ief, rows=True, resident=True)
    rec.zsqr()
    a_inf, b_inf, _, _ = g.terminator(nsites=4 * len(pairs))
    res_host = x.damping(tmat, ief, rows=True)
    res_host_t = x.damping(tmat, ief, rows=True, a_inf=a_inf, b_inf=b_inf)
    ta = torch.from_numpy(np.ascontiguousarray(rec.a_b.transpose(3, 2, 1, 0))).cuda()
    tb = torch.from_numpy(np.ascontiguousarray(rec.b2_b.transpose(3, 2, 1, 0))).cuda()
    tt = torch.from_numpy(np.ascontiguousarray(tmat.transpose(4, 3, 2, 1, 0))).cuda()
    res_t = x.damping(tt, ief, rows=True, coef=(ta, tb))
    for other in (res_dev2, res_host, res_host_t, res_t):
        for a, b in zip(res_dev, other):
            assert np.array_equal(a, b)
    g0 = T.chain_g0(rec, g, "block", 4 * len(pairs), zsqr=False)
    T.check_damping(res_dev, T.damping_restated(g0, pairs, tmat), ief)
else:
    # 8192 pairs at nE = 2510: g0 of their chains would take 427 GB, more than the device holds
    pairs = np.array([(1, 2)], np.int32)
    rec, g, ene, nv1, dpar = T.setup(pairs, lld=4, channels=2501)
    assert len(ene) == 2510
    rec.zsqr()
    x = Exchange(rec, g)
    tmat, ief = T.random_tmat(1), 1300
    one = x.damping(tmat, ief, rows=True)
    n = 8192
    ta = torch.from_numpy(np.ascontiguousarray(rec.a_b[..., :4].transpose(3, 2, 1, 0))).cuda().repeat(n, 1, 1, 1)
    tb = torch.from_numpy(np.ascontiguousarray(rec.b2_b[..., :4].transpose(3, 2, 1, 0))).cuda().repeat(n, 1, 1, 1)
    tt = torch.from_numpy(np.ascontiguousarray(tmat.transpose(4, 3, 2, 1, 0))).cuda().repeat(n, 1, 1, 1, 1)
    rec.lattice.ijpair = np.repeat(pairs, n, axis=0)
    free0 = torch.cuda.mem_get_info()[0]
    at_ef, total = x.damping(tt, ief, coef=(ta, tb))
    used = free0 - torch.cuda.mem_get_info()[0]
    assert np.array_equal(at_ef, np.repeat(one[0], n, axis=1))
    t = np.zeros_like(one[1])
    for _ in range(n):
        t = t + one[2][:9, :, 0]
    assert np.array_equal(total, t)
    print("device ms for %d pairs: %.1f, device memory taken by the call: %.0f MiB" % (n, x.timing()[0], used / 2**20))
    # (the rows of 8192 pairs alone would be 2.8 GiB; the figure is printed, not asserted: other processes share the device)
rec.close()
print("DAMPING_DEVICE_OK")
"""


def test_coefficient_sources_agree_bitwise():
    """Resident chains (i == j pairs compacted), caller coefficients with and without caller terminators, and device-pointer
    coefficients and tmat give the same bits; so does a repeated call.  And they match the restatement."""
    run_device_script(DEVICE_SCRIPT, "sources", "DAMPING_DEVICE_OK")


def test_memory_is_bounded_for_8192_pairs():
    """8192 pairs at nE = 2510 and lld 4 with rows = NULL finish; every pair (all the same chains) carries
    the single-pair result and total is the ordered sum."""
    run_device_script(DEVICE_SCRIPT, "memory", "DAMPING_DEVICE_OK")


SPLIT_PAIRS = np.array([(1, 1), (1, 2), (3, 19), (2, 2), (4, 50), (6, 7), (8, 8)], np.int32)


def split_calls(rows=True):
    from rslmtoasa_amd.recursion import site_partition
    rec, g, ene, nv1, dpar = setup(SPLIT_PAIRS, lld=8, channels=100)
    rec.zsqr()
    tmat, ief = random_tmat(len(SPLIT_PAIRS)), 61
    whole = Exchange(rec, g).damping(tmat, ief, rows=rows)
    halves = []
    for r in range(2):
        rec.rank, rec.nprocs = r, 2
        s, e = site_partition(r, 2, len(SPLIT_PAIRS))
        coef = (rec.a_b[..., 4 * (s - 1):4 * e], rec.b2_b[..., 4 * (s - 1):4 * e])
        halves.append(Exchange(rec, g).damping(tmat[..., s - 1:e], ief, rows=rows, pair_offset=s - 1, npairs_total=len(SPLIT_PAIRS), coef=coef))
    rec.rank, rec.nprocs = 0, 1
    rec.close()
    return whole, halves


def test_partitioned_images_sum_to_the_single_call():
    whole, halves = split_calls()
    assert np.array_equal(halves[0][0] + halves[1][0], whole[0])
    # a pair's rows do not depend on the other pairs of the launch
    assert np.array_equal(np.concatenate([halves[0][2], halves[1][2]], axis=2), whole[2])


def test_totals_of_a_split_call():
    """`total` is the sum over the call's pairs in ascending pair order from zero, ((0 + p1) + p2) + ...  Floating-point addition is not
    associative, so the sum of two halves' totals, (p1 + .. + p4) + (p5 + .. + p7), is not the single call's total to the last bit in
    general; the fixed order that does hold is checked instead: continuing the ordered sum from the first half's total through the second
    half's rows gives the single call's total bit for bit, and each call's total is the ordered sum of its own rows."""
    whole, halves = split_calls()
    for at_ef, total, rows in [whole] + halves:
        assert np.array_equal(total, ordered_total(rows))
    t = halves[0][1].copy()
    for q in range(halves[1][2].shape[2]):
        t = t + halves[1][2][:9, :, q]
    assert np.array_equal(t, whole[1])
    assert close(halves[0][1] + halves[1][1], whole[1], 0.0)


def test_two_calls_are_bitwise_equal():
    rec, g, ene, nv1, dpar = setup(PAIRS, lld=8, channels=100, kind="chebyshev")
    tmat = random_tmat(len(PAIRS))
    a = Exchange(rec, g).damping(tmat, 40, kind="chebyshev", rows=True)
    b = Exchange(rec, g).damping(tmat, 40, kind="chebyshev", rows=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    rec.close()


def test_bad_arguments_are_errors():
    pairs = np.array([(1, 2)], np.int32)
    rec, g, ene, nv1, dpar = setup(pairs, lld=6, channels=40)
    L, h = rec._L, rec._h
    same = np.zeros(1, np.int32)
    tmat = random_tmat(1)
    at_ef, total = np.zeros((18, 1), order="F"), np.zeros((9, len(ene)), order="F")
    ab = np.asfortranarray(rec.a_b[..., :4])
    bb = np.asfortranarray(rec.b2_b[..., :4])
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(kind=0, npairs=1, ief=3, tm=tmat, outs=(at_ef, total), same_=same):
        at_ef[:], total[:] = -7.0, -7.0
        rc = L.rsrec_damping(h, kind, npairs, P(same_), 6, len(ene), P(ene), ief, 0, -0.6, 0.4, None, None, P(ab), P(bb), P(tm), 0, 1,
                             P(outs[0]), P(outs[1]), None)
        if rc:                                              # nothing ran: the outputs are untouched
            assert np.all(at_ef == -7.0) and np.all(total == -7.0)
        return rc
    assert call() == 0
    assert call(ief=0) == _lib.ERR_ARG
    assert call(ief=len(ene) + 1) == _lib.ERR_ARG
    assert call(ief=len(ene)) == 0
    assert call(tm=None) == _lib.ERR_ARG
    assert call(npairs=0) == _lib.ERR_ARG
    assert call(kind=2) == _lib.ERR_ARG
    assert call(outs=(None, total)) == _lib.ERR_ARG
    assert call(outs=(at_ef, None)) == _lib.ERR_ARG
    assert call(same_=None) == _lib.ERR_ARG
    assert call() == 0                                          # the handle still works
    rec.close()


def test_resident_compacted_chains_refuse_caller_terminators():
    pairs = np.array([(1, 1), (1, 2)], np.int32)
    rec, g, ene, nv1, dpar = setup(pairs, lld=6, channels=40)
    ai = np.zeros((18, 18, 8), order="F")
    with pytest.raises(_lib.RsrecError) as ei:
        Exchange(rec, g).damping(random_tmat(2), 5, resident=True, a_inf=ai, b_inf=ai)
    assert ei.value.code == _lib.ERR_ARG and "terminators" in str(ei.value)
    Exchange(rec, g).damping(random_tmat(2), 5, resident=True)      # the handle still works, with the device terminator
    rec.close()


@pytest.mark.parametrize("kind,res", [("block", True), ("chebyshev", True), ("chebyshev", False)])
def test_exchange_is_unchanged_by_a_damping_call(kind, res):
    """rsrec_exchange after rsrec_damping on the same handle gives the bits of a handle that never ran damping: on the chains the seeded
    recursion left on the device (block: compacted; Chebyshev: 4 per pair) and on the recursion's host arrays."""
    fermi = -0.05

    def exchange_only():
        rec, g, ene, nv1, dpar = setup(PAIRS, lld=8, channels=100, kind=kind)
        out = Exchange(rec, g).compute(fermi, nv1, dpar, kind=kind, resident=res, integrand=True, cumulative=True)
        rec.close()
        return out
    rec, g, ene, nv1, dpar = setup(PAIRS, lld=8, channels=100, kind=kind)
    x = Exchange(rec, g)
    before = x.compute(fermi, nv1, dpar, kind=kind, resident=res, integrand=True, cumulative=True)
    x.damping(random_tmat(len(PAIRS)), 30, kind=kind, resident=res, rows=True)
    after = x.compute(fermi, nv1, dpar, kind=kind, resident=res, integrand=True, cumulative=True)
    rec.close()
    for a, b, c in zip(before, after, exchange_only()):
        assert np.array_equal(a, b) and np.array_equal(a, c)
