"""rsrec_exchange_contour and rsrec_contour_occupation (kernels_contour.hpp) against the numpy restatement of the reference's
Gauss-Legendre contour stages (contour_reference.py).  Block: the restatement is fed with g from ``Green.block_green(..., eta=...)``, one
call per point (pinned to the reference by test_block_green_eta_against_reference); Chebyshev: with chebyshev_green_ij_eta restated in
numpy from the moments.

Bar: the rule of test_exchange_oracle / test_gpu_exchange, 1e-12 relative to the pair's scale; a quantity that vanishes by symmetry is
judged on the pair's largest row, and a contour sum on the largest |summand| (the sum multiplies small values by weights of several
thousand and can cancel)."""
import ctypes as C

import numpy as np
import pytest

from contour_reference import chebyshev_green_eta, contour_eta, occupation
from exchange_reference import PI
from helpers import objects_from, supercell_problem
from pair_cases import (EMAX, EMIN, TOL, block_g_at_points, check_contour_pairs as check_pairs, onsite, random_contour_dmat as random_dmat,
                        run_device_script, setup)
from rslmtoasa_amd import _lib
from rslmtoasa_amd.exchange import Exchange, contour_dmat, gauss_legendre
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.recursion import Recursion

pytestmark = pytest.mark.gpu

PAIRS = np.array([(1, 1), (1, 2), (1, 9), (5, 60), (3, 3)], np.int32)
NPTS = (1, 5, 64, 67)          # 67: past one wave's worth of points


@pytest.mark.parametrize("hoh", [False, True])
def test_block_matches_restatement(hoh):
    rec, g, ene, nv1, dpar = setup(PAIRS, hoh=hoh, lld=8, channels=100)
    rec.zsqr()
    n = 4 * len(PAIRS)
    a_inf, b_inf, _, _ = g.terminator(nsites=n)
    e0 = float(ene[55])
    dmat = random_dmat(len(PAIRS))
    for npts in (NPTS if not hoh else (64,)):
        x, w = gauss_legendre(npts)
        gp = block_g_at_points(rec, e0, contour_eta(x), n, a_inf, b_inf)
        xc, rows = Exchange(rec, g).contour(x, w, e0, dmat, rows=True, coef=(rec.a_b, rec.b2_b))
        check_pairs(xc, rows, gp, PAIRS, dmat, x, w)
        xc_t, rows_t = Exchange(rec, g).contour(x, w, e0, dmat, rows=True, coef=(rec.a_b, rec.b2_b), a_inf=a_inf, b_inf=b_inf)
        assert np.array_equal(xc, xc_t) and np.array_equal(rows, rows_t)            # caller terminators = the device's own
    rec.close()


def test_physical_dmat_and_sym_term():
    """dmat gathered from hamiltonian%ee by ``contour_dmat``, and control%sym_term honoured."""
    p = supercell_problem((4, 4, 4))
    rec, g, ene, nv1, dpar = setup(PAIRS, lld=6, channels=100)
    rec.zsqr()
    g.sym_term = True
    n = 4 * len(PAIRS)
    a_inf, b_inf, _, _ = g.terminator(nsites=n)
    dmat = contour_dmat(p["ee"], p["iz"], PAIRS)
    assert dmat.shape == (9, 9, 2, len(PAIRS)) and np.abs(dmat).max() > 0
    assert np.array_equal(dmat[:, :, 0, 1], np.real(p["ee"][:9, :9, 0, 0] - p["ee"][9:, 9:, 0, 0]))
    x, w = gauss_legendre(64)
    e0 = float(ene[40])
    g1 = Green(rec, np.array([e0]), sym_term=True)
    gp = np.zeros((18, 18, 64, n), np.complex128)
    for k, et in enumerate(contour_eta(x)):
        gp[:, :, k, :] = g1.block_green(a_inf, b_inf, eta=1j * et, nsites=n)[:, :, 0, :]
    xc, rows = Exchange(rec, g).contour(x, w, e0, dmat, rows=True, coef=(rec.a_b, rec.b2_b))
    check_pairs(xc, rows, gp, PAIRS, dmat, x, w)
    rec.close()


def test_chebyshev_matches_restatement():
    rec, g, ene, nv1, dpar = setup(PAIRS, kind="chebyshev", lld=10, channels=100)
    n = 4 * len(PAIRS)
    e0 = float(ene[55])
    dmat = random_dmat(len(PAIRS))
    for npts in NPTS:
        x, w = gauss_legendre(npts)
        gp = chebyshev_green_eta(rec.mu_n[:, :, :, :n], e0, contour_eta(x), EMIN, EMAX)
        xc, rows = Exchange(rec, g).contour(x, w, e0, dmat, kind="chebyshev", rows=True)
        check_pairs(xc, rows, gp, PAIRS, dmat, x, w)
    rec.close()


def occ_close(occ, ref, y):
    """1e-12 on the scale of the largest |summand| of the sum (or of the occupation itself)."""
    return np.abs(occ - ref).max() / max(np.abs(y).max() / PI, np.abs(ref).max()) <= TOL


@pytest.mark.parametrize("npts", NPTS)
def test_block_occupation_equals_the_loop_it_replaces(npts):
    """contour_occupation = sum_k over single-point block_green(eta_k) calls, the weighted sum formed in numpy from the per-point g."""
    rec = onsite("block", 8)
    n = 3
    g = Green(rec, np.array([-0.07]))
    x, w = gauss_legendre(npts)
    e0 = -0.07
    res_occ, res_gd = g.contour_occupation(x, w, e0, diag=True, resident=True)
    rec.zsqr()
    a_inf, b_inf, _, _ = g.terminator(nsites=n)
    gp = block_g_at_points(rec, e0, contour_eta(x), n, a_inf, b_inf)
    d = np.arange(18)
    gd = gp[d, d]                                            # (18, npts, n)
    ref = occupation(gd, x, w)
    y = (gd.real * w[None, :, None]) / (x * x)[None, :, None]
    occ, gdev = g.contour_occupation(x, w, e0, diag=True)
    assert np.abs(gdev - gd).max() <= TOL * np.abs(gd).max()
    print("%d points: occ deviation %.2e, largest summand / pi %.3e" % (npts, np.abs(occ - ref).max(), np.abs(y).max() / PI))
    assert occ_close(occ, ref, y)
    assert np.array_equal(occ, occupation(gdev, x, w))       # the device's own diagonal, summed in order: the same bits
    assert np.array_equal(occ, res_occ) and np.array_equal(gdev, res_gd)     # resident chains = the host arrays after zsqr
    occ_t = g.contour_occupation(x, w, e0, a_inf=a_inf, b_inf=b_inf)
    assert np.array_equal(occ, occ_t)
    if npts == 64:                                           # a converged contour counts electrons: 0 < occ < 1 per spin-orbital
        assert np.all(occ > 0) and np.all(occ < 1)
    rec.close()


def test_chebyshev_occupation_matches_restatement():
    rec = onsite("chebyshev", 10)
    g = Green(rec, np.array([-0.07]))
    e0 = -0.07
    for npts in NPTS:
        x, w = gauss_legendre(npts)
        gp = chebyshev_green_eta(rec.mu_n[:, :, :, :3], e0, contour_eta(x), EMIN, EMAX)
        d = np.arange(18)
        gd = gp[d, d]
        ref = occupation(gd, x, w)
        y = (gd.real * w[None, :, None]) / (x * x)[None, :, None]
        occ, gdev = g.contour_occupation(x, w, e0, kind="chebyshev", diag=True)
        print("%d points: g deviation / scale %.2e, occ deviation %.2e" % (npts, np.abs(gdev - gd).max() / np.abs(gd).max(), np.abs(occ - ref).max()))
        assert np.abs(gdev - gd).max() <= TOL * np.abs(gd).max()
        assert occ_close(occ, ref, y)
        res = g.contour_occupation(x, w, e0, kind="chebyshev", resident=True)
        assert np.array_equal(occ, res)
    rec.close()


def test_occupation_images_of_a_partition_sum_to_the_single_call():
    rec = onsite("block", 6, sites=(1, 30, 64, 7, 12))
    rec.zsqr()
    g = Green(rec, np.array([-0.07]))
    x, w = gauss_legendre(5)
    whole = g.contour_occupation(x, w, -0.07)
    from rslmtoasa_amd.recursion import site_partition
    a_b, b2_b = rec.a_b.copy(), rec.b2_b.copy()
    parts = []
    for r in range(2):
        rec.rank, rec.nprocs = r, 2
        s, e = site_partition(r, 2, 5)
        rec.a_b[..., :e - s + 1], rec.b2_b[..., :e - s + 1] = a_b[..., s - 1:e], b2_b[..., s - 1:e]
        parts.append(g.contour_occupation(x, w, -0.07, site_offset=s - 1, nsites_total=5))
    rec.rank, rec.nprocs = 0, 1
    assert np.array_equal(parts[0] + parts[1], whole)
    rec.close()


DEVICE_SCRIPT = r"""
from contour_reference import contour_eta
from rslmtoasa_amd.exchange import Exchange, gauss_legendre
if mode == "sources":
    pairs = np.array([(1, 1), (1, 2), (7, 30), (2, 2), (9, 40)], np.int32)
    for kind, lld in (("block", 8), ("chebyshev", 6)):
        rec, g, ene, nv1, dpar = T.setup(pairs, lld=lld, channels=100, kind=kind)
        ex = Exchange(rec, g)
        x, w = gauss_legendre(64)
        e0, dmat = float(ene[50]), T.random_contour_dmat(len(pairs))
        res_dev = ex.contour(x, w, e0, dmat, kind=kind, rows=True, resident=True)          # block: the i == j pairs compacted
        res_dev2 = ex.contour(x, w, e0, dmat, kind=kind, rows=True, resident=True)
        td = torch.from_numpy(np.ascontiguousarray(dmat.transpose(3, 2, 1, 0))).cuda()
        if kind == "block":
            rec.zsqr()
            a_inf, b_inf, _, _ = g.terminator(nsites=4 * len(pairs))
            others = [ex.contour(x, w, e0, dmat, rows=True), ex.contour(x, w, e0, dmat, rows=True, a_inf=a_inf, b_inf=b_inf)]
            ta = torch.from_numpy(np.ascontiguousarray(rec.a_b.transpose(3, 2, 1, 0))).cuda()
            tb = torch.from_numpy(np.ascontiguousarray(rec.b2_b.transpose(3, 2, 1, 0))).cuda()
            others.append(ex.contour(x, w, e0, td, rows=True, coef=(ta, tb)))
            gp = T.block_g_at_points(rec, e0, contour_eta(x), 4 * len(pairs), a_inf, b_inf)
            T.check_contour_pairs(res_dev[0], res_dev[1], gp, pairs, dmat, x, w)
        else:
            tm = torch.from_numpy(np.ascontiguousarray(rec.mu_n.transpose(3, 2, 1, 0))).cuda()
            others = [ex.contour(x, w, e0, dmat, kind=kind, rows=True), ex.contour(x, w, e0, td, kind=kind, rows=True, coef=(tm,))]
        for other in [res_dev2] + others:
            for a, b in zip(res_dev, other):
                assert np.array_equal(a, b)
        rec.close()
else:
    # just above one chunk of pairs at lld 4 (512 MiB of staged coefficients: 3236 pairs), every pair the same chains
    pairs = np.array([(1, 2)], np.int32)
    rec, g, ene, nv1, dpar = T.setup(pairs, lld=4, channels=40)
    rec.zsqr()
    ex = Exchange(rec, g)
    x, w = gauss_legendre(5)
    e0, dmat = float(ene[20]), T.random_contour_dmat(1)
    one = ex.contour(x, w, e0, dmat, rows=True)
    n = 3300
    ta = torch.from_numpy(np.ascontiguousarray(rec.a_b[..., :4].transpose(3, 2, 1, 0))).cuda().repeat(n, 1, 1, 1)
    tb = torch.from_numpy(np.ascontiguousarray(rec.b2_b[..., :4].transpose(3, 2, 1, 0))).cuda().repeat(n, 1, 1, 1)
    td = torch.from_numpy(np.ascontiguousarray(dmat.transpose(3, 2, 1, 0))).cuda().repeat(n, 1, 1, 1)
    rec.lattice.ijpair = np.repeat(pairs, n, axis=0)
    xc, rows = ex.contour(x, w, e0, td, rows=True, coef=(ta, tb))
    assert np.array_equal(xc, np.repeat(one[0], n, axis=1)) and np.array_equal(rows, np.repeat(one[1], n, axis=2))
    print("device ms for %d pairs: %.1f" % (n, ex.timing()[0]))
    rec.close()
print("CONTOUR_DEVICE_OK")
"""


def test_coefficient_sources_agree_bitwise():
    """Resident chains (block: i == j pairs compacted), caller coefficients with and without caller terminators, and device-pointer
    coefficients and dmat give the same bits; so does a repeated call.  And they match the restatement."""
    run_device_script(DEVICE_SCRIPT, "sources", "CONTOUR_DEVICE_OK")


def test_pairs_past_one_chunk_carry_the_single_pair_result():
    run_device_script(DEVICE_SCRIPT, "chunks", "CONTOUR_DEVICE_OK")


SPLIT_PAIRS = np.array([(1, 1), (1, 2), (3, 19), (2, 2), (4, 50), (6, 7), (8, 8)], np.int32)


def test_partitioned_images_sum_to_the_single_call():
    from rslmtoasa_amd.recursion import site_partition
    rec, g, ene, nv1, dpar = setup(SPLIT_PAIRS, lld=6, channels=100)
    rec.zsqr()
    x, w = gauss_legendre(5)
    e0, dmat = float(ene[50]), random_dmat(len(SPLIT_PAIRS))
    whole = Exchange(rec, g).contour(x, w, e0, dmat, rows=True)
    halves = []
    for r in range(2):
        rec.rank, rec.nprocs = r, 2
        s, e = site_partition(r, 2, len(SPLIT_PAIRS))
        coef = (rec.a_b[..., 4 * (s - 1):4 * e], rec.b2_b[..., 4 * (s - 1):4 * e])
        halves.append(Exchange(rec, g).contour(x, w, e0, dmat[..., s - 1:e], rows=True, pair_offset=s - 1, npairs_total=len(SPLIT_PAIRS), coef=coef))
    rec.rank, rec.nprocs = 0, 1
    rec.close()
    assert np.array_equal(halves[0][0] + halves[1][0], whole[0])
    assert np.array_equal(np.concatenate([halves[0][1], halves[1][1]], axis=2), whole[1])


def test_bad_arguments_are_errors():
    pairs = np.array([(1, 2)], np.int32)
    rec, g, ene, nv1, dpar = setup(pairs, lld=6, channels=40)
    L, h = rec._L, rec._h
    same = np.zeros(1, np.int32)
    dmat = random_dmat(1)
    x, w = gauss_legendre(5)
    xc = np.zeros((13, 1), order="F")
    occ = np.zeros((18, 4), order="F")
    ab = np.asfortranarray(rec.a_b[..., :4])
    bb = np.asfortranarray(rec.b2_b[..., :4])
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(kind=0, npairs=1, npts=5, x_=x, w_=w, dm=dmat, out=xc, same_=same):
        xc[:] = -7.0
        rc = L.rsrec_exchange_contour(h, kind, npairs, P(same_), 6, npts, P(x_), P(w_), -0.1, 0, EMIN, EMAX, None, None, P(ab), P(bb), P(dm), 0, 1,
                                      P(out), None)
        if rc:                                              # nothing ran: the output is untouched
            assert np.all(xc == -7.0)
        return rc

    def call_occ(kind=0, nsites=4, npts=5, x_=x, w_=w, out=occ):
        return L.rsrec_contour_occupation(h, kind, nsites, 6, npts, P(x_), P(w_), -0.1, 0, EMIN, EMAX, None, None, P(ab), P(bb), 0, 4, P(out), None)
    assert call() == 0
    assert call(npts=0) == _lib.ERR_ARG
    assert call(npairs=0) == _lib.ERR_ARG
    assert call(kind=2) == _lib.ERR_ARG
    assert call(x_=None) == _lib.ERR_ARG
    assert call(w_=None) == _lib.ERR_ARG
    assert call(dm=None) == _lib.ERR_ARG
    assert call(out=None) == _lib.ERR_ARG
    assert call(same_=None) == _lib.ERR_ARG
    assert call(x_=np.zeros(5)) == _lib.ERR_ARG             # eta = (1 - x) / x needs x > 0
    assert call() == 0                                      # the handle still works
    assert call_occ() == 0
    assert call_occ(npts=0) == _lib.ERR_ARG
    assert call_occ(nsites=0) == _lib.ERR_ARG
    assert call_occ(kind=-1) == _lib.ERR_ARG
    assert call_occ(x_=None) == _lib.ERR_ARG
    assert call_occ(w_=None) == _lib.ERR_ARG
    assert call_occ(out=None) == _lib.ERR_ARG
    assert call_occ() == 0
    rec.close()


def test_resident_compacted_chains_refuse_caller_terminators():
    pairs = np.array([(1, 1), (1, 2)], np.int32)
    rec, g, ene, nv1, dpar = setup(pairs, lld=6, channels=40)
    ai = np.zeros((18, 18, 8), order="F")
    x, w = gauss_legendre(5)
    with pytest.raises(_lib.RsrecError) as ei:
        Exchange(rec, g).contour(x, w, -0.1, random_dmat(2), resident=True, a_inf=ai, b_inf=ai)
    assert ei.value.code == _lib.ERR_ARG and "terminators" in str(ei.value)
    Exchange(rec, g).contour(x, w, -0.1, random_dmat(2), resident=True)      # the handle still works, with the device terminator
    rec.close()


@pytest.mark.parametrize("kind", ["block", "chebyshev"])
def test_exchange_is_unchanged_by_a_contour_call(kind):
    """rsrec_exchange after the contour call on the same handle gives the bits from before it."""
    rec, g, ene, nv1, dpar = setup(PAIRS, lld=6, channels=100, kind=kind)
    ex = Exchange(rec, g)
    before = ex.compute(-0.05, nv1, dpar, kind=kind, resident=True)
    x, w = gauss_legendre(64)
    ex.contour(x, w, float(ene[50]), random_dmat(len(PAIRS)), kind=kind, resident=True)
    after = ex.compute(-0.05, nv1, dpar, kind=kind, resident=True)
    rec.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["contour_block", "contour_cheb"])
def test_matches_the_compiled_reference(name):
    """The fixtures of the compiled reference's own routines (tools/contour_fixture): Exchange.contour and Green.contour_occupation on the
    reference's coefficients against its T_comm_xc and its block_green_eta / chebyshev_green_eta diagonals, under the rule of
    test_contour_oracle.py; block with the device terminator and with the reference's a_inf / b_inf."""
    from helpers import load_golden
    z = load_golden(name)
    kind = "block" if int(z["kind"]) == 0 else "chebyshev"
    pairs = np.asarray(z["pairs"], np.int32)
    p = supercell_problem((4, 4, 4))
    ham, lat, ctl, en = objects_from(p, [1], int(z["lld"]), emin=float(z["emin"]), emax=float(z["emax"]))
    lat.ijpair = pairs
    rec = Recursion(ham, lat, ctl, en)
    e0 = float(z["ene"][int(z["fermi_point"]) - 1])
    x, w = gauss_legendre(64)
    assert np.array_equal(x, z["x"]) and np.array_equal(w, z["w"])
    g = Green(rec, z["ene"])
    coef = (z["a_b"], z["b_sqrt"]) if kind == "block" else (z["mu_n"],)
    terms = [(None, None)] + ([(z["a_inf"], z["b_inf"])] if kind == "block" else [])
    for a_inf, b_inf in terms:
        xc, rows = Exchange(rec, g).contour(x, w, e0, z["dmat"], kind=kind, rows=True, coef=coef, a_inf=a_inf, b_inf=b_inf)
        occ, gd = g.contour_occupation(x, w, e0, kind=kind, diag=True, coef=coef, a_inf=a_inf, b_inf=b_inf)
        for q in range(len(pairs)):
            scale = max(np.abs(z["xc"][:, q]).max(), np.abs(rows[:, :, q]).max() * 1.0e3 / 4.0 / PI)
            dev = np.abs(xc[:, q] - z["xc"][:, q]).max() / scale
            ref = z["gdiag"][..., q]
            dg = np.abs(gd[..., 4 * q:4 * q + 4] - ref).max() / np.abs(ref).max()
            print("%s pair %d (%s terminator): xc deviation / scale %.2e, diagonal deviation / scale %.2e"
                  % (name, q, "device" if a_inf is None else "reference", dev, dg))
            assert dev <= TOL and dg <= TOL
            y = (ref.real * w[None, :, None]) / (x * x)[None, :, None]
            assert occ_close(occ[:, 4 * q:4 * q + 4], occupation(ref, x, w), y)
    rec.close()
