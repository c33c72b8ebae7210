"""rsrec_exchange (kernels_exchange.hpp) against the numpy restatement of the reference's exchange workflow (exchange_reference.py):
intersite Green functions, the 41 energy-resolved integrands, the Simpson integrals and the cumulative J of fort.150."""
import numpy as np
import pytest

from exchange_reference import PI, combos, simpson_f
from helpers import load_golden, objects_from, supercell_problem
from pair_cases import (check_exchange as check_against, close, exchange_restated as reference, onsite, pair_list, random_contour_dmat,
                        random_tmat, run_device_script, setup)
from rslmtoasa_amd import _lib
from rslmtoasa_amd.exchange import Exchange, gauss_legendre
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.recursion import Recursion

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hoh", [False, True])
def test_block_matches_restatement(hoh):
    rng = np.random.default_rng(7)
    pairs = np.array([(1, 1), (1, 2), (1, 9), (1, 17), (5, 60), (3, 3)], np.int32)
    rec, g, ene, nv1, dpar = setup(pairs, hoh=hoh)
    fermi = -0.05
    out, _ = reference(rec, g, ene, nv1, dpar, fermi, "block", pairs)
    res = Exchange(rec, g).compute(fermi, nv1, dpar, kind="block", integrand=True, cumulative=True, coef=(rec.a_b, rec.b2_b))
    check_against(res, out)
    assert np.abs(res[0][0]).max() > 0 and np.abs(res[-1]).max() > 0
    # the device's cumulative J is the O(nE^2) loop of calculate_exchange_twoindex bit for bit, given the device's own integrand
    for q in range(len(pairs)):
        y, _ = combos(res[-1][:, :, q])
        direct = np.array([simpson_f(y[13:14], ene, ef, nv1)[0] for ef in ene]) * 1.0e3 / 4.0 / PI
        assert np.array_equal(res[4][:, q], direct), q
    rec.close()


def test_chebyshev_matches_restatement():
    pairs = np.array([(1, 1), (1, 2), (2, 9), (4, 33)], np.int32)
    rec, g, ene, nv1, dpar = setup(pairs, kind="chebyshev", lld=12)
    fermi = float(ene[150]) + 0.3 * (ene[1] - ene[0])
    out, _ = reference(rec, g, ene, nv1, dpar, fermi, "chebyshev", pairs)
    res = Exchange(rec, g).compute(fermi, nv1, dpar, kind="chebyshev", integrand=True, cumulative=True)
    check_against(res, out)
    rec.close()


DEVICE_SCRIPT = r"""
from rslmtoasa_amd.exchange import Exchange
if mode == "sources":
    pairs = np.array([(1, 1), (1, 2), (7, 30), (2, 2), (9, 40)], np.int32)
    rec, g, ene, nv1, dpar = T.setup(pairs, lld=8)
    x = Exchange(rec, g)
    fermi = -0.05
    res_dev = x.compute(fermi, nv1, dpar, resident=True, integrand=True, cumulative=True)
    res_dev2 = x.compute(fermi, nv1, dpar, resident=True, integrand=True, cumulative=True)
    rec.zsqr()
    a_inf, b_inf, _, _ = g.terminator(nsites=4 * len(pairs))
    res_host = x.compute(fermi, nv1, dpar, integrand=True, cumulative=True)
    res_host_t = x.compute(fermi, nv1, dpar, integrand=True, cumulative=True, a_inf=a_inf, b_inf=b_inf)
    ta = torch.from_numpy(np.ascontiguousarray(rec.a_b.transpose(3, 2, 1, 0))).cuda()
    tb = torch.from_numpy(np.ascontiguousarray(rec.b2_b.transpose(3, 2, 1, 0))).cuda()
    res_t = x.compute(fermi, nv1, dpar, integrand=True, cumulative=True, coef=(ta, tb))
    for other in (res_dev2, res_host, res_host_t, res_t):
        for a, b in zip(res_dev, other):
            assert np.array_equal(a, b)
    out, _ = T.exchange_restated(rec, g, ene, nv1, dpar, fermi, "block", pairs, zsqr=False)
    T.check_exchange(res_dev, out)
else:
    # 8192 pairs at nE = 2510: g0 of their chains would take 427 GB, more than the device holds
    pairs = np.array([(1, 2)], np.int32)
    rec, g, ene, nv1, dpar = T.setup(pairs, lld=4, channels=2501)
    assert len(ene) == 2510
    rec.zsqr()
    fermi = -0.05
    x = Exchange(rec, g)
    one = x.compute(fermi, nv1, dpar)
    n = 8192
    ta = torch.from_numpy(np.ascontiguousarray(rec.a_b[..., :4].transpose(3, 2, 1, 0))).cuda().repeat(n, 1, 1, 1)
    tb = torch.from_numpy(np.ascontiguousarray(rec.b2_b[..., :4].transpose(3, 2, 1, 0))).cuda().repeat(n, 1, 1, 1)
    rec.lattice.ijpair = np.repeat(pairs, n, axis=0)
    many = x.compute(fermi, nv1, np.repeat(dpar, n, axis=3), coef=(ta, tb))
    for k in range(4):
        assert np.array_equal(many[k], np.repeat(one[k], n, axis=1))
    print("device ms for %d pairs: %.1f" % (n, x.timing()[0]))
rec.close()
print("EXCHANGE_DEVICE_OK")
"""


def test_coefficient_sources_agree_bitwise():
    """Host arrays, device arrays and the chains the last seeded call left on the device (i == j pairs: compacted, as recur_b_ij runs
    them) give the same bits; so do repeated calls.  And they match the restatement."""
    run_device_script(DEVICE_SCRIPT, "sources", "EXCHANGE_DEVICE_OK")


def test_memory_is_bounded_for_8192_pairs():
    """8192 pairs at nE = 2510 and lld 4 finish, and every pair (all the same chains) carries the single-pair result."""
    run_device_script(DEVICE_SCRIPT, "memory", "EXCHANGE_DEVICE_OK")


def test_many_pairs_on_a_supercell():
    rng = np.random.default_rng(11)
    pairs = pair_list(8 * 8 * 8, 220, rng)
    rec, g, ene, nv1, dpar = setup(pairs, lld=6, dims=(8, 8, 8), channels=60)
    fermi = -0.05
    out, _ = reference(rec, g, ene, nv1, dpar, fermi, "block", pairs, cumulative=False)
    res = Exchange(rec, g).compute(fermi, nv1, dpar, integrand=True)
    check_against(res, out, with_jcum=False)
    rec.close()


def test_partitioned_images_sum_to_the_single_call():
    pairs = np.array([(1, 1), (1, 2), (3, 19), (2, 2), (4, 50), (6, 7), (8, 8)], np.int32)
    rec, g, ene, nv1, dpar = setup(pairs, lld=8, channels=100)
    rec.zsqr()
    fermi = -0.05
    whole = Exchange(rec, g).compute(fermi, nv1, dpar)
    parts = []
    for r in range(2):
        rec.rank, rec.nprocs = r, 2
        from rslmtoasa_amd.recursion import site_partition
        s, e = site_partition(r, 2, len(pairs))
        coef = (rec.a_b[..., 4 * (s - 1):4 * e], rec.b2_b[..., 4 * (s - 1):4 * e])
        parts.append(Exchange(rec, g).compute(fermi, nv1, dpar[..., s - 1:e], pair_offset=s - 1, npairs_total=len(pairs), coef=coef))
    rec.rank, rec.nprocs = 0, 1
    for k in range(4):
        assert np.array_equal(parts[0][k] + parts[1][k], whole[k])
    rec.close()


@pytest.mark.parametrize("kind", ["block", "chebyshev"])
@pytest.mark.parametrize("case", ["compute", "damping", "contour", "contour_occupation"])
def test_chunk_caps_give_the_uncapped_bits(case, kind, monkeypatch):
    """RSREC_PAIR_CHUNK = 1, 2 and 4 make these five-pair (three-site) calls run two to five chunks, the last one short: every array they
    return, per-item rows included, carries the bits of the one-chunk call, on the resident chains and on the host coefficient arrays."""
    if case == "contour_occupation":
        rec = onsite(kind, 8)
        x, w = gauss_legendre(8)
        g = Green(rec, np.array([-0.07]))
        call = lambda **kw: g.contour_occupation(x, w, -0.07, kind=kind, diag=True, **kw)
    else:
        pairs = np.array([(1, 1), (1, 2), (7, 30), (2, 2), (9, 40)], np.int32)
        rec, g, ene, nv1, dpar = setup(pairs, lld=8, channels=100, kind=kind)
        ex = Exchange(rec, g)
        x, w = gauss_legendre(8)
        tmat, dmat = random_tmat(len(pairs)), random_contour_dmat(len(pairs))
        call = {"compute": lambda **kw: ex.compute(-0.05, nv1, dpar, kind=kind, integrand=True, cumulative=True, **kw),
                "damping": lambda **kw: ex.damping(tmat, 61, kind=kind, rows=True, **kw),
                "contour": lambda **kw: ex.contour(x, w, float(ene[50]), dmat, kind=kind, rows=True, **kw)}[case]
    one = call(resident=True)
    if kind == "block":
        rec.zsqr()
    one_host = call()
    assert np.abs(one[0]).max() > 0 and np.abs(one_host[0]).max() > 0
    for cap in ("1", "2", "4"):
        monkeypatch.setenv("RSREC_PAIR_CHUNK", cap)
        many, many_host = call(resident=True), call()
        monkeypatch.delenv("RSREC_PAIR_CHUNK")
        assert len(many) == len(one) and len(many_host) == len(one_host)
        for a, b in list(zip(one, many)) + list(zip(one_host, many_host)):
            assert np.array_equal(a, b), cap
    rec.close()


def test_bad_arguments_are_errors():
    pairs = np.array([(1, 2)], np.int32)
    rec, g, ene, nv1, dpar = setup(pairs, lld=6, channels=40)
    L, h = rec._L, rec._h
    import ctypes as C
    same = np.zeros(1, np.int32)
    buf = [np.zeros((13, 1)), np.zeros((13, 1)), np.zeros((13, 1)), np.zeros((28, 1))]
    ab = np.asfortranarray(rec.a_b[..., :4])
    bb = np.asfortranarray(rec.b2_b[..., :4])
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(kind=0, npairs=1, nen=len(ene), outs=buf, same_=same):
        return L.rsrec_exchange(h, kind, npairs, P(same_), 6, nen, P(ene), nv1, -0.05, 0, -0.6, 0.4, None, None, P(ab), P(bb), P(dpar), 0, 1,
                                *[P(o) for o in outs], None, None)
    assert call() == 0
    assert call(npairs=0) == _lib.ERR_ARG
    assert call(npairs=-3) == _lib.ERR_ARG
    assert call(nen=nv1 + 8) == _lib.ERR_ARG
    assert call(kind=2) == _lib.ERR_ARG
    assert call(kind=-1) == _lib.ERR_ARG
    assert call(outs=[None] + buf[1:]) == _lib.ERR_ARG
    assert call(outs=buf[:3] + [None]) == _lib.ERR_ARG
    assert call(same_=None) == _lib.ERR_ARG
    assert call() == 0                                          # the handle still works
    rec.close()


def test_resident_compacted_chains_refuse_caller_terminators():
    """recur_b_ij runs an i == j pair with one chain; caller terminators come in slot order and cannot be matched to that list."""
    pairs = np.array([(1, 1), (1, 2)], np.int32)
    rec, g, ene, nv1, dpar = setup(pairs, lld=6, channels=40)
    ai = np.zeros((18, 18, 8), order="F")
    with pytest.raises(_lib.RsrecError) as ei:
        Exchange(rec, g).compute(-0.05, nv1, dpar, resident=True, a_inf=ai, b_inf=ai)
    assert ei.value.code == _lib.ERR_ARG and "terminators" in str(ei.value)
    Exchange(rec, g).compute(-0.05, nv1, dpar, resident=True)      # the handle still works, with the device terminator
    rec.close()


@pytest.mark.parametrize("name", ["exchange_block", "exchange_cheb", "exchange_cheb_hoh"])
def test_matches_the_compiled_reference(name):
    """rsrec_exchange on the reference's pair coefficients against the compiled reference's own exchange flow (tools/exchange_fixture):
    T_comm_xc, the first-order values and the parts at full precision, fort.150's cumulative J.  Terminators from the device."""
    z = load_golden(name)
    pairs = np.asarray(z["pairs"], np.int32)
    p = supercell_problem((4, 4, 8))
    ham, lat, ctl, en = objects_from(p, [1], int(z["lld"]), emin=float(z["emin"]), emax=float(z["emax"]))
    lat.ijpair = pairs
    rec = Recursion(ham, lat, ctl, en)
    g = Green(rec, z["ene"])
    coef = (z["a_b"], z["b_sqrt"]) if str(z["kind"]) == "block" else (z["mu_n"],)
    xc, so, fo, parts, jcum = Exchange(rec, g).compute(float(z["fermi"]), int(z["nv1"]), z["dpar"], kind=str(z["kind"]), cumulative=True, coef=coef)
    for q in range(len(pairs)):
        floor = max(np.abs(z["xc"][:, q]).max(), np.abs(z["fo"][:, q]).max(), np.abs(z["parts"][:, q]).max()) * 1e-2
        assert close(xc[:, q], z["xc"][:, q], floor) and close(fo[:, q], z["fo"][:, q], floor) and close(parts[:, q], z["parts"][:, q], floor), q
        assert close(jcum[:, q], z["fort150"][:, 1, q], 0.0), q
    rec.close()
