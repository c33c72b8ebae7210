"""rsrec_chebyshev_evolve on the GPU: psi(t) = sum of steps of sum_n w_n T_n(H~), chi(t) with the source term D p_n, the projection of
psi on the seed and the Chebyshev moments of chi per record.

Reference for values: the dense numpy restatement tests/evolve_reference.py (held to the C oracle and to an eigen-decomposition by
tests/test_evolve_restatement.py), judged at helpers.RTOL of the magnitude sums it propagates through the steps -- sum_n |w_n| |p_n| and
so on with |H~|, |D| and the magnitudes of the state -- the largest of every 18 x 18 block, the convention of test_gpu_kubo_shot.py.  Those
sums outgrow the values from korder 13 on, so every output is also held to 1e-12 of its largest value (assert_blocks; measured 2.2e-16
to 1.1e-15), and the ratio is printed.  Shapes: the ragged 75-atom lattice of kubo_cases (75 * 324 elements is no multiple of a workgroup's
tile; 18 * 75 = 2 mod 4: the Gram's last k-step ends in the zero block) with random non-Hermitian operators, a = 60, three random-phase
vectors and kubo_vbatch = 2 (the last batch is partial); and, as the Hermitian anchor, the 4 x 4 x 8 alloy cell with real
evolution_weights and D from position_commutator."""

import numpy as np
import pytest

import evolve_reference as E
from helpers import RTOL, load_golden
from kubo_cases import KK_ODD, ptr, ragged_case, torch_first  # noqa: F401  (torch_first: autouse fixture)
from lattice_seed_reference import alloy_case
from pair_direct_reference import dense_h
from rslmtoasa_amd import _lib
from rslmtoasa_amd.recursion import evolution_order, evolution_weights, position_commutator
from test_gpu_lattice_seed import make_rec

pytestmark = pytest.mark.gpu

DIAG = np.arange(18)
MOM = 19
OUTS = ("ret", "m0_full", "m0_diag", "m_full", "m_diag")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


def random_w(korder, seed=3):
    rng = np.random.default_rng(seed + korder)
    w = rng.standard_normal(korder) + 1j * rng.standard_normal(korder)
    return np.ascontiguousarray(w * (1.5 / np.abs(w).sum()))


def evolve(c, w, nt, stride, mom, vecs=None, want=None, dest="host", seeds=None, d_op="case", do_op="case", korder=None, w_ptr=True, a=None, nseed=None,
           seed_ptrs=(True, True), nvec=None, fill=0.0):
    """rsrec_chebyshev_evolve on the case's vectors with D = the case's v_b / vo_b: (rc, dict of the outputs asked for).  ``want``: the
    outputs (default: ret, and all four moment outputs if mom > 0)."""
    rec = c.rec
    sel = slice(None) if vecs is None else vecs
    sd, cf = (np.ascontiguousarray(c.seeds[sel]), np.ascontiguousarray(c.coefs[sel])) if seeds is None else seeds
    nv = sd.shape[0]
    if want is None:
        want = OUTS if mom > 0 else ("ret",)
    shapes = {"ret": (18, 18, nt, nv), "m0_full": (18, 18, mom, nv), "m0_diag": (18, mom, nv), "m_full": (18, 18, mom, nt, nv), "m_diag": (18, mom, nt, nv)}

    def alloc(shape):
        shape = tuple(max(int(q), 0) for q in shape)
        if dest == "host":
            return np.full(shape, fill, np.complex128, order="F")
        import torch
        return torch.full(shape[::-1], fill, dtype=torch.complex128, device="cuda")
    out = {k: alloc(shapes[k]) for k in want}
    dop = c.ops[2] if isinstance(d_op, str) else d_op
    doo = c.ops[3] if isinstance(do_op, str) else do_op
    rc = rec._L.rsrec_chebyshev_evolve(rec._h, nv if nvec is None else nvec, sd.shape[1] if nseed is None else nseed, ptr(sd) if seed_ptrs[0] else None,
                                       ptr(cf) if seed_ptrs[1] else None, c.a if a is None else a, c.b, ptr(dop), ptr(doo), len(w) if korder is None else korder,
                                       ptr(w) if w_ptr else None, nt, stride, mom, *[ptr(out.get(k)) for k in OUTS])

    def host(x):
        if isinstance(x, np.ndarray):
            return x
        import torch
        torch.cuda.synchronize()
        return x.cpu().numpy().transpose(tuple(range(x.ndim))[::-1])
    return rc, {k: host(v) for k, v in out.items()}


class Shared:
    """A ragged lattice with D = its v_b / vo_b, kubo_vbatch = 2, and the restated calls, computed once each and left unchanged."""

    def __init__(self, hoh):
        self.hoh = hoh
        self.c = ragged_case(hoh)
        self.c.rec.set_option("kubo_vbatch", 2)
        p, ops, seeds, coefs = E.ragged_problem(hoh)
        assert np.array_equal(coefs, self.c.coefs) and np.array_equal(ops[1], self.c.ops[2])
        self.H, self.D = dense_h(p), E.dense_operator(p, ops[1], ops[3])
        self.cache = {}

    def ref(self, korder, nt, stride):
        """the restated call with random_w(korder) and mom = MOM: six single steps restated once per korder, of which a call with
        (nt, stride), nt * stride <= 6, takes every stride-th record"""
        if korder not in self.cache:
            c = self.c
            r = E.evolve(self.H, self.D, c.a, c.b, c.seeds, c.coefs, random_w(korder), 6, 1, MOM)
            for v in r.values():
                v.setflags(write=False)
            self.cache[korder] = r
        take = np.arange(1, nt + 1) * stride - 1
        return {k: (v if k.startswith("m0") else np.take(v, take, axis=-2)) for k, v in self.cache[korder].items()}


@pytest.fixture(scope="module")
def shared():
    cases = {hoh: Shared(hoh) for hoh in (False, True)}
    yield cases
    for s in cases.values():
        s.c.rec.close()


SHARP = 1e-12


def assert_blocks(got, ref, mag, what):
    """every 18 x 18 block within RTOL of the largest magnitude sum of the block, and the whole output within SHARP of its largest value.
    The magnitude sums grow with every order and step (from korder 13 on they exceed the values by orders of magnitude), so the second
    bound is the one that bites there.  It comes from the lengths of the sums, not from what the library gives: a value is reached through
    at most 6 steps of 37 orders and a Gram over 18 * 128 rows, each adding a few units of 1.1e-16 of the largest value in both routes --
    below 1e-13 if every one of them added up, so 1e-12 leaves a factor of ten."""
    dev = np.abs(got - ref).max(axis=(0, 1))
    bound = mag.real.max(axis=(0, 1))
    scale = np.abs(ref).max()
    print("%s: worst |x - ref| / magnitude sum %.2e, / max|x| %.2e" % (what, (dev / bound).max(), dev.max() / scale))
    assert np.all(dev <= RTOL * bound), (what, float((dev / bound).max()))
    assert dev.max() <= SHARP * scale, (what, float(dev.max() / scale))


@pytest.mark.parametrize("korder", [2, 13, 37])
@pytest.mark.parametrize("kernels", [2, 1])
@pytest.mark.parametrize("hoh", [False, True])
def test_values_against_the_restatement(hoh, kernels, korder, shared):
    S = shared[hoh]
    c, rec = S.c, S.c.rec
    w = random_w(korder)
    rec.set_option("kernels", kernels)
    try:
        for nt, stride in ((1, 1), (3, 2)):
            R = S.ref(korder, nt, stride)
            for mom in (0, 1, 2, MOM):
                rc, out = evolve(c, w, nt, stride, mom)
                t = rec.timing()
                assert rc == 0, c.last_error()
                what = "hoh=%d kernels=%d korder=%d nt=%d stride=%d mom=%d" % (hoh, kernels, korder, nt, stride, mom)
                assert_blocks(out["ret"], R["ret"], R["ret_mag"], what + " ret")
                # two batches (2 + 1 vectors): korder - 1 H products and as many D products per step, mom - 1 H products per moment stage
                per_h, per_d = (2, 3) if hoh else (1, 1)
                assert t["hop_launches"] == 2 * (nt * stride * (korder - 1) * (per_h + per_d) + (1 + nt) * max(mom - 1, 0) * per_h), what
                assert abs(t["evolve_pass_ms"] + t["evolve_record_ms"] - t["rest_ms"]) <= 1e-9
                assert t["evolve_pass_ms"] > 0 and t["evolve_record_ms"] > 0 and t["hop_ms"] > 0 and t["total_ms"] >= t["hop_ms"]
                if mom == 0:
                    continue
                assert_blocks(out["m0_full"], R["m0_full"][:, :, :mom], R["m0_mag"][:, :, :mom], what + " m0")
                assert_blocks(out["m_full"], R["m_full"][:, :, :mom], R["m_mag"][:, :, :mom], what + " m")
                assert same_bits(out["m_diag"], out["m_full"][DIAG, DIAG]) and same_bits(out["m0_diag"], out["m0_full"][DIAG, DIAG])
    finally:
        rec.set_option("kernels", 0)


def test_hermitian_anchor_on_the_alloy_cell():
    """real weights of exp(-i H tau), D = [X, H]: one random-phase vector, nt = 2; then a one-atom seed, whose tr ret is tr U_jj(t)"""
    dims, p, H, a, b, emin, emax, cr, cell = alloy_case(False)
    sv = load_golden("bccFe_nsp2_block")["slot_vec"]
    d_op = position_commutator(p["ee"], sv, (0.0, 1.0, 1.0), alat=1.0)
    Dm = E.dense_operator(p, d_op)
    tau = 8.0 / a
    w = evolution_weights(tau, evolution_order(tau, a), a, b)
    kk = H.shape[0] // 18
    rng = np.random.default_rng(12)
    cases = [(np.arange(1, kk + 1, dtype=np.int32)[None, :], (np.exp(2j * np.pi * rng.random(kk)) / np.sqrt(kk))[None, :]),
             (np.array([[37]], np.int32), np.ones((1, 1), np.complex128))]
    rec = make_rec(p, 4, emin, emax)
    try:
        for seeds, coefs in cases:
            R = E.evolve(H, Dm, a, b, seeds, coefs, w, 2, 1, 4)
            got = rec.evolve(d_op, w, 2, stride=1, mom=4, seeds=seeds, coefs=coefs, blocks=True)
            what = "alloy cell, %d seed(s)" % seeds.shape[1]
            for key in ("ret", "m0_full", "m_full"):
                assert_blocks(got[key], R[key], R[key.split("_")[0] + "_mag"], "%s %s" % (what, key))
            assert same_bits(got["m_diag"], got["m_full"][DIAG, DIAG])
            tr, tr_ref = np.trace(got["ret"], axis1=0, axis2=1), np.trace(R["ret"], axis1=0, axis2=1)
            print("%s: tr ret %s, restated %s" % (what, tr.ravel(), tr_ref.ravel()))
            assert np.all(np.abs(tr - tr_ref) <= 18 * RTOL * R["ret_mag"].real.max())
            # chi^H chi is Hermitian and positive, and grows while the packet spreads
            m1 = got["m_full"][:, :, 0, :, 0]
            assert np.all(np.trace(m1, axis1=0, axis2=1).real > 0) and np.trace(m1[:, :, 1]).real > np.trace(m1[:, :, 0]).real
    finally:
        rec.close()


@pytest.mark.parametrize("hoh", [False, True])
def test_bits(hoh, shared):
    S = shared[hoh]
    c, rec = S.c, S.c.rec
    korder, nt, stride = 13, 2, 2
    w = random_w(korder)
    rc, base = evolve(c, w, nt, stride, MOM)
    assert rc == 0, c.last_error()

    def same(out, ref=None, keys=OUTS):
        ref = base if ref is None else ref
        return all(same_bits(out[k], ref[k]) for k in keys if k in out)
    rc, out = evolve(c, w, nt, stride, MOM)
    assert rc == 0 and same(out), "run to run"
    for vb in (1, 4):
        rec.set_option("kubo_vbatch", vb)
        try:
            rc, out = evolve(c, w, nt, stride, MOM)
        finally:
            rec.set_option("kubo_vbatch", 2)
        assert rc == 0 and same(out), "kubo_vbatch=%d" % vb
    for orders in (1, 2, 5, 16):
        rec.set_option("evolve_orders", orders)
        try:
            rc, out = evolve(c, w, nt, stride, MOM)
        finally:
            rec.set_option("evolve_orders", 0)
        assert rc == 0 and same(out), "evolve_orders=%d" % orders
    rec.set_option("evolve_orders", 16)
    try:
        w37 = random_w(37)
        rc, deep = evolve(c, w37, 1, 1, 2)
        rec.set_option("evolve_orders", 1)
        rc1, fused = evolve(c, w37, 1, 1, 2)
    finally:
        rec.set_option("evolve_orders", 0)
    assert rc == 0 and rc1 == 0 and same(deep, fused), "korder 37: two full batched passes and a short one against the fused pass"
    rc, out = evolve(c, w, nt, stride, MOM, vecs=slice(2, 3))
    assert rc == 0 and all(same_bits(out[k][..., 0], base[k][..., 2]) for k in OUTS), "vector 2 alone"
    rc, out = evolve(c, w, nt, stride, MOM, vecs=slice(None, None, -1))
    assert rc == 0 and all(same_bits(out[k][..., ::-1], base[k]) for k in OUTS), "vectors in reverse order"
    rc, out = evolve(c, w, nt, stride, MOM, dest="device")
    assert rc == 0 and same(out), "device outputs"
    rc, out = evolve(c, w, nt, stride, MOM, want=("m_diag",))
    assert rc == 0 and same(out), "m_diag alone"
    rc, out = evolve(c, w, nt, stride, MOM, want=("ret", "m0_diag"))
    assert rc == 0 and same(out), "ret and m0_diag alone"
    assert same_bits(base["m_diag"], base["m_full"][DIAG, DIAG]) and same_bits(base["m0_diag"], base["m0_full"][DIAG, DIAG])
    rc, longer = evolve(c, w, 3, stride, MOM)
    assert rc == 0 and same_bits(longer["m0_full"], base["m0_full"]), "m0 does not depend on nt"
    assert all(same_bits(longer[k][..., :nt, :], base[k]) for k in ("ret", "m_full", "m_diag")), "records 1..s of a longer call"
    rc, one = evolve(c, w, 1, 2, MOM)
    rc2, two = evolve(c, w, 2, 1, MOM)
    assert rc == 0 and rc2 == 0 and all(same_bits(one[k][..., 0, :], two[k][..., 1, :]) for k in ("ret", "m_full", "m_diag")), "(nt=1, stride=2) is record 2 of (nt=2, stride=1)"
    c.diag(9)                                                        # another call's data in the Kubo buffers
    rc, out = evolve(c, w, nt, stride, MOM)
    assert rc == 0 and same(out), "after rsrec_kubo_moments_diag"


def test_long_run_folds_its_timing_events(shared):
    """12 steps of 37 orders with hoh in two batches: more than 8192 timing events, so the call folds them into its sums on the way and
    gives them back -- the launch count and the sums stay those of the whole call, and the bits those of a short call"""
    S = shared[True]
    c, rec = S.c, S.c.rec
    w = random_w(37)
    rc, out = evolve(c, w, 4, 3, 0)
    t = rec.timing()
    assert rc == 0, c.last_error()
    assert t["hop_launches"] == 2 * (12 * 36 * 5)
    assert abs(t["evolve_pass_ms"] + t["evolve_record_ms"] - t["rest_ms"]) <= 1e-9
    assert 0 < t["hop_ms"] <= t["total_ms"] and 0 < t["evolve_pass_ms"] < t["total_ms"]
    rc, short = evolve(c, w, 1, 3, 0)
    assert rc == 0 and same_bits(short["ret"][:, :, 0], out["ret"][:, :, 0])


@pytest.mark.parametrize("hoh", [False, True])
def test_cross_checks(hoh, shared):
    S = shared[hoh]
    c, rec = S.c, S.c.rec
    w = random_w(13)
    zero = np.zeros_like(c.ops[2])
    rc, out = evolve(c, w, 2, 1, 5, d_op=zero, do_op=zero if hoh else None, fill=7.0)
    assert rc == 0, c.last_error()
    assert not out["m_full"].any() and not out["m_diag"].any(), "d_op = 0: chi stays an exact zero"
    assert np.abs(out["m0_full"]).max() > 0
    unit = np.zeros(13, np.complex128)
    unit[0] = 1.0
    rc, out = evolve(c, unit, 3, 2, 0)
    assert rc == 0, c.last_error()
    gram = np.einsum("vk,ab->abv", np.abs(c.coefs) ** 2, np.eye(18))                  # r^H r = sum_j |c_j|^2 1
    for s in range(3):
        assert np.abs(out["ret"][:, :, s] - gram).max() <= 1e-14, "w = (1, 0, ...): ret is the seed Gram at every record"
    lld = 4
    rc, out = evolve(c, w, 1, 1, 2 * lld + 2, want=("m0_full",))
    assert rc == 0, c.last_error()
    m_g = np.zeros((18, 18, 2 * lld + 2, 1, 3), np.complex128, order="F")
    rc = rec._L.rsrec_chebyshev_lattice(rec._h, 3, KK_ODD, ptr(c.seeds), ptr(c.coefs), lld, c.a, c.b, 1, None, ptr(m_g))
    assert rc == 0, c.last_error()
    dev = np.abs(out["m0_full"] - m_g[:, :, :, 0]).max()
    print("hoh=%d m0_full against rsrec_chebyshev_lattice: %.2e of max %.2e" % (hoh, dev, np.abs(m_g).max()))
    assert dev <= RTOL * np.abs(m_g).max()


def test_refusals_leave_the_handle_usable(shared):
    S = shared[True]
    c = S.c
    korder = 13
    w = random_w(korder)
    rc, base = evolve(c, w, 2, 1, 3)
    assert rc == 0, c.last_error()
    nan_w, inf_w = w.copy(), w.copy()
    nan_w[5] = np.nan
    inf_w[0] = complex(0.0, np.inf)
    big_w = np.zeros(_lib.EVOLVE_KORDER_MAX + 1, np.complex128)
    no_seed = (np.zeros((1, 4), np.int32), np.ones((1, 4), np.complex128))
    far_seed = (np.full((1, 1), KK_ODD + 1, np.int32), np.ones((1, 1), np.complex128))
    refusals = [
        ("korder = 1", lambda: evolve(c, w, 2, 1, 3, korder=1)),
        ("korder too large", lambda: evolve(c, big_w, 2, 1, 3)),
        ("nt = 0", lambda: evolve(c, w, 0, 1, 3)),
        ("nt too large", lambda: evolve(c, w, _lib.EVOLVE_NT_MAX + 1, 1, 0)),
        ("stride = 0", lambda: evolve(c, w, 2, 0, 3)),
        ("stride too large", lambda: evolve(c, w, 2, _lib.EVOLVE_STRIDE_MAX + 1, 3)),
        ("mom < 0", lambda: evolve(c, w, 2, 1, -1, want=("ret",))),
        ("mom too large", lambda: evolve(c, w, 1, 1, _lib.EVOLVE_MOM_MAX + 1, want=("ret",))),
        ("w NULL", lambda: evolve(c, w, 2, 1, 3, w_ptr=False)),
        ("d_op NULL", lambda: evolve(c, w, 2, 1, 3, d_op=None)),
        ("hoh without do_op", lambda: evolve(c, w, 2, 1, 3, do_op=None)),
        ("NaN weight", lambda: evolve(c, nan_w, 2, 1, 3)),
        ("Inf weight", lambda: evolve(c, inf_w, 2, 1, 3)),
        ("every output NULL", lambda: evolve(c, w, 2, 1, 3, want=())),
        ("moment output with mom = 0", lambda: evolve(c, w, 2, 1, 0, want=("ret", "m_diag"))),
        ("m0 output with mom = 0", lambda: evolve(c, w, 2, 1, 0, want=("m0_full",))),
        ("nseed = 0", lambda: evolve(c, w, 2, 1, 3, nseed=0)),
        ("seed_atoms NULL", lambda: evolve(c, w, 2, 1, 3, seed_ptrs=(False, True))),
        ("seed_coef NULL", lambda: evolve(c, w, 2, 1, 3, seed_ptrs=(True, False))),
        ("a = 0", lambda: evolve(c, w, 2, 1, 3, a=0.0)),
        ("nvec < 0", lambda: evolve(c, w, 2, 1, 3, nvec=-1)),
        ("vector without a seed", lambda: evolve(c, w, 2, 1, 3, seeds=no_seed)),
        ("seed atom outside the lattice", lambda: evolve(c, w, 2, 1, 3, seeds=far_seed)),
    ]
    for what, call in refusals:
        rc = call()[0]
        assert rc == _lib.ERR_ARG, (what, rc)
        assert b"rsrec_chebyshev_evolve" in c.last_error(), (what, c.last_error())
    none = (np.zeros((0, 1), np.int32), np.zeros((0, 1), np.complex128))
    assert evolve(c, w, 2, 1, 3, seeds=none)[0] == 0                  # nvec = 0
    huge = w.copy()
    huge[1] = 1e300
    rc, out = evolve(c, huge, 2, 1, 3, fill=7.0)
    assert rc == _lib.ERR_DIVERGED and b"rsrec_chebyshev_evolve" in c.last_error()
    assert all(np.all(v == 7.0) for v in out.values()), "a diverged call leaves the outputs alone"
    rc, out = evolve(c, w, 2, 1, 3)
    assert rc == 0 and all(same_bits(out[k], base[k]) for k in OUTS)
    R = S.ref(korder, 2, 1)
    assert_blocks(out["m_full"], R["m_full"][:, :, :3], R["m_mag"][:, :, :3], "after the refusals")
