"""rsrec_kubo_single_shot on the GPU: s(:, :, e, v, j) = sum_{n,m} wl(m, e) wr(n, e) mu_j(:, :, n, m, v) without the moments.

Reference for values: the C oracle's moments (oracle.kubo_moments, independent of the code under test) contracted with the weights in
numpy, judged at helpers.RTOL of the magnitude sum sum_{nm} |wl(m, e)| |wr(n, e)| |mu(n, m)| of a block (its largest element): the
rounding of both routes is bounded by about (cond_ll + 18 kk) eps of that sum, orders below 1e-10 at these sizes.  The ratio to max|s|
and the deviation from the library's own rsrec_kubo_moments, contracted the same way, are printed.  The end-to-end cases are anchored on
the compiled reference's mu_nm in tests/golden/fccPt_kubo*.npz.  Shapes: the ragged 75-atom lattice of kubo_cases (18 * 75 = 2 mod 4: the
Gram's last k-step ends in the zero block) and the 512-atom fixtures."""
import ctypes as C

import numpy as np
import pytest

import cond_reference as R
from helpers import RTOL, load_golden, random_problem, random_vec_coefficients
from kubo_cases import KK_ODD, Ragged, ptr, stack, torch_first  # noqa: F401  (torch_first: autouse fixture)
from rslmtoasa_amd import _lib
from rslmtoasa_amd.conductivity import Conductivity
from rslmtoasa_amd.recursion import Energy, kubo_bastin_weights, kubo_greenwood_weights
from test_gpu_conductivity import make_rec, window

pytestmark = pytest.mark.gpu

LL = 13                # odd: every P in {2, 5, 16} ends on a short pass
LL_DEEP = 37           # shot_orders = 16: two full passes + 5
DIAG = np.arange(18)


def same_bits(a, b):
    """the same shape and, element by element, the same bits, whatever the memory order of either array"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


def ragged_problem(hoh):
    """the operator kubo_cases.ragged_case builds (the first draws of its generator), for the oracle"""
    rng = np.random.default_rng(4242 + int(hoh))
    p = random_problem(rng, KK_ODD, 5, 2, 0, hoh, False)
    if hoh:
        p["eeo"] = np.asfortranarray(p["eeo"] * 0.1)
    return p


def random_weights(seed, ll, ne):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((2, ll, ne)) + 1j * rng.standard_normal((2, ll, ne))
    return np.asfortranarray(w[0]), np.asfortranarray(w[1])


def shot(c, outs, wl, wr, vecs=None, full="host", diag="host", nout=None, ne=None, cond_ll=None, v_b="case", wl_ptr="given", wr_ptr="given", seeds=None, a=None, nseed=None, seed_ptrs=(True, True), nvec=None):
    """rsrec_kubo_single_shot on the case's vectors with output operators outs = [(v, vo), ...]: (rc, s_full, s_diag)"""
    rec = c.rec
    sel = slice(None) if vecs is None else vecs
    sd, cf = (np.ascontiguousarray(c.seeds[sel]), np.ascontiguousarray(c.coefs[sel])) if seeds is None else seeds
    nvec_arg = sd.shape[0] if nvec is None else nvec
    nvec = sd.shape[0]
    nseed_arg = sd.shape[1] if nseed is None else nseed
    v_out, vo_out = (stack([o[0] for o in outs]), stack([o[1] for o in outs])) if outs else (None, None)
    ll, nw = wl.shape
    no = len(outs) if nout is None else nout

    def alloc(kind, shape):
        if kind is None:
            return None
        if kind == "host":
            return np.zeros(shape, np.complex128, order="F")
        import torch
        return torch.zeros(shape[::-1], dtype=torch.complex128, device="cuda")
    s_full, s_diag = alloc(full, (18, 18, nw, nvec, max(no, 1))), alloc(diag, (18, nw, nvec, max(no, 1)))
    vb = c.ops[2] if isinstance(v_b, str) else v_b
    rc = rec._L.rsrec_kubo_single_shot(rec._h, no, nvec_arg, nseed_arg, ptr(sd) if seed_ptrs[0] else None, ptr(cf) if seed_ptrs[1] else None,
                                       ll if cond_ll is None else cond_ll, c.a if a is None else a, c.b, ptr(v_out), ptr(vo_out), ptr(vb), ptr(c.ops[3]),
                                       nw if ne is None else ne, ptr(wl) if wl_ptr == "given" else None, ptr(wr) if wr_ptr == "given" else None,
                                       ptr(s_full), ptr(s_diag))

    def host(x):
        if x is None or isinstance(x, np.ndarray):
            return x
        import torch
        torch.cuda.synchronize()
        return x.cpu().numpy().transpose(tuple(range(x.ndim))[::-1])
    return rc, host(s_full), host(s_diag)


def contract(mu, wl, wr):
    """(s, magnitude sum) of moments mu (18, 18, n, m, v) with weights (ll, ne): both (18, 18, ne, v)"""
    ll = wl.shape[0]
    m = mu[:, :, :ll, :ll]
    return np.einsum("me,ne,abnmv->abev", wl, wr, m), np.einsum("me,ne,abnmv->abev", np.abs(wl), np.abs(wr), np.abs(m))


def assert_blocks(s, ref, mag, what):
    """every 18 x 18 block within RTOL of the largest magnitude sum of the block"""
    dev = np.abs(s - ref).max(axis=(0, 1))
    bound = mag.max(axis=(0, 1))
    print("%s: worst |s - ref| / magnitude sum %.2e, / max|s| %.2e" % (what, (dev / bound).max(), (dev / np.abs(ref).max(axis=(0, 1))).max()))
    assert np.all(dev <= RTOL * bound), (what, float((dev / bound).max()))


class Shared:
    """A ragged lattice with its three output operators and the oracle's moments of each, computed once and left unchanged."""

    def __init__(self, hoh, oracle_lib):
        self.hoh = hoh
        self.r = Ragged(hoh, 977, False)
        self.c = self.r.c
        self.outs = self.r.outs
        self.oracle = oracle_lib.Oracle(ragged_problem(hoh))
        self.cache = {}

    def moments(self, j, ll, vecs=slice(None)):
        key = (j, ll, str(vecs))
        if key not in self.cache:
            c, (v, vo) = self.c, self.outs[j]
            mu = self.oracle.kubo_moments(c.seeds[vecs], c.coefs[vecs], ll, c.a, c.b, v, c.ops[2], vo, c.ops[3])
            mu.setflags(write=False)
            self.cache[key] = mu
        return self.cache[key]

    def library_moments(self, j, ll):
        c, keep = self.c, self.c.ops
        c.ops = [self.outs[j][0], self.outs[j][1]] + keep[2:]
        try:
            return c.full(ll)
        finally:
            c.ops = keep


@pytest.fixture(scope="module")
def shared(oracle_lib):
    cases = {hoh: Shared(hoh, oracle_lib) for hoh in (False, True)}
    yield cases
    for s in cases.values():
        s.c.rec.close()


@pytest.mark.parametrize("kernels", [2, 1])
@pytest.mark.parametrize("hoh", [False, True])
def test_ragged_random_weights(hoh, kernels, shared):
    S = shared[hoh]
    c, rec = S.c, S.c.rec
    wl, wr = random_weights(11, LL, 3)
    rec.set_option("kernels", kernels)
    try:
        rc, s_full, s_diag = shot(c, S.outs[:2], wl, wr)
        t = rec.timing()
    finally:
        rec.set_option("kernels", 0)
    assert rc == 0, c.last_error()
    assert s_full.shape == (18, 18, 3, 3, 2) and s_diag.shape == (18, 3, 3, 2)
    assert same_bits(s_diag, s_full[DIAG, DIAG])
    for j in range(2):
        ref, mag = contract(S.moments(j, LL), wl, wr)
        assert_blocks(s_full[..., j], ref, mag, "hoh=%d kernels=%d out %d vs oracle" % (hoh, kernels, j))
        own = contract(S.library_moments(j, LL), wl, wr)[0]
        print("   vs the library's own rsrec_kubo_moments: %.2e of the magnitude sum" % (np.abs(s_full[..., j] - own).max(axis=(0, 1)) / mag.max(axis=(0, 1))).max())
    # one batch of nb = 3 vectors, nout = 2, ne = 3 <= 8 (include/rsrec.h)
    assert t["hop_launches"] == (2 * LL + 1 + 3 * (1 + 2 * 2) if hoh else LL + 3 * 2)
    assert abs(t["shot_accum_ms"] + t["shot_final_ms"] - t["rest_ms"]) <= 1e-9
    assert t["shot_accum_ms"] > 0 and t["shot_final_ms"] > 0 and t["hop_ms"] > 0 and t["total_ms"] >= t["hop_ms"]


@pytest.mark.parametrize("hoh", [False, True])
def test_bits_depend_on_own_column_vector_and_operator_only(hoh, shared):
    S = shared[hoh]
    c, rec = S.c, S.c.rec
    wl, wr = random_weights(11, LL, 3)
    rc, base, base_d = shot(c, S.outs[:2], wl, wr)
    assert rc == 0, c.last_error()
    for P in (1, 2, 5, 16):
        rec.set_option("shot_orders", P)
        try:
            rc, s, d = shot(c, S.outs[:2], wl, wr)
        finally:
            rec.set_option("shot_orders", 0)
        assert rc == 0 and same_bits(s, base) and same_bits(d, base_d), "shot_orders=%d" % P
    rec.set_option("kubo_vbatch", 1)
    try:
        rc, s, d = shot(c, S.outs[:2], wl, wr)
    finally:
        rec.set_option("kubo_vbatch", 0)
    assert rc == 0 and same_bits(s, base) and same_bits(d, base_d), "kubo_vbatch=1"
    rc, s, d = shot(c, S.outs[:2], np.asfortranarray(wl[:, 2:3]), np.asfortranarray(wr[:, 2:3]))
    assert rc == 0 and same_bits(s[:, :, 0], base[:, :, 2]) and same_bits(d[:, 0], base_d[:, 2]), "column 2 alone"
    rc, s, d = shot(c, S.outs[:2], wl, wr, vecs=slice(2, 3))
    assert rc == 0 and same_bits(s[:, :, :, 0], base[:, :, :, 2]) and same_bits(d[:, :, 0], base_d[:, :, 2]), "vector 2 alone"
    rc, s, d = shot(c, S.outs[1::-1], wl, wr)
    assert rc == 0 and same_bits(s[..., ::-1], base) and same_bits(d[..., ::-1], base_d), "output operators swapped"
    rc, s, d = shot(c, S.outs[:2], wl, wr, full="device", diag="device")
    assert rc == 0 and same_bits(s, base) and same_bits(d, base_d), "device outputs"
    rc, s, d = shot(c, S.outs[:2], wl, wr, full=None)
    assert rc == 0 and s is None and same_bits(d, base_d), "s_diag alone"
    rc, s, d = shot(c, S.outs[:2], wl, wr)
    assert rc == 0 and same_bits(s, base) and same_bits(d, base_d), "two identical calls"
    c.diag(LL + 4)                                                   # another call's data in the Kubo buffers
    rc, s, d = shot(c, S.outs[:2], wl, wr)
    assert rc == 0 and same_bits(s, base) and same_bits(d, base_d), "after rsrec_kubo_moments_diag"


@pytest.mark.parametrize("cond_ll", [1, 2, LL_DEEP])
def test_depth_and_width_edges(cond_ll, shared):
    """shot_orders = 16, ne = 16 (two launches of 8 columns in the final stage), nout = 3, one vector"""
    S = shared[False]
    c, rec = S.c, S.c.rec
    wl, wr = random_weights(23, cond_ll, 16)
    rec.set_option("shot_orders", 16)
    try:
        rc, s_full, s_diag = shot(c, S.outs, wl, wr, vecs=slice(0, 1))
        t = rec.timing()
    finally:
        rec.set_option("shot_orders", 0)
    assert rc == 0, c.last_error()
    assert s_full.shape == (18, 18, 16, 1, 3) and same_bits(s_diag, s_full[DIAG, DIAG])
    assert t["hop_launches"] == cond_ll + 1 * 3 * 2
    for j in range(3):
        ref, mag = contract(S.moments(j, LL_DEEP, slice(0, 1)), wl, wr)
        assert_blocks(s_full[..., j], ref, mag, "cond_ll=%d out %d" % (cond_ll, j))


def pinned_scaling(z):
    """the fixture's a, b to the last bit, as test_end_to_end_gpu_moments_then_integrand pins them"""
    import rslmtoasa_amd.recursion as Rm
    orig = Rm.chebyshev_scaling
    Rm.chebyshev_scaling = lambda e0, e1: (float(z["acheb"]), float(z["bcheb"]))
    return Rm, orig


def inside(emin, emax, n):
    de = emax - emin
    return np.concatenate([[emin + 0.015 * de], np.linspace(emin + 0.13 * de, emax - 0.21 * de, n - 2), [emax - 0.012 * de]])


@pytest.mark.parametrize("name,cond_ll,nvec", [("fccPt_kubo", 10, None), ("fccPt_kubo_hoh", 10, None), ("fccPt_kubo_random", 6, 2)])
def test_integrand_at_matches_the_compiled_reference(name, cond_ll, nvec):
    z = load_golden(name)
    emin, emax = window(z)
    ene = inside(emin, emax, 8)
    rec = make_rec(z, Energy(emin, emax))
    if "rng" in z:
        seeds, coefs = random_vec_coefficients(z["rng"])
        vectors = dict(seeds=seeds[:nvec], coefs=coefs[:nvec])
    else:
        vectors = dict(atlist=z["atlist"])
    Rm, orig = pinned_scaling(z)
    try:
        got = Conductivity(rec).integrand_at(z["v_a"], z["v_b"], ene, cond_ll, vo_a=z.get("vo_a"), vo_b=z.get("vo_b"), **vectors)
        wl, wr = kubo_bastin_weights(ene, cond_ll, emin, emax)
    finally:
        Rm.chebyshev_scaling = orig
        rec.close()
    mu = np.asarray(z["mu_nm"])[:, :, :cond_ll, :cond_ll, :got.shape[2]]
    ref = R.integrand_factorised(mu, ene, emin, emax)
    assert got.shape == ref.shape == (18, 8, mu.shape[4])
    mag = np.einsum("me,ne,lnmv->lev", np.abs(wl), np.abs(wr), np.abs(mu[DIAG, DIAG]))
    mag = mag[:, 0::2] + mag[:, 1::2]
    ratio = np.abs(got - ref) / mag
    print("%s: worst |integrand_at - reference| / magnitude sum %.2e, / max|ref| %.2e" % (name, ratio.max(), np.abs(got - ref).max() / np.abs(ref).max()))
    assert np.all(np.abs(got - ref) <= RTOL * mag), (name, float(ratio.max()))


def test_greenwood_equals_the_contracted_moments(shared):
    S = shared[False]
    c, rec = S.c, S.c.rec
    Rm, orig = pinned_scaling(dict(acheb=c.a, bcheb=c.b))
    ene = np.array([-0.6, 0.05, 0.7])
    try:
        got = Conductivity(rec).greenwood(c.ops[0], c.ops[2], ene, LL, seeds=c.seeds, coefs=c.coefs)
        d = rec.compute_moments_stochastic(c.ops[0], c.ops[2], LL, seeds=c.seeds, coefs=c.coefs, diag=True)
        wl, wr = kubo_greenwood_weights(ene, LL, rec.en.energy_min, rec.en.energy_max)
    finally:
        Rm.chebyshev_scaling = orig
    ref = np.einsum("me,ne,lnmv->lev", wl, wr, d)
    mag = np.einsum("me,ne,lnmv->lev", np.abs(wl), np.abs(wr), np.abs(d))
    assert got.shape == (18, 3, 3)
    print("greenwood: worst deviation %.2e of the magnitude sum" % (np.abs(got - ref) / mag).max())
    assert np.all(np.abs(got - ref) <= RTOL * mag)


def test_refusals_leave_the_handle_usable(shared):
    S = shared[True]
    c = S.c
    wl, wr = random_weights(11, LL, 3)
    rc, base, base_d = shot(c, S.outs[:2], wl, wr)
    assert rc == 0, c.last_error()
    big = np.zeros((LL, 17), np.complex128, order="F")
    nan_w, inf_w = wr.copy(order="F"), wl.copy(order="F")
    nan_w[5, 1] = np.nan
    inf_w[0, 2] = complex(0.0, np.inf)
    no_seed = (np.zeros((1, 4), np.int32), np.ones((1, 4), np.complex128))
    far_seed = (np.full((1, 1), KK_ODD + 1, np.int32), np.ones((1, 1), np.complex128))
    keep3 = c.ops[3]
    refusals = [
        ("ne = 0", lambda: shot(c, S.outs[:2], wl, wr, ne=0)),
        ("ne = 17", lambda: shot(c, S.outs[:2], big, big)),
        ("cond_ll = 0", lambda: shot(c, S.outs[:2], wl, wr, cond_ll=0)),
        ("cond_ll too large", lambda: shot(c, S.outs[:2], wl, wr, cond_ll=_lib.KUBO_SHOT_LL_MAX + 1)),
        ("nout = 0", lambda: shot(c, S.outs[:2], wl, wr, nout=0)),
        ("nout = 9", lambda: shot(c, S.outs[:2], wl, wr, nout=9)),
        ("wl NULL", lambda: shot(c, S.outs[:2], wl, wr, wl_ptr=None)),
        ("wr NULL", lambda: shot(c, S.outs[:2], wl, wr, wr_ptr=None)),
        ("v_out NULL", lambda: shot(c, [], wl, wr, nout=1)),
        ("v_b NULL", lambda: shot(c, S.outs[:2], wl, wr, v_b=None)),
        ("NaN weight", lambda: shot(c, S.outs[:2], wl, nan_w)),
        ("Inf weight", lambda: shot(c, S.outs[:2], inf_w, wr)),
        ("both outputs NULL", lambda: shot(c, S.outs[:2], wl, wr, full=None, diag=None)),
        ("hoh without vo_out", lambda: shot(c, [(o[0], None) for o in S.outs[:2]], wl, wr)),
        ("nseed = 0", lambda: shot(c, S.outs[:2], wl, wr, nseed=0)),
        ("seed_atoms NULL", lambda: shot(c, S.outs[:2], wl, wr, seed_ptrs=(False, True))),
        ("seed_coef NULL", lambda: shot(c, S.outs[:2], wl, wr, seed_ptrs=(True, False))),
        ("a = 0", lambda: shot(c, S.outs[:2], wl, wr, a=0.0)),
        ("nvec < 0", lambda: shot(c, S.outs[:2], wl, wr, nvec=-1)),
        ("vector without a seed", lambda: shot(c, S.outs[:2], wl, wr, seeds=no_seed)),
        ("seed atom outside the lattice", lambda: shot(c, S.outs[:2], wl, wr, seeds=far_seed)),
    ]
    for what, call in refusals:
        rc = call()[0]
        assert rc == _lib.ERR_ARG, (what, rc)
        assert b"rsrec_kubo_single_shot" in c.last_error(), (what, c.last_error())
    c.ops[3] = None                                                   # hoh without vo_b
    try:
        assert shot(c, S.outs[:2], wl, wr)[0] == _lib.ERR_ARG and b"rsrec_kubo_single_shot" in c.last_error()
    finally:
        c.ops[3] = keep3
    none = (np.zeros((0, 1), np.int32), np.zeros((0, 1), np.complex128))
    assert shot(c, S.outs[:2], wl, wr, seeds=none)[0] == 0            # nvec = 0
    rc, s, d = shot(c, S.outs[:2], wl, wr)
    assert rc == 0 and same_bits(s, base) and same_bits(d, base_d)
    ref, mag = contract(S.moments(0, LL), wl, wr)
    assert_blocks(s[..., 0], ref, mag, "after the refusals")
