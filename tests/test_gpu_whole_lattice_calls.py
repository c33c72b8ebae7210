"""The entry points that work on the whole lattice share one call setup (WholeLatticeCall in rsrec.hip: the region of all atoms, the launch
shape of a batch, the SpMM launches with their events and flop accounting, the Chebyshev stepper, the closing bookkeeping):
rsrec_kubo_moments, rsrec_orbital_moments and rsrec_apply_operator interleaved on one handle must not see each other, and the shared end
keeps the two meanings of rest_ms."""
import numpy as np
import pytest

from helpers import load_golden
from test_gpu_kubo import KUBO_CASES, make_rec, scaled, vec_err

pytestmark = pytest.mark.gpu
COND_LL, NVEC = 4, 3
ORBITAL_SEEDS = np.array([7, 3, 100], np.int32)


def problem(name):
    """A Kubo fixture with what the calls below need besides it.  Positions: chebyshev_orbital_mod takes lattice%cr of the handle's own
    lattice, and the Kubo fixtures (512 atoms) store none -- cr and alat are those of fccPt_orbital_hoh (124 atoms), its columns repeated
    over the 512 atoms.  They enter the orbital moments as the per-atom factors X, Y only; any fixed array serves a comparison of a call
    with itself."""
    z = load_golden(name)
    zo = load_golden("fccPt_orbital_hoh")
    kk = z["nn"].shape[0]
    rng = np.random.default_rng(11)
    return dict(z=z, kk=kk, hoh=bool(int(z["hoh"])), a=float(z["acheb"]), b=float(z["bcheb"]), alat=float(zo["alat"]),
                cr=np.asfortranarray(zo["cr"][:, np.arange(kk) % zo["cr"].shape[1]]),
                seeds=np.tile(np.arange(1, kk + 1, dtype=np.int32), (NVEC, 1)),
                coefs=np.exp(2j * np.pi * rng.random((NVEC, kk))) / np.sqrt(kk),
                x=np.asfortranarray(rng.standard_normal((18, 18, kk)) + 1j * rng.standard_normal((18, 18, kk))))


def new_handle(q):
    """Three vectors in batches of two, three orbital seeds in batches of two: the last batch of either call is short (one chain)."""
    rec, _ = make_rec(q["z"])
    rec.set_option("kubo_vbatch", 2)
    rec.set_option("batch", 2)
    return rec


def steps(q):
    """The calls of the test in their order, each `name, f(rec) -> array`."""
    z = q["z"]

    def kubo(rec):
        return rec.compute_moments_stochastic(z["v_a"], z["v_b"], COND_LL, vo_a=z.get("vo_a"), vo_b=z.get("vo_b"), seeds=q["seeds"], coefs=q["coefs"]).copy()

    def ham(rec):
        return (rec.ham_hoh_vec_matmul if q["hoh"] else rec.ham_vec_matmul)(q["x"], q["a"], q["b"])

    def velo(rec):
        return rec.velo_vec_matmul(z["v_a"], q["x"], z.get("vo_a"))

    def orbital(rec):
        return rec.chebyshev_orbital_mod(q["cr"], q["alat"], seeds=ORBITAL_SEEDS)

    def lanczos(rec):
        rec.recur_b()
        return np.concatenate([rec.a_b.ravel(), rec.b2_b.ravel()])

    def kubo_chunked(rec):
        rec.set_option("kubo_lchunk", 3)                     # chunks of 3 + 1 left vectors
        return kubo(rec)

    return [("kubo", kubo), ("ham", ham), ("velo", velo), ("orbital", orbital), ("recur_b", lanczos), ("kubo_lchunk", kubo_chunked)]


@pytest.fixture(scope="module", params=KUBO_CASES)
def case(request):
    q = problem(request.param)
    import rslmtoasa_amd.recursion as R
    orig = scaled(None, q["z"])
    yield q
    R.chebyshev_scaling = orig


def test_interleaved_whole_lattice_calls_leak_no_state(case):
    """Kubo moments, ham[_hoh]_vec_matmul, velo_vec_matmul, orbital moments, recur_b and the Kubo call again with the left matrix in chunks
    on ONE handle: each gives the bits of the same call made first on a fresh handle (the region of all atoms, the work vectors, the seed
    tables, the kept Kubo buffers and the operator tables are shared between them).  No tolerance.  The chunked call on a fresh handle is
    also within 1e-13 of the one-chunk call, the bar of test_left_matrix_in_chunks."""
    q = case
    rec = new_handle(q)
    got = [(name, f(rec)) for name, f in steps(q)]
    rec.close()
    fresh = {}
    for name, f in steps(q):
        one = new_handle(q)
        fresh[name] = f(one)
        one.close()
    for name, res in got:
        assert np.array_equal(res, fresh[name]), name
    assert vec_err(fresh["kubo_lchunk"], fresh["kubo"]) < 1e-13


def test_timing_counters_keep_both_meanings_of_rest_ms(case):
    """rsrec_kubo_moments reports its contractions as rest_ms (so hop_ms + rest_ms stays below total_ms: seeding, copies and gaps are in
    neither); rsrec_orbital_moments reports rest_ms = total_ms - hop_ms.  Both end in the same function."""
    q = case
    rec = new_handle(q)
    calls = dict(steps(q))
    calls["kubo"](rec)
    t = rec.timing()
    print("kubo", t)
    assert t["hop_launches"] > 0
    assert t["rest_ms"] > 0 and t["hop_ms"] > 0
    assert t["hop_ms"] + t["rest_ms"] <= t["total_ms"]
    calls["orbital"](rec)
    t = rec.timing()
    print("orbital", t)
    rec.close()
    assert t["hop_launches"] > 0
    assert t["rest_ms"] == pytest.approx(t["total_ms"] - t["hop_ms"], rel=1e-12, abs=1e-12)
