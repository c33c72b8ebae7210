"""The 16x16 block of the folded A_n Gram as ONE tile  S = Re G + Im G = (Ur - Ui)^T Tr + (Ur + Ui)^T Ti  per (group, spin) partial
(kernels_spmm5.hpp, S5Gram), split by k_gram_groupsum into Re G = (S + S^T) / 2 and Im G = (S - S^T) / 2 on the summed matrix: exact when
G = sum u^H H u is Hermitian, i.e. for the operators that passed the Hermiticity check the fold is tied to.  The shapes of
tests/test_gpu_gram_fold.py: bcc 4x4x4 (eight full groups), bcc 5x4x3 (four padding atoms in the last group) and rnd444 (Hermitian,
full complex: Im G is not small against Re G), three sites with one repeated, LL = 8, every level folded, both forms of the kernel.
"""
import functools

import numpy as np
import pytest

from helpers import RTOL, rel_err
from test_gpu_gram_fold import FORMS, LLD, NEVER, engine, oracle_coefficients, problem, run

NAMES = ["fe444", "fe543", "rnd444"]


def frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def on_and_off(name, form):
    """Fold on, then fold off (s5_gram_min = NEVER), on one handle: (a_on, b_on, a_off, b_off).  Computed once per (problem, form)."""
    rec = engine(problem(name), FORMS[form])
    a1, b1, t1 = run(rec)
    rec.set_option("s5_gram_min", NEVER)
    a0, b0, t0 = run(rec)
    rec.close()
    assert t1["gram_folded_launches"] == LLD - 1 and t1["hop_fuses_a"] == 1
    assert t0["gram_folded_launches"] == 0 and t0["hop_fuses_a"] == 0
    return frozen(a1, b1, a0, b0)


def hermiticity_defect(a):
    """max over (folded level, site) of  |A - A^H|_max / |A|_max  (every level but the last folds; a_b(:,:,lld) = 0)."""
    worst = 0.0
    for n in range(LLD - 1):
        for s in range(a.shape[3]):
            m = a[:, :, n, s]
            worst = max(worst, float(np.abs(m - m.conj().T).max() / np.abs(m).max()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_symmetrised_gram_against_the_oracle(name, form, oracle_lib):
    a, b, _, _ = on_and_off(name, form)
    a_o, b_o = oracle_coefficients(oracle_lib, name)
    ea, eb = rel_err(a, a_o), rel_err(b, b_o)
    print(name, form, "a_b %.2e b2_b %.2e" % (ea, eb))
    assert ea < RTOL and eb < RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["fe543", "rnd444"])
def test_fold_on_against_fold_off(name, form):
    a1, b1, a0, b0 = on_and_off(name, form)
    ea, eb = rel_err(a1, a0), rel_err(b1, b0)
    print(name, form, "on/off a_b %.2e b2_b %.2e" % (ea, eb))
    assert ea < RTOL and eb < RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_folded_a_n_is_hermitian(name, form):
    """The symmetrised block is Hermitian by construction and the strips by completion; only the 2x2 corner is formed entry by entry."""
    a1, _, a0, _ = on_and_off(name, form)
    d1, d0 = hermiticity_defect(a1), hermiticity_defect(a0)
    print(name, form, "|A - A^H| / |A|: fold on %.2e, fold off %.2e" % (d1, d0))
    assert d1 <= d0 + RTOL
    assert d1 <= RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_both_forms_give_the_same_bits(name):
    """The persistent (LDS) and the global-load form run the same stream and the same epilogue on the same groups in the same order."""
    a1, b1, _, _ = on_and_off(name, "persistent")
    a2, b2, _, _ = on_and_off(name, "global")
    assert np.array_equal(a1, a2) and np.array_equal(b1, b2)


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["fe543", "rnd444"])
def test_symmetrised_results_are_bitwise_reproducible(name, form):
    """Two calls on one handle; batch = 1 against the batch; graph replay against plain launches; the repeated site against its first
    occurrence."""
    rec = engine(problem(name), FORMS[form] + (("graph", 0),))
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
    for _ in range(3):                       # capture, then two replays
        a2, b2, t2 = run(rec)
        assert t2["gram_folded_launches"] == LLD - 1
        assert np.array_equal(a2, a) and np.array_equal(b2, b)
    rec.close()
    a1, b1, _, _ = on_and_off(name, form)    # and another handle
    assert np.array_equal(a1, a) and np.array_equal(b1, b)


# ---- the epilogue in numpy (no GPU) ----------------------------------------------------------------------------------------------
NATOMS, NB = 24, 18


def block_operator(rng, eps=0.0):
    """Random Hermitian block operator on NATOMS atoms (dense: every pair coupled, H[j][i] = H[i][j]^H), as one matrix of norm ~ 1; eps adds
    an anti-Hermitian part of the same norm times eps.  Returns (H + eps K, K)."""
    n = NATOMS * NB
    x = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    y = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    h, k = x + x.conj().T, y - y.conj().T
    h /= np.linalg.norm(h, 2)
    k /= np.linalg.norm(k, 2)
    return h + eps * k, k


def epilogue_model(h, u):
    """What k_spmm5's epilogue and k_gram_groupsum form from t' = H u: per atom the tile S_i = (Ur - Ui)^T Tr + (Ur + Ui)^T Ti of columns
    a, b < 16, rows 16, 17 and the corner of u_i^H t'_i as they are; summed over the atoms in order; THEN Re = (S + S^T) / 2,
    Im = (S - S^T) / 2 and G[a < 16][16 + e] = conj(G[16 + e][a])."""
    t = h @ u
    s = np.zeros((16, 16))
    low = np.zeros((2, NB), np.complex128)
    for i in range(NATOMS):
        ui, ti = u[NB * i:NB * (i + 1)], t[NB * i:NB * (i + 1)]
        ur, uim, tr, tim = ui[:, :16].real, ui[:, :16].imag, ti[:, :16].real, ti[:, :16].imag
        s += (ur - uim).T @ tr + (ur + uim).T @ tim
        low += ui[:, 16:].conj().T @ ti
    g = np.zeros((NB, NB), np.complex128)
    g[:16, :16] = 0.5 * (s + s.T) + 0.5j * (s - s.T)
    g[16:, :] = low
    g[:16, 16:] = low[:, :16].conj().T
    return g


def test_epilogue_model_on_a_hermitian_operator():
    rng = np.random.default_rng(7)
    for _ in range(3):
        h, _ = block_operator(rng)
        u = rng.standard_normal((NATOMS * NB, NB)) + 1j * rng.standard_normal((NATOMS * NB, NB))
        g = u.conj().T @ h @ u
        err = np.abs(epilogue_model(h, u) - g).max() / np.abs(g).max()
        print("model against sum u^H H u: %.2e" % err)
        assert err < 1e-13
    # one atom's share alone is not Hermitian: the identities hold for the sum only
    ui, ti = u[:NB], (h @ u)[:NB]
    gi = ui.conj().T @ ti
    assert np.abs(gi - gi.conj().T).max() > 1e-3 * np.abs(gi).max()


@pytest.mark.parametrize("eps", [1e-3, 1e-6, 1e-9])
def test_epilogue_model_loses_the_anti_hermitian_part(eps):
    """With H + eps K, K anti-Hermitian, sum u^H (H + eps K) u = G + eps A with A = u^H K u anti-Hermitian: Re A is antisymmetric and Im A
    symmetric.  Of S = Re + Im the symmetric part then is Re G + eps Im A and the antisymmetric one Im G + eps Re A: the 16x16 block comes
    out as G + eps (Im A + i Re A) instead of G + eps (Re A + i Im A) -- a deviation of eps sqrt(2) |Re A - Im A| exactly (the model is
    linear in H), O(eps) and no smaller.  Hence the fold stays tied to the Hermiticity check."""
    rng = np.random.default_rng(11)
    h, k = block_operator(rng, eps)
    u = rng.standard_normal((NATOMS * NB, NB)) + 1j * rng.standard_normal((NATOMS * NB, NB))
    g, a = u.conj().T @ h @ u, u.conj().T @ k @ u
    dev = np.abs(epilogue_model(h, u) - g)[:16, :16].max()
    lost = eps * np.sqrt(2.0) * np.abs(a.real - a.imag)[:16, :16].max()
    print("eps %.0e: deviation %.3e, eps sqrt(2) |Re A - Im A| %.3e, |G| %.3e" % (eps, dev, lost, np.abs(g).max()))
    assert 0.5 * lost <= dev <= 2.0 * lost
