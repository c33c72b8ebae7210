"""Inputs with KNOWN square roots for the 18x18 eigen-solver (jacobi18 + matfun18, rslmtoasa_amd/csrc/eig18.hpp), and chains whose
block-Lanczos coefficients have known spectra.  Plain module: numpy only, every input from a fixed numpy.random.default_rng seed.

  exact_cases()       B = G^H G of small Gaussian integers, S = B B: integers below 2^40, so S is exact in double and sqrt(S) = B is
                      known exactly without any high-precision library;
  diagonal_cases()    diagonal S (the solver leaves before its first sweep): sqrt(S) = sqrt of the diagonal, bit for bit;
  spectrum_cases()    S = U diag(lambda) U^H (degenerate, clustered, graded, ...) and S of 2x2 blocks; the exact root of the ROUNDED
                      double matrix is in tests/golden/eig18_roots.npz (tools/eig18_fixture/make_fixture.py, mpmath at 50 digits), as
                      a double-double pair root_hi + root_lo;
  perturbed_lower()   a case with its strict lower triangle off by a rounding: the root asked for is the one of the upper triangle;
  prescribed_chain()  a 1-D chain whose hops are P diag(sigma) Q^H: eig(B_n^2) = sigma_n^2 and eig(A_n) = eig(E_{n+1}) exactly.
"""
import os

import numpy as np

NB = 18
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eig18_roots.npz")


def herm(a):
    return 0.5 * (a + a.conj().T)


def fro(a):
    return float(np.sqrt(np.sum(np.abs(np.asarray(a, dtype=np.complex128)) ** 2)))


def random_unitary(rng, n=NB):
    q, r = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    d = np.diagonal(r)
    return q * (d / np.abs(d))


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) integer matrices: the root is known exactly
# ---------------------------------------------------------------------------------------------------------------------------------
def _int_gram(gr, gi):
    """(re, im) of G^H G in int64."""
    return gr.T @ gr + gi.T @ gi, gr.T @ gi - gi.T @ gr


def _int_square(br, bi):
    return br @ br - bi @ bi, br @ bi + bi @ br


def _exact_pair(br, bi):
    """B (complex128) and S = B B from the integer parts of B; asserts that S is integer-valued, below 2^40, and that the product in
    double is the product in integers (so S holds B^2 exactly)."""
    br, bi = np.asarray(br, np.int64), np.asarray(bi, np.int64)
    assert np.array_equal(br, br.T) and np.array_equal(bi, -bi.T)
    sr, si = _int_square(br, bi)
    assert max(np.abs(sr).max(), np.abs(si).max()) < 2 ** 40
    B = br.astype(np.float64) + 1j * bi.astype(np.float64)
    S = sr.astype(np.float64) + 1j * si.astype(np.float64)
    assert np.array_equal(B @ B, S) and np.array_equal(S, np.round(S.real) + 1j * np.round(S.imag))
    return B, S


def _full_rank_gram(rng, n, lo, hi, real=False):
    """G^H G of an n x n matrix of integers in [lo, hi] (+ i the same), redrawn while rank-deficient."""
    while True:
        gr = rng.integers(lo, hi + 1, (n, n))
        gi = np.zeros_like(gr) if real else rng.integers(lo, hi + 1, (n, n))
        if np.linalg.matrix_rank(gr + 1j * gi) == n:
            return _int_gram(gr, gi)


def _kron_int(a, b):
    (ar, ai), (br, bi) = a, b
    return np.kron(ar, br) - np.kron(ai, bi), np.kron(ar, bi) + np.kron(ai, br)


def exact_cases():
    """[(name, S, B)]: S = B B exactly, B Hermitian positive definite."""
    out = []
    rng = np.random.default_rng(18001)
    for j in range(2):
        out.append(("dense%d" % j,) + _exact_pair(*_full_rank_gram(rng, NB, -2, 2))[::-1])
    # spin-diagonal: two 9x9 blocks
    br, bi = np.zeros((NB, NB), np.int64), np.zeros((NB, NB), np.int64)
    for s in (0, 9):
        br[s:s + 9, s:s + 9], bi[s:s + 9, s:s + 9] = _full_rank_gram(rng, 9, -2, 2)
    out.append(("spin_diagonal",) + _exact_pair(br, bi)[::-1])
    # real, the worst-conditioned of a few draws with cond(B) <= 1e6
    best = None
    for _ in range(40):
        g = _full_rank_gram(rng, NB, -3, 3, real=True)
        c = np.linalg.cond(g[0].astype(np.float64))
        if c <= 1e6 and (best is None or c > best[0]):
            best = (c, g)
    assert best is not None and best[0] > 1e3
    out.append(("real",) + _exact_pair(*best[1])[::-1])
    eye = np.eye(NB, dtype=np.int64)
    out.append(("seven_identity",) + _exact_pair(7 * eye, 0 * eye)[::-1])
    # three 6-fold eigenvalues: kron(G3^H G3, I6), rows and columns mixed by a signed permutation (an integer +-1 matrix)
    g3 = _full_rank_gram(rng, 3, -2, 2)
    kr, ki = _kron_int(g3, (np.eye(6, dtype=np.int64), np.zeros((6, 6), np.int64)))
    m = np.zeros((NB, NB), np.int64)
    m[np.arange(NB), rng.permutation(NB)] = rng.choice([-1, 1], NB)
    out.append(("kron3x6_mixed",) + _exact_pair(m @ kr @ m.T, m @ ki @ m.T)[::-1])
    # two 9-fold eigenvalues: kron(I9, G2^H G2)
    g2 = _full_rank_gram(rng, 2, -2, 2)
    out.append(("kron9x2",) + _exact_pair(*_kron_int((np.eye(9, dtype=np.int64), np.zeros((9, 9), np.int64)), g2))[::-1])
    return [(n, S, B) for n, S, B in out]


def diagonal_cases():
    """[(name, S, B)]: diagonal S, B = sqrt of its diagonal (IEEE sqrt, correctly rounded: the device must give these bits)."""
    rng = np.random.default_rng(18002)
    asc = np.arange(1.0, NB + 1.0) ** 2
    real = np.sort(10.0 ** rng.uniform(-3, 3, NB))
    out = [("diag_ascending", asc), ("diag_descending", asc[::-1].copy()), ("diag_shuffled", rng.permutation(asc)),
           ("diag_real_descending", real[::-1].copy()), ("diag_real_shuffled", rng.permutation(real)), ("zero", np.zeros(NB)),
           ("seven_squared_identity", np.full(NB, 49.0))]
    return [(n, np.diag(d).astype(np.complex128), np.diag(np.sqrt(d)).astype(np.complex128)) for n, d in out]


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) prescribed spectra; the exact roots are in the fixture
# ---------------------------------------------------------------------------------------------------------------------------------
def _pair_blocks(rng, pairs, equal_diagonal):
    """Positive definite S that couples only the given pairs (p, q): [[a, x], [conj x, b]] with |x| < sqrt(a b); b = a if asked."""
    S = np.zeros((NB, NB), np.complex128)
    for p, q in pairs:
        a = rng.uniform(0.5, 2.0)
        b = a if equal_diagonal else rng.uniform(0.5, 2.0)
        x = rng.uniform(0.1, 0.8) * np.sqrt(a * b) * np.exp(2j * np.pi * rng.random())
        S[p, p], S[q, q], S[p, q], S[q, p] = a, b, x, np.conj(x)
    return S


def spectrum_cases():
    """[(name, S)]: Hermitian positive definite (exactly Hermitian in double), two seeds per class, names '<class>_<seed index>'."""
    k = np.arange(NB, dtype=np.float64)
    spectra = [
        ("deg3x6", np.repeat([0.7, 1.3, 2.9], 6)),
        ("deg2x9", np.repeat([0.6, 1.9], 9)),
        ("equal", np.full(NB, 1.7)),
        ("cluster", 1.0 + 1e-13 * k),
        ("graded8", 10.0 ** (-8.0 * k / 17.0)),
        ("graded12", 10.0 ** (-12.0 * k / 17.0)),
        ("one_small", np.concatenate([[1e-4], np.linspace(0.5, 2.0, NB - 1)])),
    ]
    out = []
    for j in range(2):
        rng = np.random.default_rng(18100 + j)
        for name, lam in spectra:
            U = random_unitary(rng)
            out.append(("%s_%d" % (name, j), herm((U * lam) @ U.conj().T)))
        # D (I + 0.1 R) D with a strongly graded D: the relative accuracy of the small eigenvalues is what a Jacobi method is good at
        R = herm(rng.standard_normal((NB, NB)) + 1j * rng.standard_normal((NB, NB)))
        R /= np.linalg.norm(R, 2)
        D = 10.0 ** (-k / 1.5)
        out.append(("scaled_diag_%d" % j, herm(D[:, None] * (np.eye(NB) + 0.1 * R) * D[None, :])))
        # only 2x2 blocks coupled: beta == 0 on most pairs of every round
        out.append(("pairs_%d" % j, _pair_blocks(rng, [(2 * i, 2 * i + 1) for i in range(9)], False)))
        # app == aqq exactly on the coupled pairs: tau == 0, a 45 degree rotation
        out.append(("tau_zero_%d" % j, _pair_blocks(rng, [(i, NB - 1 - i) for i in range(9)], True)))
    for _, S in out:
        assert np.array_equal(S, S.conj().T)
    return out


def load_roots():
    """{name: (S, root_hi, root_lo)} of the fixture: sqrt(S) = root_hi + root_lo to about 1e-32."""
    with np.load(GOLDEN, allow_pickle=False) as z:
        names = [str(n) for n in z["names"]]
        return {n: (z["S"][:, :, i], z["root_hi"][:, :, i], z["root_lo"][:, :, i]) for i, n in enumerate(names)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.complex128), np.ascontiguousarray(b, dtype=np.complex128)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def spectrum_cases_with_roots():
    """[(name, S, B)] with B the exact root rounded to double; the inputs regenerated here must be the fixture's, bit for bit."""
    roots = load_roots()
    out = []
    for name, S in spectrum_cases():
        assert name in roots and same_bits(S, roots[name][0]), "tests/golden/eig18_roots.npz does not hold the input %s" % name
        out.append((name, S, roots[name][1]))
    assert len(out) == len(roots)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) Hermitian only to rounding
# ---------------------------------------------------------------------------------------------------------------------------------
def perturbed_lower(S, seed):
    """S with its strict lower triangle multiplied by (1 + 1e-15 xi), xi uniform in [-1, 1]: what a sum of rounded products leaves.
    LAPACK's zheev('U') never reads that triangle; the Jacobi solver does.  The root asked for stays sqrt(S)."""
    rng = np.random.default_rng(seed)
    P = np.array(S, dtype=np.complex128, copy=True)
    il = np.tril_indices(NB, -1)
    P[il] *= 1.0 + 1e-15 * rng.uniform(-1.0, 1.0, len(il[0]))
    return P


PERTURBED = ("deg3x6_0", "graded8_0", "one_small_1", "cluster_0", "pairs_1", "tau_zero_0")


def perturbed_cases():
    byname = {n: (S, B) for n, S, B in spectrum_cases_with_roots()}
    return [(n + "_lower", perturbed_lower(byname[n][0], 18200 + i), byname[n][1]) for i, n in enumerate(PERTURBED)]


# ---------------------------------------------------------------------------------------------------------------------------------
# powers of two: sqrt(S 2^k) = sqrt(S) 2^(k/2), and a Jacobi method that tests convergence scale-free gives that bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
SCALE_IN = (-480, -400, -100, 100, 400, 480)       # the squared-norm tests of the solver neither under- nor overflowed here before
SCALE_OUT = (-600, -520, 500, 600)                 # ... and did here: early exit at the small end, NaN at the large end
SCALE_BASES = ("dense0", "deg3x6_0", "graded8_0")


def scaled(a, k):
    a = np.asarray(a, dtype=np.complex128)
    return np.ldexp(a.real, k) + 1j * np.ldexp(a.imag, k)


def scale_bases():
    byname = {n: (S, B) for n, S, B in exact_cases() + spectrum_cases_with_roots()}
    return [(n,) + byname[n] for n in SCALE_BASES]


# ---------------------------------------------------------------------------------------------------------------------------------
# error measures (the bars of tests/test_gpu_eig18.py; tests/test_eig18_cases.py holds the CPU oracle to the same ones)
# ---------------------------------------------------------------------------------------------------------------------------------
FORWARD_FLOOR = 1e-13          # the bar tests/test_gpu_parity.py holds zsqr to
ORACLE_FACTOR = 16.0
BACKWARD = 1e-13


def forward_error(B, exact):
    return fro(B - exact) / fro(exact)


def forward_bar(oracle_error):
    return max(FORWARD_FLOOR, ORACLE_FACTOR * oracle_error)


def structure_errors(B, S):
    """(backward ||B B - S|| / ||S||, ||B - B^H|| / ||B||, -min eig(herm B) / ||B||): each must stay <= BACKWARD."""
    nb = fro(B)
    return fro(B @ B - S) / fro(S), fro(B - B.conj().T) / nb, -float(np.linalg.eigvalsh(herm(B)).min()) / nb


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) chains with prescribed block-Lanczos spectra
# ---------------------------------------------------------------------------------------------------------------------------------
def prescribed_chain(sigmas, seed):
    """A 1-D chain of N = len(sigmas) + 1 atoms, one atom type per atom, three slots: the atom itself, atom k - 1, atom k + 1 (0 = none at
    the ends).  On-site blocks E_k random Hermitian; the hop INTO atom k + 1 from atom k is T_k = P_k diag(sigmas[k - 1]) Q_k^H with
    random unitaries (slot 2 of atom k + 1), the opposite slot holds T_k^H; lsham = 0.  Block Lanczos seeded at atom 1 with lld = N walks
    down the chain: in exact arithmetic B_n^2 = U^H T_n^H T_n U and A_n = U'^H E_{n+1} U' with unitary U, U', so

        eig(b2_b[:, :, n]) = sigmas[n - 1]^2 (n = 1 .. N - 1),    eig(a_b[:, :, n]) = eig(E_{n+1}) (n = 0 .. N - 2).

    Returns (problem dict for the oracle / objects_from, [sorted sigma_n^2 for n = 1 ..], [sorted eig(E_k) for k = 1 ..])."""
    rng = np.random.default_rng(seed)
    sigmas = [np.asarray(s, dtype=np.float64) for s in sigmas]
    N = len(sigmas) + 1
    nn = np.zeros((N, 4), np.int32, order="F")
    ee = np.zeros((NB, NB, 3, N), np.complex128, order="F")
    E = []
    for k in range(N):
        nn[k, 0] = 3
        nn[k, 1] = k                                   # slot 2: atom k - 1 (1-based; 0 at the left end)
        nn[k, 2] = k + 2 if k + 1 < N else 0           # slot 3: atom k + 1
        Ek = herm(rng.standard_normal((NB, NB)) + 1j * rng.standard_normal((NB, NB))) * 0.3
        ee[:, :, 0, k] = Ek
        E.append(np.linalg.eigvalsh(Ek))
    for k, s in enumerate(sigmas):                     # hop between atoms k + 1 and k + 2 (1-based)
        assert s.shape == (NB,) and (s > 0).all()
        T = (random_unitary(rng) * s) @ random_unitary(rng).conj().T
        ee[:, :, 1, k + 1] = T
        ee[:, :, 2, k] = T.conj().T
    p = dict(nn=nn, iz=np.arange(1, N + 1, dtype=np.int32), ee=ee, lsham=np.zeros((NB, NB, N), np.complex128, order="F"), nmax=0, hoh=0, nsp=2)
    return p, [np.sort(s ** 2) for s in sigmas], E


def chain_sigmas(kind, nhops, seed):
    """The singular values of every hop of a well-conditioned chain: 'uniform' in [0.5, 1.5], 'deg3x6' three 6-fold values, 'equal' one."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return [rng.uniform(0.5, 1.5, NB) for _ in range(nhops)]
    if kind == "deg3x6":
        return [np.repeat(rng.uniform(0.5, 1.5, 3), 6) for _ in range(nhops)]
    if kind == "equal":
        return [np.full(NB, rng.uniform(0.5, 1.5)) for _ in range(nhops)]
    raise ValueError(kind)


def graded_sigmas(kind, seed):
    """Two hops (N = 3): the first ill-conditioned -- kappa(B_1^2) = 1e4 or 1e8 graded, or one sigma = 1e-4 --, the second uniform in
    [0.5, 1.5].  Rounding is amplified by about sqrt(kappa) at the graded level and by kappa per further level, so a chain never holds
    more than one graded hop."""
    rng = np.random.default_rng(seed)
    k = np.arange(NB, dtype=np.float64)
    first = {"kappa1e4": 10.0 ** (-2.0 * k / 17.0), "kappa1e8": 10.0 ** (-4.0 * k / 17.0),
             "one_small": np.concatenate([[1e-4], np.linspace(0.5, 1.5, NB - 1)])}[kind]
    return [first, rng.uniform(0.5, 1.5, NB)]


def chain_spectrum_errors(a_b, b2_b, sig2, E):
    """(worst |eig(b2_b[n]) - sigma_n^2| / max sigma_n^2 per level n = 1 .., worst |eig(herm a_b[n]) - eig E_{n+1}| / max|eig E| per level
    n = 0 ..) of one chain's coefficients (18, 18, lld)."""
    eb = [float(np.abs(np.linalg.eigvalsh(herm(b2_b[:, :, n + 1])) - s).max() / s.max()) for n, s in enumerate(sig2)]
    ea = [float(np.abs(np.linalg.eigvalsh(herm(a_b[:, :, n])) - E[n]).max() / np.abs(E[n]).max()) for n in range(len(sig2))]
    return np.array(eb), np.array(ea)
