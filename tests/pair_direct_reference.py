"""Dense numpy restatement of the pair moments from one Chebyshev chain per atom (rsrec_chebyshev_pairs_direct).  Not a test module.

H is built as a dense matrix from ``nn`` / ``ee`` / ``lsham`` (and ``eeo`` / ``enim`` with hoh, ``hall`` / ``hallo`` for atoms with their
own blocks), the vectors follow the three-term recurrence psi_{n+1} = 2 H~ psi_n - psi_{n-1}, and M_ji(n) is the block at atom j of the vector started at atom i.  The four
slots of a pair are then either the reference's own values (``both``) or the ones without (M_ii + M_jj)/2 (the cancelling form)."""
import functools

import numpy as np

from helpers import load_golden, supercell_problem


def _stencil(nn, iz, nmax, per_type, per_atom):
    """Row block i holds the blocks of atom i (per_atom(:,:,slot,i) for the first nmax atoms, else per_type(:,:,slot,type_i)) at the
    column blocks of nn(i, slot); slot 1 is the atom itself."""
    kk = nn.shape[0]
    M = np.zeros((18 * kk, 18 * kk), np.complex128)
    for i in range(kk):
        B = per_atom[:, :, :, i] if i < nmax else per_type[:, :, :, int(iz[i]) - 1]
        M[18 * i:18 * i + 18, 18 * i:18 * i + 18] += B[:, :, 0]
        for s in range(1, int(nn[i, 0])):
            n = int(nn[i, s])
            if n:
                M[18 * i:18 * i + 18, 18 * (n - 1):18 * n] += B[:, :, s]
    return M


def dense_h(p):
    """H (18 kk, 18 kk) of a problem dict: h + l.s (hop_b, recursion.f90:1582, :1608), or with hoh h - (h o) h + e_nu + l.s (hop_b_hoh,
    :1411), h from ee / hall and h o from eeo / hallo."""
    nn, iz, nmax = np.asarray(p["nn"]), np.asarray(p["iz"]), int(p.get("nmax", 0))
    kk = nn.shape[0]
    H = _stencil(nn, iz, nmax, p["ee"], p.get("hall"))
    if p.get("hoh"):
        H = H - _stencil(nn, iz, nmax, p["eeo"], p.get("hallo")) @ H
    for i in range(kk):
        t = int(iz[i]) - 1
        H[18 * i:18 * i + 18, 18 * i:18 * i + 18] += p["lsham"][:, :, t] + (p["enim"][:, :, t] if p.get("hoh") else 0.0)
    return H


def chain_blocks(H, a, b, source, nmom):
    """(kk, 18, 18, nmom): block (atom, :, :, n) of T_n(H~) applied to the identity at the 1-based atom ``source``, H~ = (H - b)/a."""
    kk = H.shape[0] // 18
    Ht = (H - b * np.eye(H.shape[0])) / a
    p0 = np.zeros((18 * kk, 18), np.complex128)
    p0[18 * (source - 1):18 * source] = np.eye(18)
    out = np.zeros((kk, 18, 18, nmom), np.complex128)
    out[..., 0] = p0.reshape(kk, 18, 18)
    p1 = Ht @ p0
    out[..., 1] = p1.reshape(kk, 18, 18)
    for n in range(2, nmom):
        p0, p1 = p1, 2.0 * (Ht @ p1) - p0
        out[..., n] = p1.reshape(kk, 18, 18)
    return out


def pair_moments(H, a, b, pairs, lld, both_ends):
    """(mu (18,18,2 lld + 2,4 npairs), m_pair (18,18,2 lld + 2,2,npairs)) as the library call defines them."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    nmom = 2 * lld + 2
    sources = sorted(set(int(i) for i in pairs[:, 0]) | (set(int(j) for j in pairs[:, 1]) if both_ends else set()))
    chain = {s: chain_blocks(H, a, b, s, nmom) for s in sources}
    mu = np.zeros((18, 18, nmom, 4 * len(pairs)), np.complex128, order="F")
    m_pair = np.zeros((18, 18, nmom, 2, len(pairs)), np.complex128, order="F")
    for q, (i, j) in enumerate(pairs):
        i, j = int(i), int(j)
        mji = chain[i][j - 1]
        if i == j:
            mij = mji
            slots = [0.5 * mji] * 4
        else:
            mij = chain[j][i - 1] if both_ends else np.conj(mji.transpose(1, 0, 2))
            o, s = 0.5 * (mij + mji), 0.5 * 1j * (mij - mji)
            d = 0.5 * (chain[i][i - 1] + chain[j][j - 1]) if both_ends else 0.0
            slots = [d + o, d - o, d + s, d - s] if both_ends else [o, -o, s, -s]
        for r in range(4):
            mu[:, :, :, 4 * q + r] = slots[r]
        m_pair[:, :, :, 0, q], m_pair[:, :, :, 1, q] = mij, mji
    return mu, m_pair


def gij_gji(mu, q):
    """The combinations every consumer forms of the four slots of pair q (green.f90:446-453): (M_ij, M_ji)."""
    d, s = mu[..., 4 * q] - mu[..., 4 * q + 1], (mu[..., 4 * q + 2] - mu[..., 4 * q + 3]) / 1j
    return 0.5 * (d + s), 0.5 * (d - s)


def pair_scale(ref, q):
    """The largest slot magnitude of pair q in a four-slot image: what the pair's deviations are judged on."""
    return np.abs(ref[..., 4 * q:4 * q + 4]).max()


@functools.lru_cache(maxsize=None)
def fixture_dense(name="sc_4x4x8_cheb_ij"):
    """The dense-route images of a committed pair fixture: (fixture, (mu, m_pair) of the both form, of the cancelling form)."""
    g = load_golden(name)
    H = dense_h(supercell_problem(g["dims"], hoh=bool(g["hoh"])))
    a, b, lld = float(g["acheb"]), float(g["bcheb"]), int(g["lld"])
    return g, pair_moments(H, a, b, g["pairs"], lld, True), pair_moments(H, a, b, g["pairs"], lld, False)


@functools.lru_cache(maxsize=None)
def consumer_sensitivity():
    """How far moments that are right to rounding move the exchange values: xc / fo / parts of ``exchange_cheb.npz`` recomputed (numpy
    restatement, g0 from the C oracle) from the dense-route moments of both forms, against the fixture's values, as a fraction of the
    largest |value| of the call.  This is the yardstick for comparing the consumers' values between the four-chain and the direct
    route (10 x it on the device, where the summation order differs).  Measured: 1.5e-13, the moments themselves being 9e-13 or less
    from the reference's; the distant pair (|J| = 2.8e-6) moves by 2.4e-16 absolute."""
    from exchange_reference import exchange_pair, fixture_g0
    z = load_golden("exchange_cheb")
    g, both, cancel = fixture_dense()
    assert str(z["source"]) == "sc_4x4x8_cheb_ij" and np.array_equal(z["pairs"], g["pairs"])
    scale = max(np.abs(z[k]).max() for k in ("xc", "fo", "parts"))
    worst = 0.0
    for mu, _ in (both, cancel):
        zz = dict(z)
        zz["mu_n"] = mu
        for p in range(len(z["pairs"])):
            xc, _, fo, parts, _, _ = exchange_pair(fixture_g0(zz, p), bool(z["same"][p]), z["dpar"][..., p], z["ene"], float(z["fermi"]), int(z["nv1"]),
                                                   cumulative=False)
            for mine, key in ((xc, "xc"), (fo, "fo"), (parts, "parts")):
                worst = max(worst, np.abs(mine - z[key][:, p]).max() / scale)
    return worst
