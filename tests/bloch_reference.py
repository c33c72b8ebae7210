"""Dense numpy restatement of the k-resolved Chebyshev moments (rsrec_chebyshev_bloch), and their independent oracle.  Not a test module.

``bloch_sums`` restates the call: the lattice Fourier sum of the Chebyshev vector started at a source atom, group by group, built on
``pair_direct_reference.chain_blocks``.  ``bloch_hamiltonian_moments`` knows nothing of chains: on a periodic one-atom cell it forms the
18x18 H~(k) = sum_j exp(-i k.(r_j - r_i)) H[j,i] and runs the three-term recurrence on that matrix."""
import functools

import numpy as np

from helpers import load_golden, supercell_problem
from pair_direct_reference import chain_blocks, dense_h
from rslmtoasa_amd.lattice import BCC_PRIMITIVE, supercell_positions


def displacements(cr, source, cell=None):
    """(3, kk): cr(:,j) - cr(:,source), reduced to the minimum image d - cell nint(cell^-1 d) when ``cell`` (columns = supercell vectors) is given."""
    d = np.asarray(cr, np.float64) - np.asarray(cr, np.float64)[:, source - 1:source]
    if cell is not None:
        cell = np.asarray(cell, np.float64)
        d = d - cell @ np.rint(np.linalg.solve(cell, d))
    return d


def bloch_sums(H, a, b, sources, lld, cr, cell, kpts, group=None, ngroup=1):
    """(18,18,2 lld + 2,nk,ngroup,nsrc) as the library call defines s_k.  kpts (3,nk); group (kk) with values 0..ngroup or None."""
    nmom, kk = 2 * lld + 2, H.shape[0] // 18
    kpts = np.asarray(kpts, np.float64).reshape(3, -1)
    group = np.ones(kk, np.int32) if group is None else np.asarray(group)
    out = np.zeros((18, 18, nmom, kpts.shape[1], ngroup, len(sources)), np.complex128, order="F")
    chains = {}
    for s, src in enumerate(sources):
        src = int(src)
        if src not in chains:
            chains[src] = chain_blocks(H, a, b, src, nmom)
        w = np.exp(-1j * (kpts.T @ displacements(cr, src, cell)))            # (nk, kk)
        for g in range(ngroup):
            out[:, :, :, :, g, s] = np.einsum("qj,jabn->abnq", w * (group == g + 1)[None, :], chains[src])
    return out


def stencil_column(p, source):
    """(kk, 18, 18): the blocks H[j, source] of a problem dict WITHOUT hoh and without per-atom blocks, straight from ``nn`` / ``ee`` /
    ``lsham`` -- the column of pair_direct_reference.dense_h for lattices too large for a dense matrix."""
    assert not p.get("hoh") and not int(p.get("nmax", 0))
    nn, iz = np.asarray(p["nn"]), np.asarray(p["iz"])
    col = np.zeros((nn.shape[0], 18, 18), np.complex128)
    t = int(iz[source - 1]) - 1
    col[source - 1] += p["ee"][:, :, 0, t] + p["lsham"][:, :, t]
    for j, s in np.argwhere(nn[:, 1:] == source):
        if s + 1 < int(nn[j, 0]):
            col[j] += p["ee"][:, :, s + 1, int(iz[j]) - 1]
    return col


def bloch_hamiltonian_moments(H, a, b, source, lld, cr, cell, kpts):
    """(18,18,2 lld + 2,nk): T_n of the 18x18 H~(k) = (sum_j exp(-i k.d(j,i)) H[j,i] - b) / a, i = ``source``: what S_i(k, n) is on a
    periodic one-atom cell at supercell-commensurate k.  ``H``: the dense matrix, or its column of blocks (kk, 18, 18) at ``source``."""
    nmom = 2 * lld + 2
    kpts = np.asarray(kpts, np.float64).reshape(3, -1)
    w = np.exp(-1j * (kpts.T @ displacements(cr, source, cell)))
    col = H if H.ndim == 3 else H[:, 18 * (source - 1):18 * source].reshape(H.shape[0] // 18, 18, 18)
    out = np.zeros((18, 18, nmom, kpts.shape[1]), np.complex128, order="F")
    for q in range(kpts.shape[1]):
        Hk = (np.einsum("j,jab->ab", w[q], col) - b * np.eye(18)) / a
        t0, t1 = np.eye(18, dtype=np.complex128), Hk
        out[:, :, 0, q], out[:, :, 1, q] = t0, t1
        for n in range(2, nmom):
            t0, t1 = t1, 2.0 * (Hk @ t1) - t0
            out[:, :, n, q] = t1
    return out


def supercell_cell(dims, primitive=BCC_PRIMITIVE):
    """(3,3), columns = the supercell vectors n_i a_i."""
    return np.asfortranarray((np.asarray(dims, np.float64)[:, None] * primitive).T)


def commensurate_k(dims, m, primitive=BCC_PRIMITIVE):
    """(3, len(m)): k = 2 pi sum_i (m_i / n_i) b_i with b = inv(primitive).T rows, for integer triples m."""
    bvec = np.linalg.inv(primitive).T
    frac = np.asarray(m, np.float64).reshape(-1, 3) / np.asarray(dims, np.float64)[None, :]
    return np.asfortranarray((2.0 * np.pi * frac @ bvec).T)


def image_errors(mine, ref):
    """Largest deviation of every (group, source) image, relative to the largest element of that image of ``ref`` (nk and n included).
    An image that is all zero in ``ref`` (a group the region never reaches) must be all zero: 0.0 or inf."""
    def one(m, r):
        scale = np.abs(r).max()
        if scale == 0:
            return 0.0 if np.all(m == 0) else np.inf
        return float(np.abs(m - r).max() / scale)
    return [[one(mine[..., g, s], ref[..., g, s]) for g in range(ref.shape[4])] for s in range(ref.shape[5])]


@functools.lru_cache(maxsize=None)
def fixture_case(hoh=False):
    """The committed 4x4x8 pair fixture's operator: (dims, problem dict, dense H, a, b, lld, emin, emax, positions, cell)."""
    g = load_golden("sc_4x4x8_cheb_ij_hoh" if hoh else "sc_4x4x8_cheb_ij")
    dims = tuple(int(x) for x in g["dims"])
    p = supercell_problem(dims, hoh=hoh)
    return dims, p, dense_h(p), float(g["acheb"]), float(g["bcheb"]), int(g["lld"]), float(g["emin"]), float(g["emax"]), supercell_positions(dims), supercell_cell(dims)
