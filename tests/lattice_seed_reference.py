"""Dense numpy restatement of the Chebyshev moments from whole-lattice seeds (rsrec_chebyshev_lattice), and the cells its tests run on.
Not a test module.

``lattice_moments`` restates the call on ``pair_direct_reference.dense_h``: the seed x = sum_j c_j |j> (x) 1_18 placed entry by entry (a
later entry on the same atom overwrites), the three-term recurrence on the whole vector, and per order the seed-weighted sum of the
vector's own blocks, M_g(n) = sum_{j in g} conj(c_j) [T_n(H~) x]_j."""
import functools

import numpy as np

from bloch_reference import fixture_case, supercell_cell
from helpers import supercell_problem
from pair_direct_reference import dense_h
from rslmtoasa_amd.lattice import supercell_positions


def placed_coefficients(kk, seeds, coefs):
    """(kk) complex: what lies on every atom after the entries of one chain are placed in order (atom 0: unused entry)."""
    c = np.zeros(kk, np.complex128)
    for s, v in zip(np.asarray(seeds).ravel(), np.asarray(coefs).ravel()):
        if s:
            c[int(s) - 1] = v
    return c


def lattice_moments(H, a, b, seeds, coefs, lld, group=None, ngroup=1):
    """(18,18,2 lld + 2,ngroup,nchains) as the library call defines m_g.  seeds, coefs (nchains, nseed); group (kk) with values
    0..ngroup or None."""
    nmom, kk = 2 * lld + 2, H.shape[0] // 18
    seeds, coefs = np.asarray(seeds).reshape(len(seeds), -1), np.asarray(coefs).reshape(len(seeds), -1)
    group = np.ones(kk, np.int32) if group is None else np.asarray(group)
    Ht = (H - b * np.eye(H.shape[0])) / a
    out = np.zeros((18, 18, nmom, ngroup, len(seeds)), np.complex128, order="F")
    for c in range(len(seeds)):
        w = placed_coefficients(kk, seeds[c], coefs[c])
        p0 = np.kron(w[:, None], np.eye(18))                               # (18 kk, 18): block j = c_j 1
        p1 = Ht @ p0
        for n in range(nmom):
            if n >= 2:
                p0, p1 = p1, 2.0 * (Ht @ p1) - p0
            blocks = (p0 if n == 0 else p1).reshape(kk, 18, 18)
            for g in range(ngroup):
                out[:, :, n, g, c] = np.einsum("j,jab->ab", np.conj(w) * (group == g + 1), blocks)
    return out


def plane_wave_seeds(kpts, cr):
    """(seeds (nk, kk) int32, coefs (nk, kk)): c_j = exp(+i k.r_j) / sqrt(kk) on every atom, as Recursion.bloch_average builds them."""
    k = np.asarray(kpts, np.float64).reshape(3, -1)
    kk = np.asarray(cr).shape[1]
    return np.tile(np.arange(1, kk + 1, dtype=np.int32), (k.shape[1], 1)), np.exp(1j * (k.T @ np.asarray(cr, np.float64))) / np.sqrt(float(kk))


ALLOY_SHIFT = 0.15              # on-site shift of the second atom type
ALLOY_LLD = 5
ALLOY_K = [(0, 0, 0), (1, 2, 3), (2, 0, 4)]      # commensurate points of the 4x4x8 cell, Gamma included


@functools.lru_cache(maxsize=None)
def alloy_case(hoh=False):
    """A two-type random 4x4x8 cell: the bcc Fe stencil (with hoh: every hoh array) duplicated along the type axis, the second type's
    on-site block shifted by ALLOY_SHIFT, the types drawn at random.  Returns (dims, problem dict, dense H, a, b, emin, emax, cr, cell)."""
    from rslmtoasa_amd.recursion import chebyshev_scaling
    dims, _, _, _, _, _, emin, emax, _, _ = fixture_case(hoh)
    p = dict(supercell_problem(dims, hoh=hoh))
    kk = p["nn"].shape[0]
    p["iz"] = np.random.default_rng(7).integers(1, 3, kk).astype(np.int32)
    for key in ("ee", "lsham", "eeo", "enim"):
        if key in p:
            p[key] = np.asfortranarray(np.concatenate([p[key], p[key]], axis=-1))
    p["ee"][:, :, 0, 1] += ALLOY_SHIFT * np.eye(18)
    emax = emax + ALLOY_SHIFT
    a, b = chebyshev_scaling(emin, emax)
    return dims, p, dense_h(p), a, b, emin, emax, supercell_positions(dims), supercell_cell(dims)
