"""Dense numpy restatement of rsrec_chebyshev_bloch_map: functions of H at many k-points from energy-weighted sums of the Chebyshev vectors.
Not a test module.

``green_weights`` are the coefficients green%chebyshev_green applies to the moments, built on ``contour_reference.jackson_kernel``;
``bloch_map`` restates the call on ``pair_direct_reference.chain_blocks`` and ``bloch_reference.displacements``: it accumulates
Y_e = sum_n w(n, e) psi_{n-1} order by order, then takes ONE phase sum per energy -- the order of sums of the library, not that of
``bloch_reference.bloch_sums``."""
import numpy as np

from bloch_reference import displacements
from contour_reference import jackson_kernel
from pair_direct_reference import chain_blocks


def green_weights(nmom, a, b, ene):
    """(nmom, ne): w(n, e) = jackson(n) (2 for n > 1) (-i exp(-i (n-1) acos x_e)) / sqrt(a^2 - (E_e - b)^2), x_e = (E_e - b) / a."""
    ene = np.asarray(ene, np.float64).ravel()
    kern = jackson_kernel(nmom)
    w = np.zeros((nmom, len(ene)), np.complex128, order="F")
    for e, en in enumerate(ene):
        th = np.arccos((en - b) / a)
        for i in range(nmom):
            w[i, e] = kern[i] * (-1j * np.exp(-1j * i * th)) / np.sqrt(a ** 2 - (en - b) ** 2)
    return w


def bloch_map(H, a, b, sources, lld, cr, cell, kpts, w, group=None, ngroup=1):
    """(18,18,ne,nk,ngroup,nsrc) as the library call defines g_k.  kpts (3,nk); w (2 lld + 2, ne); group (kk) with values 0..ngroup or None."""
    nmom, kk = 2 * lld + 2, H.shape[0] // 18
    kpts = np.asarray(kpts, np.float64).reshape(3, -1)
    w = np.asarray(w, np.complex128)
    assert w.shape[0] == nmom
    ne = w.shape[1]
    group = np.ones(kk, np.int32) if group is None else np.asarray(group)
    out = np.zeros((18, 18, ne, kpts.shape[1], ngroup, len(sources)), np.complex128, order="F")
    acc = {}
    for s, src in enumerate(sources):
        src = int(src)
        if src not in acc:
            psi = chain_blocks(H, a, b, src, nmom)
            y = np.zeros((kk, 18, 18, ne), np.complex128)
            for n in range(nmom):                                # order by order, as the chain delivers the vectors
                y += psi[..., n, None] * w[n][None, None, None, :]
            acc[src] = y
        ph = np.exp(-1j * (kpts.T @ displacements(cr, src, cell)))           # (nk, kk)
        for g in range(ngroup):
            out[:, :, :, :, g, s] = np.einsum("qj,jabe->abeq", ph * (group == g + 1)[None, :], acc[src])
    return out


def weighted_moments(mom, w):
    """sum_n w(n, e) mom(:, :, n, ...) -> (18, 18, ne, ...): the weights applied to moments that exist (bloch_sums, bloch_hamiltonian_moments)."""
    return np.einsum("abn...,ne->abe...", mom, np.asarray(w, np.complex128))
