"""Dense numpy restatement of rsrec_chebyshev_site_map, the per-atom blocks of functions of H from whole-lattice seeds.  Not a test module.

``site_map`` restates the call on ``pair_direct_reference.dense_h``: every vector x^v = sum_j c^v_j |j> (x) 1_18 placed with
``lattice_seed_reference.placed_coefficients`` (a later entry on the same atom overwrites), the three-term recurrence on the whole
vector, per order the projection z_n[j] = sum_v conj(c^v_j) [T_{n-1}(H~) x^v]_j, then the weights: D(:,:,e,j) = sum_n w(n,e) z_n[j].
``onsite_function`` is what the call estimates: the on-site blocks of sum_n w(n,e) T_{n-1}(H~) themselves."""
import numpy as np

from lattice_seed_reference import placed_coefficients


def site_map(H, a, b, seeds, coefs, lld, w):
    """(d_full (18,18,ne,kk), d_diag (18,ne,kk), cnorm (kk)) as the library call defines them.  seeds, coefs (nvec, nseed); w (2 lld + 2, ne)."""
    nmom, kk = 2 * lld + 2, H.shape[0] // 18
    w = np.asarray(w, np.complex128).reshape(nmom, -1)
    seeds, coefs = np.asarray(seeds).reshape(len(seeds), -1), np.asarray(coefs).reshape(len(seeds), -1)
    Ht = (H - b * np.eye(H.shape[0])) / a
    z = np.zeros((nmom, kk, 18, 18), np.complex128)
    cnorm = np.zeros(kk)
    for v in range(len(seeds)):
        c = placed_coefficients(kk, seeds[v], coefs[v])
        cnorm += np.abs(c) ** 2
        p0 = np.kron(c[:, None], np.eye(18))                               # (18 kk, 18): block j = c_j 1
        p1 = Ht @ p0
        for n in range(nmom):
            if n >= 2:
                p0, p1 = p1, 2.0 * (Ht @ p1) - p0
            z[n] += np.conj(c)[:, None, None] * (p0 if n == 0 else p1).reshape(kk, 18, 18)
    d_full = np.asfortranarray(np.einsum("ne,njab->abej", w, z))
    d_diag = np.asfortranarray(np.einsum("ne,njaa->aej", w, z))
    return d_full, d_diag, cnorm


def onsite_function(H, a, b, lld, w):
    """(18,18,ne,kk): block (j, j) of sum_n w(n, e) T_{n-1}(H~), from the dense polynomials."""
    nmom, kk = 2 * lld + 2, H.shape[0] // 18
    w = np.asarray(w, np.complex128).reshape(nmom, -1)
    Ht = (H - b * np.eye(H.shape[0])) / a
    t0, t1 = np.eye(H.shape[0], dtype=np.complex128), Ht.astype(np.complex128)
    out = np.zeros((18, 18, w.shape[1], kk), np.complex128, order="F")
    for n in range(nmom):
        if n >= 2:
            t0, t1 = t1, 2.0 * (Ht @ t1) - t0
        t = t0 if n == 0 else t1
        blocks = np.stack([t[18 * j:18 * j + 18, 18 * j:18 * j + 18] for j in range(kk)], axis=2)    # (18,18,kk)
        out += w[n][None, None, :, None] * blocks[:, :, None, :]
    return out


def worst(mine, ref):
    """Largest deviation relative to the largest element of the reference output."""
    return float(np.abs(np.asarray(mine) - ref).max() / np.abs(ref).max())
