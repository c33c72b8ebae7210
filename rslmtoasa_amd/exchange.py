"""Drop-in counterpart of ``type(exchange)``'s two main routines (exchange.f90:1032-1615) on the GPU.

green%calculate_intersite_gf + _twoindex (green.f90:386-469) and the integrands and Fermi-weighted Simpson integrals of
exchange%calculate_exchange + _twoindex become one call, ``rsrec_exchange``.  Neither g0 nor the 24 intersite arrays are formed: per
(pair, energy) the kernel reduces g0 of the pair's chains to 41 real integrands, and per pair to 67 numbers (kernels_exchange.hpp).
The traces of exchange%calculate_gilbert_damping (exchange.f90:674-694) come from the same chains through ``rsrec_damping``, the
auxiliary-GF exchange tensor of calculate_jij_auxgreen (:171-335) through ``rsrec_exchange_aux`` and the spin-lattice coupling of
calculate_jijk (:338-601) through ``rsrec_spin_lattice`` (kernels_auxgreen.hpp).
"""
import ctypes as C

import numpy as np

from . import _lib

NINT = 41   # integrand rows per (pair, energy), order in kernels_exchange.hpp
NDAMP = 18  # damping rows per (pair, energy): dtott (9, l fastest), then dtottim (9)
NAUX = 9    # Jij_aux rows per (pair, energy) and Jijk rows per (trio, energy): xx, xy, xz, yx, .. zz
NCONT = 13  # contour rows per (pair, point): jtot, jjtot(1:3), itot(3,3) (k fastest) = T_comm_xc's order


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _any_ptr(a):
    """Pointer of a numpy array or of a device tensor (complete before the call: the library reads it on its own stream)."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        import torch
        torch.cuda.synchronize(a.device)
        return C.c_void_p(a.data_ptr())
    return _ptr(a)


def exchange_dpar(c, dele, vmad, iz, pairs):
    """dpar (4,3,2,npairs) for rsrec_exchange from the potential parameters of the atom types (potential%c, %dele, %vmad).

    ``c, dele``: (ntype, 3, 2) -- per type, l = 0..2, spin up / down; ``vmad``: (ntype,); ``iz``: lattice%iz (1-based types per atom);
    ``pairs``: (npairs, 2) 1-based atoms (lattice%ijpair).  Per side (i, j) and l: (c_up + vmad, c_dn + vmad, dele_up, dele_dn), the
    sums formed in double as d_matrix forms them (symbolic_atom.f90:251-252); d_matrix's cmplx() then rounds them to single precision,
    which rsrec_exchange does too."""
    c, dele, vmad = np.asarray(c, np.float64), np.asarray(dele, np.float64), np.asarray(vmad, np.float64)
    iz, pairs = np.asarray(iz), np.asarray(pairs)
    out = np.zeros((4, 3, 2, len(pairs)), np.float64, order="F")
    for p, ij in enumerate(pairs):
        for side in range(2):
            t = int(iz[int(ij[side]) - 1]) - 1
            out[0, :, side, p] = c[t, :, 0] + vmad[t]
            out[1, :, side, p] = c[t, :, 1] + vmad[t]
            out[2, :, side, p] = dele[t, :, 0]
            out[3, :, side, p] = dele[t, :, 1]
    return out


def aux_apar(c, dele, vmad, iz, pairs):
    """apar (2,3,2,2,npairs) for rsrec_exchange_aux: (c + vmad, dele) per l, spin and side (atom i, atom j) of every pair, the sums formed
    in double as p_matrix forms them (symbolic_atom.f90:420); the library rounds them to single precision as the reference's cmplx() does.
    Arguments as ``exchange_dpar``."""
    c, dele, vmad = np.asarray(c, np.float64), np.asarray(dele, np.float64), np.asarray(vmad, np.float64)
    iz, pairs = np.asarray(iz), np.asarray(pairs)
    out = np.zeros((2, 3, 2, 2, len(pairs)), np.float64, order="F")
    for p, ij in enumerate(pairs):
        for side in range(2):
            t = int(iz[int(ij[side]) - 1]) - 1
            out[0, :, :, side, p] = c[t] + vmad[t]
            out[1, :, :, side, p] = dele[t]
    return out


def trio_apar(c, dele, vmad, qpar, iz, trios):
    """apar (3,3,2,3,ntrios) for rsrec_spin_lattice: (c + vmad, dele, qpar) per l, spin and atom (i, j, k) of every trio.
    ``qpar``: (ntype, 3, 2) like ``c``; ``trios``: (ntrios, 3) 1-based atoms (lattice%ijktrio(:, 1:3))."""
    c, dele, vmad, qpar = (np.asarray(a, np.float64) for a in (c, dele, vmad, qpar))
    iz, trios = np.asarray(iz), np.asarray(trios)
    out = np.zeros((3, 3, 2, 3, len(trios)), np.float64, order="F")
    for n, ijk in enumerate(trios):
        for atom in range(3):
            t = int(iz[int(ijk[atom]) - 1]) - 1
            out[0, :, :, atom, n] = c[t] + vmad[t]
            out[1, :, :, atom, n] = dele[t]
            out[2, :, :, atom, n] = qpar[t]
    return out


def trio_pairs(trios):
    """The pairs of the trios in the order lattice%ijpair holds them (lattice.f90:644-651): (i,j), (i,k), (j,k) per trio -> (3 ntrios, 2)."""
    t = np.asarray(trios, np.int32).reshape(-1, 3)
    return np.stack([t[:, [0, 1]], t[:, [0, 2]], t[:, [1, 2]]], axis=1).reshape(-1, 2)


def _factorial2(n):
    return 1.0 if n <= 0 else float(np.prod(np.arange(n, 0, -2)))


def _real_harmonic_p(u):
    """Real spherical harmonics of l = 1 at the unit vector u, m = -1, 0, 1 (y, z, x)."""
    k = np.sqrt(3.0 / (4.0 * np.pi))
    return {-1: k * u[1], 0: k * u[2], 1: k * u[0]}


def _ylm_grid(n=32):
    """Real spherical harmonics l = 0..2 in (l, m) order on a Gauss-Legendre x uniform-phi grid, with the quadrature weights."""
    x, w = np.polynomial.legendre.leggauss(n)
    phi = 2.0 * np.pi * np.arange(2 * n) / (2 * n)
    ct, ph = np.meshgrid(x, phi, indexing="ij")
    wt = np.repeat(w[:, None], 2 * n, axis=1) * (2.0 * np.pi / (2 * n))
    st = np.sqrt(1.0 - ct * ct)
    X, Y, Z = st * np.cos(ph), st * np.sin(ph), ct
    k0, k1 = 0.5 / np.sqrt(np.pi), np.sqrt(3.0 / (4.0 * np.pi))
    k2 = 0.5 * np.sqrt(15.0 / np.pi)
    ylm = {(0, 0): k0 + 0 * X, (1, -1): k1 * Y, (1, 0): k1 * Z, (1, 1): k1 * X,
           (2, -2): k2 * X * Y, (2, -1): k2 * Y * Z, (2, 0): 0.25 * np.sqrt(5.0 / np.pi) * (3 * Z * Z - 1), (2, 1): k2 * X * Z,
           (2, 2): 0.5 * k2 * (X * X - Y * Y)}
    return ylm, wt


def disp_matrix(disp_vec, ws_radius):
    """One 9 x 9 spin block of symbolic_atom%disp_matrix (symbolic_atom.f90:274-355) for lmax = 2, complex: the approximate displacement
    of the regular solution of the Laplace equation, in the program's orbital order s, px, py, pz, dxy, dyz, dzx, x2-y2, 3z2-r2.
    mat(l'm', lm) = -(4 pi / (3 ws_radius)) (2l-1)!! / (2l'-1)!! sum_m'' G(lm, l'm', 1m'') Y_1m''(u) for l' <= l, zero otherwise,
    with G the Gaunt coefficients of real harmonics (here by quadrature, exact for these degrees) and u the unit displacement."""
    d = np.asarray(disp_vec, np.float64)
    nrm = np.sqrt(np.sum(d * d))
    u = d / nrm if nrm != 0 else np.zeros(3)
    order = {(0, 0): 1, (1, -1): 3, (1, 0): 4, (1, 1): 2, (2, -2): 5, (2, -1): 6, (2, 0): 9, (2, 1): 7, (2, 2): 8}
    ylm, wt = _ylm_grid()
    y1 = _real_harmonic_p(u)
    mat = np.zeros((9, 9), np.complex128)
    for i in range(3):
        for j in range(3):
            if i > j:
                continue
            f = _factorial2(2 * j - 1) / _factorial2(2 * i - 1)
            for k in range(-i, i + 1):
                for n in range(-j, j + 1):
                    for m in (-1, 0, 1):
                        gaunt = float(np.sum(wt * ylm[(j, n)] * ylm[(i, k)] * ylm[(1, m)]))
                        mat[order[(i, k)] - 1, order[(j, n)] - 1] += f * gaunt * y1[m]
    return mat * ((-4.0 * np.pi) / (3.0 * ws_radius))


def damping_tmat(tmat, iz, pairs):
    """tmat (18,18,3,2,npairs) for rsrec_damping from hamiltonian%tmat (18,18,3,ntype): the type of atom i, then of atom j, per pair."""
    tmat, iz, pairs = np.asarray(tmat, np.complex128), np.asarray(iz), np.asarray(pairs)
    out = np.zeros((18, 18, 3, 2, len(pairs)), np.complex128, order="F")
    for p, ij in enumerate(pairs):
        for side in range(2):
            out[:, :, :, side, p] = tmat[:, :, :, int(iz[int(ij[side]) - 1]) - 1]
    return out


def contour_dmat(ee, iz, pairs):
    """dmat (9,9,2,npairs) for rsrec_exchange_contour from hamiltonian%ee (18,18,nnmax,ntype): per pair, of atom i then atom j,
    real(ee(1:9,1:9,1,iz) - ee(10:18,10:18,1,iz)) (exchange.f90:1819-1820) -- a dense matrix, unlike the diagonal d_matrix of ``exchange_dpar``."""
    ee, iz, pairs = np.asarray(ee), np.asarray(iz), np.asarray(pairs)
    out = np.zeros((9, 9, 2, len(pairs)), np.float64, order="F")
    for p, ij in enumerate(pairs):
        for side in range(2):
            t = int(iz[int(ij[side]) - 1]) - 1
            out[:, :, side, p] = np.real(ee[0:9, 0:9, 0, t] - ee[9:18, 9:18, 0, t])
    return out


def gauss_legendre(n, a=0.0, b=1.0):
    """n-point Gauss-Legendre nodes and weights on (a, b), the nodes in DESCENDING order as the reference's gauss_legendre returns them
    (math.f90:1763-1794): Newton's iteration on P_n from the Chebyshev guess, to 1e-14, the node pairs filled symmetrically."""
    x, w = np.zeros(n), np.zeros(n)
    for i in range(1, (n + 1) // 2 + 1):
        z = np.cos(np.pi * (i - 0.25) / (n + 0.5))
        while True:
            p1, p2 = 1.0, 0.0
            for j in range(1, n + 1):
                p1, p2 = ((2.0 * j - 1.0) * z * p1 - (j - 1.0) * p2) / j, p1
            pp = n * (z * p1 - p2) / (z * z - 1.0)
            z1, z = z, z - p1 / pp
            if abs(z - z1) <= 1e-14:
                break
        x[i - 1] = a + (b - a) * (z + 1) / 2
        x[n - i] = a + (b - a) * (1 - z) / 2
        w[i - 1] = w[n - i] = (b - a) * 2.0 / ((1.0 - z * z) * pp * pp) / 2
    return x, w


class Exchange:
    """``Exchange(recursion, green).compute(...)`` on the rank's pairs after recur_b_ij / chebyshev_recur_ij (block: and zsqr)."""

    def __init__(self, recursion, green):
        self.recursion = recursion
        self.green = green

    def compute(self, fermi, nv1, dpar, kind="block", integrand=False, cumulative=False, resident=False, a_inf=None, b_inf=None,
                pair_offset=0, npairs_total=None, coef=None):
        """Returns (xc, so, fo, parts) = T_comm_xc, T_comm_xcso, T_comm_xcfo (13, npairs_total), T_comm_xcparts (28, npairs_total),
        then jcum (nen, npairs) if ``cumulative`` and the integrand (41, nen, npairs) if ``integrand``.

        The pairs are lattice%ijpair of this rank.  Coefficients: ``resident=True`` reads the chains the last seeded recursion left on the
        device; else ``coef`` (a_b, b_sqrt) / (mu_n,) if given, else the recursion's arrays (a_b, b2_b after zsqr / mu_n).  Terminators:
        ``a_inf, b_inf`` (18,18,4*npairs) or None (computed on the device)."""
        rec = self.recursion
        ene, npairs, npairs_total, same, lld, k, ca, cb, a_inf, b_inf = self._call_setup(kind, resident, coef, a_inf, b_inf, npairs_total)
        dpar = np.asfortranarray(dpar, dtype=np.float64)
        xc = np.zeros((13, npairs_total), order="F")
        so, fo = np.zeros_like(xc), np.zeros_like(xc)
        parts = np.zeros((28, npairs_total), order="F")
        jcum = np.zeros((len(ene), npairs), order="F") if cumulative else None
        integ = np.zeros((NINT, len(ene), npairs), order="F") if integrand else None

        rec._check(rec._L.rsrec_exchange(rec._h, k, npairs, _ptr(same), lld, len(ene), _ptr(ene), int(nv1), float(fermi), int(self.green.sym_term),
                                          float(rec.en.energy_min), float(rec.en.energy_max), _ptr(a_inf), _ptr(b_inf), _any_ptr(ca), _any_ptr(cb), _ptr(dpar),
                                          int(pair_offset), int(npairs_total), _ptr(xc), _ptr(so), _ptr(fo), _ptr(parts), _ptr(jcum), _ptr(integ)))
        del ca, cb
        out = [xc, so, fo, parts]
        if cumulative:
            out.append(jcum)
        if integrand:
            out.append(integ)
        return tuple(out)

    def _call_setup(self, kind, resident, coef, a_inf, b_inf, npairs_total):
        """What rsrec_exchange and rsrec_damping take alike, for this rank's pairs: (ene, npairs, npairs_total, same, lld, kind, coef_a,
        coef_b, a_inf, b_inf).  Coefficients: None with ``resident``, else ``coef`` or the recursion's arrays; device tensors as they are."""
        rec, ene = self.recursion, np.ascontiguousarray(self.green.ene, dtype=np.float64)
        pairs = np.asarray(rec.lattice.ijpair, dtype=np.int32)
        from .recursion import site_partition
        start, end = site_partition(rec.rank, rec.nprocs, len(pairs))
        mine = pairs[start - 1:end]
        npairs = len(mine)
        npairs_total = len(pairs) if npairs_total is None else npairs_total
        same = np.ascontiguousarray(mine[:, 0] == mine[:, 1], dtype=np.int32)
        lld = int(rec.control.lld)
        k = {"block": 0, "chebyshev": 1}[kind] if isinstance(kind, str) else int(kind)
        ca = cb = None
        if not resident:
            if coef is not None:
                arrs = list(coef)
            elif k == 0:
                arrs = [rec.a_b[:, :, :, :4 * npairs], rec.b2_b[:, :, :, :4 * npairs]]
            else:
                arrs = [rec.mu_n[:, :, :, :4 * npairs]]
            arrs = [a if hasattr(a, "data_ptr") else np.asfortranarray(a, dtype=np.complex128) for a in arrs]
            ca = arrs[0]
            cb = arrs[1] if len(arrs) > 1 else None
        if a_inf is not None:
            a_inf, b_inf = np.asfortranarray(a_inf, dtype=np.float64), np.asfortranarray(b_inf, dtype=np.float64)
        return ene, npairs, npairs_total, same, lld, k, ca, cb, a_inf, b_inf

    def damping(self, tmat, ief, kind="block", rows=False, resident=False, coef=None, a_inf=None, b_inf=None, pair_offset=0, npairs_total=None):
        """Returns (at_ef, total) = the 9 real then 9 imaginary traces of every pair at ene(ief) (18, npairs_total) and total_damping
        (9, nen) of this rank's pairs, then the rows (18, nen, npairs) if ``rows``.  The prefactor -0.25 * 2 / (pi spin_i) is the caller's.

        ``tmat``: (18,18,3,2,npairs) complex, the torque matrices of atom i and atom j of this rank's pairs (``damping_tmat``), a numpy
        array or a device tensor in that memory order; ``ief``: 1-based energy index.  Pairs, coefficients and terminators as ``compute``."""
        rec = self.recursion
        ene, npairs, npairs_total, same, lld, k, ca, cb, a_inf, b_inf = self._call_setup(kind, resident, coef, a_inf, b_inf, npairs_total)
        if tmat is not None and not hasattr(tmat, "data_ptr"):
            tmat = np.asfortranarray(tmat, dtype=np.complex128)
            if tmat.shape != (18, 18, 3, 2, npairs):
                raise ValueError("tmat must be (18, 18, 3, 2, %d), got %r" % (npairs, tmat.shape))
        at_ef = np.zeros((NDAMP, npairs_total), order="F")
        total = np.zeros((9, len(ene)), order="F")
        out_rows = np.zeros((NDAMP, len(ene), npairs), order="F") if rows else None

        rec._check(rec._L.rsrec_damping(rec._h, k, npairs, _ptr(same), lld, len(ene), _ptr(ene), int(ief), int(self.green.sym_term),
                                         float(rec.en.energy_min), float(rec.en.energy_max), _ptr(a_inf), _ptr(b_inf), _any_ptr(ca), _any_ptr(cb), _any_ptr(tmat),
                                         int(pair_offset), int(npairs_total), _ptr(at_ef), _ptr(total), _ptr(out_rows)))
        del ca, cb
        return (at_ef, total, out_rows) if rows else (at_ef, total)

    def contour(self, x, w, e0, dmat, kind="block", resident=False, coef=None, a_inf=None, b_inf=None, pair_offset=0, npairs_total=None, rows=False):
        """green%calculate_intersite_gf_eta + exchange%calculate_exchange_gauss_legendre in one call (``rsrec_exchange_contour``): returns
        xc = T_comm_xc (13, npairs_total), then the weighted per-point values (13, npts, npairs) if ``rows``.

        ``x, w``: Gauss-Legendre nodes and weights on (0, 1) (``gauss_legendre``); ``e0`` = ene(fermi_point); ``dmat``: (9,9,2,npairs)
        (``contour_dmat``), a numpy array or a device tensor in that memory order.  Pairs, coefficients and terminators as ``compute``.
        An i == j pair takes gij = gji = g(chain 1), as calculate_intersite_gf does (the reference's contour routine defines no result there)."""
        rec = self.recursion
        _, npairs, npairs_total, same, lld, k, ca, cb, a_inf, b_inf = self._call_setup(kind, resident, coef, a_inf, b_inf, npairs_total)
        x, w = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
        if x.ndim != 1 or x.shape != w.shape:
            raise ValueError("x and w must be one-dimensional and alike, got %r and %r" % (x.shape, w.shape))
        if dmat is not None and not hasattr(dmat, "data_ptr"):
            dmat = np.asfortranarray(dmat, dtype=np.float64)
            if dmat.shape != (9, 9, 2, npairs):
                raise ValueError("dmat must be (9, 9, 2, %d), got %r" % (npairs, dmat.shape))
        xc = np.zeros((NCONT, npairs_total), order="F")
        out_rows = np.zeros((NCONT, len(x), npairs), order="F") if rows else None
        rec._check(rec._L.rsrec_exchange_contour(rec._h, k, npairs, _ptr(same), lld, len(x), _ptr(x), _ptr(w), float(e0), int(self.green.sym_term),
                                                  float(rec.en.energy_min), float(rec.en.energy_max), _ptr(a_inf), _ptr(b_inf), _any_ptr(ca), _any_ptr(cb),
                                                  _any_ptr(dmat), int(pair_offset), int(npairs_total), _ptr(xc), _ptr(out_rows)))
        del ca, cb
        return (xc, out_rows) if rows else xc

    def aux(self, fermi, nv1, apar, kind="block", rows=False, resident=False, coef=None, a_inf=None, b_inf=None, pair_offset=0, npairs_total=None):
        """exchange%calculate_jij_auxgreen in one call (``rsrec_exchange_aux``): returns jaux (9, npairs_total), the unscaled Simpson
        integrals of the tensor components xx, xy, .. zz (the reference prints them * 1.0d3 / 4 / pi; an i == j pair: J00 in row 0, zeros
        below), then the rows (9, nen, npairs) if ``rows``.  ``apar``: (2,3,2,2,npairs) (``aux_apar``), a numpy array or a device tensor
        in that memory order.  Pairs, coefficients and terminators as ``compute``."""
        rec = self.recursion
        ene, npairs, npairs_total, same, lld, k, ca, cb, a_inf, b_inf = self._call_setup(kind, resident, coef, a_inf, b_inf, npairs_total)
        if apar is not None and not hasattr(apar, "data_ptr"):
            apar = np.asfortranarray(apar, dtype=np.float64)
            if apar.shape != (2, 3, 2, 2, npairs):
                raise ValueError("apar must be (2, 3, 2, 2, %d), got %r" % (npairs, apar.shape))
        jaux = np.zeros((NAUX, npairs_total), order="F")
        out_rows = np.zeros((NAUX, len(ene), npairs), order="F") if rows else None
        rec._check(rec._L.rsrec_exchange_aux(rec._h, k, npairs, _ptr(same), lld, len(ene), _ptr(ene), int(nv1), float(fermi), int(self.green.sym_term),
                                              float(rec.en.energy_min), float(rec.en.energy_max), _ptr(a_inf), _ptr(b_inf), _any_ptr(ca), _any_ptr(cb),
                                              _any_ptr(apar), int(pair_offset), int(npairs_total), _ptr(jaux), _ptr(out_rows)))
        del ca, cb
        return (jaux, out_rows) if rows else jaux

    def spin_lattice(self, fermi, nv1, apar, dmat, kind="block", rows=False, resident=False, coef=None, a_inf=None, b_inf=None, trio_offset=0,
                     ntrios_total=None):
        """exchange%calculate_jijk in one call (``rsrec_spin_lattice``): returns jijk (9, ntrios_total), the unscaled Simpson integrals
        (the reference prints them * (1.0d3 / 8 / pi) * (13.605693122994 / 1.8897261246)), then the rows (9, nen, ntrios) if ``rows``.

        The rank's pairs are the trios' pairs, three per trio in the order (i,j), (i,k), (j,k) (``trio_pairs``).  ``apar``:
        (3,3,2,3,ntrios) (``trio_apar``); ``dmat``: (9,9,ntrios) complex, one spin block of disp_matrix of atom k for every trio's
        displacement (``disp_matrix``); numpy arrays or device tensors in that memory order.  Coefficients and terminators as ``compute``."""
        rec = self.recursion
        ene, npairs, _, same, lld, k, ca, cb, a_inf, b_inf = self._call_setup(kind, resident, coef, a_inf, b_inf, None)
        ntrios = npairs // 3
        ntrios_total = ntrios if ntrios_total is None else ntrios_total
        if apar is not None and not hasattr(apar, "data_ptr"):
            apar = np.asfortranarray(apar, dtype=np.float64)
            if apar.shape != (3, 3, 2, 3, ntrios):
                raise ValueError("apar must be (3, 3, 2, 3, %d), got %r" % (ntrios, apar.shape))
        if dmat is not None and not hasattr(dmat, "data_ptr"):
            dmat = np.asfortranarray(dmat, dtype=np.complex128)
            if dmat.shape != (9, 9, ntrios):
                raise ValueError("dmat must be (9, 9, %d), got %r" % (ntrios, dmat.shape))
        jijk = np.zeros((NAUX, ntrios_total), order="F")
        out_rows = np.zeros((NAUX, len(ene), ntrios), order="F") if rows else None
        rec._check(rec._L.rsrec_spin_lattice(rec._h, k, npairs, _ptr(same), lld, len(ene), _ptr(ene), int(nv1), float(fermi), int(self.green.sym_term),
                                              float(rec.en.energy_min), float(rec.en.energy_max), _ptr(a_inf), _ptr(b_inf), _any_ptr(ca), _any_ptr(cb),
                                              _any_ptr(apar), _any_ptr(dmat), int(trio_offset), int(ntrios_total), _ptr(jijk), _ptr(out_rows)))
        del ca, cb
        return (jijk, out_rows) if rows else jijk

    def timing(self):
        """(device ms of the last call, ms in its Green + trace + integration kernels)."""
        t = self.recursion.timing()
        return t["total_ms"], t["rest_ms"]
