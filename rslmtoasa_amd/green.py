"""Host-side mirror of the reference's ``green`` type for the block-recursion Green function (green.f90:42-72, :588-621, :1191-1339).

Only the stage that sits directly on the recursion's output is here: ``block_green`` turns the block coefficients of the
sites this rank owns into ``g0(18,18,nE,site)`` on the GPU (``rsrec_block_green``).  The terminator ``a_inf, b_inf`` comes
from ``recursion%get_terminf`` (recursion.f90:2092), which stays on the CPU in the reference's own code and
is therefore an argument here.
"""
import numpy as np


def _ptr(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


class Green:
    def __init__(self, recursion, ene, sym_term=False):
        self.recursion = recursion
        self.ene = np.ascontiguousarray(ene, dtype=np.float64)      # energy%ene(1:channels_ldos+10), energy.f90:205-207
        self.sym_term = bool(sym_term)                              # control%sym_term
        self.g0 = None                                              # green%g0: allocated once, overwritten by every call (green.f90:150-170)

    def _g0_buffer(self, n):
        shape = (18, 18, len(self.ene), n)
        if self.g0 is None or self.g0.shape != shape:
            self.g0 = np.zeros(shape, dtype=np.complex128, order="F")
        return self.g0

    def _sites(self, site_offset, nsites_total):
        """The sites of this rank: their number and the number of sites in the zero-padded images (all ranks')."""
        start, end = self.recursion._my_sites()[:2]
        n = end - start + 1
        return n, (n + site_offset if nsites_total is None else nsites_total)

    def _ldos_args(self, site_offset, nsites_total, out):
        """The images of an LDOS stage and their addresses: host arrays, or ``out`` = (dtot, dosia, dosial) raw DEVICE addresses."""
        import ctypes as C
        n, ntot = self._sites(site_offset, nsites_total)
        nen = len(self.ene)
        if out is None:
            img = dict(dtot=np.zeros(nen), dosia=np.zeros((ntot, nen), order="F"), dosial=np.zeros((ntot, 18, nen), order="F"))
            ptrs = tuple(_ptr(img[k]) for k in ("dtot", "dosia", "dosial"))
        else:
            img = dict(dtot=None, dosia=None, dosial=None)
            ptrs = tuple(C.c_void_p(int(p)) for p in out)
        return self.recursion, n, nen, ntot, img, ptrs

    def block_green(self, a_inf, b_inf, eta=0.0 + 0.0j, nsites=None):
        """green%block_green: requires ``recursion.zsqr()`` to have been called (self.f90:829), like the reference."""
        rec = self.recursion
        n = rec.a_b.shape[3] if nsites is None else nsites
        lld = rec.a_b.shape[2]
        a_b = np.asfortranarray(rec.a_b[:, :, :, :n])
        b_s = np.asfortranarray(rec.b2_b[:, :, :, :n])
        a_inf = np.asfortranarray(a_inf, dtype=np.float64)
        b_inf = np.asfortranarray(b_inf, dtype=np.float64)
        assert a_inf.shape == (18, 18, n) and b_inf.shape == (18, 18, n)
        g0 = self._g0_buffer(n)
        rec._check(rec._L.rsrec_block_green(rec._h, n, lld, len(self.ene), _ptr(self.ene), float(np.real(eta)), float(np.imag(eta)),
                                            int(self.sym_term), _ptr(a_inf), _ptr(b_inf), _ptr(a_b), _ptr(b_s), _ptr(g0)))
        return g0

    def density(self, dw_l=None, cshi=None, nsites=None, nmdir=1):
        """dos%density for every site (and direction) of the last scalar recursion (density_of_states.f90:248-363, bprldos :370-404):
        ``recursion.a, recursion.b2 (llmax,18,site[,mdir])`` -> ``tdens (18, nE, site, mdir)`` on the GPU.  ``dw_l, cshi (18, site)`` are the
        potential parameters the reference reads (potential.f90:392-393: 1 and 0 unless set)."""
        rec = self.recursion
        a = np.asarray(rec.a); b2 = np.asarray(rec.b2)
        if a.ndim == 3:
            a = a[:, :, :, None]; b2 = b2[:, :, :, None]
        n = a.shape[2] if nsites is None else nsites
        a = np.asfortranarray(a[:, :, :n, :nmdir], dtype=np.float64); b2 = np.asfortranarray(b2[:, :, :n, :nmdir], dtype=np.float64)   # control%nmdir directions
        llmax, nmd = a.shape[0], a.shape[3]
        dw = np.ones((18, n), order="F") if dw_l is None else np.asfortranarray(dw_l, dtype=np.float64)
        cs = np.zeros((18, n), order="F") if cshi is None else np.asfortranarray(cshi, dtype=np.float64)
        assert dw.shape == (18, n) and cs.shape == (18, n)
        tdens = np.zeros((18, len(self.ene), n, nmd), order="F")
        rec._check(rec._L.rsrec_scalar_density(rec._h, n, nmd, llmax, int(rec.control.lld), _ptr(a), _ptr(b2), len(self.ene), _ptr(self.ene), _ptr(dw), _ptr(cs), _ptr(tdens)))
        self.tdens = tdens
        return tdens

    def sgreen(self, dw_l=None, cshi=None, nsites=None):
        """green%sgreen (green.f90:628-705) for control%nmdir = 1: g0(j,j,ie,ia) = -i pi doso(j,ie) with doso = dos%density on the GPU."""
        t = self.density(dw_l, cshi, nsites)
        assert t.shape[3] == 1, "sgreen: the nmdir = 3 combination (green.f90:684-699) stays the reference's host loop over density's output"
        g0 = self._g0_buffer(t.shape[2])
        g0[...] = 0.0
        for j in range(18):
            g0[j, j] = -1j * t[j, :, :, 0] * np.pi
        return g0

    def terminator(self, nsites=None):
        """recursion%get_terminf (recursion.f90:2092) on the GPU for the coefficients held by the recursion object (b2_b after zsqr):
        returns a_inf, b_inf (18,18,n) and the mean diagonals a_inf0, b_inf0 (n)."""
        rec = self.recursion
        n = rec.a_b.shape[3] if nsites is None else nsites
        lld = rec.a_b.shape[2]
        a_b = np.asfortranarray(rec.a_b[:, :, :, :n])
        b_s = np.asfortranarray(rec.b2_b[:, :, :, :n])
        a_inf = np.zeros((18, 18, n), np.float64, order="F")
        b_inf = np.zeros_like(a_inf)
        a0, b0 = np.zeros(n), np.zeros(n)
        rec._check(rec._L.rsrec_terminator(rec._h, n, lld, _ptr(a_b), _ptr(b_s), _ptr(a_inf), _ptr(b_inf), _ptr(a0), _ptr(b0)))
        return a_inf, b_inf, a0, b0

    def block_ldos(self, eta=0.0 + 0.0j, site_offset=0, nsites_total=None, out=None):
        """The LDOS stage for the sites of the last ``recur_b`` call, entirely on the device from the coefficients that call left
        there: zsqr -> get_terminf -> bgreen -> the reduction of bands%calculate_fermi (bands.f90:258-268).  Returns a dict with the
        zero-padded images ``dtot(nen)``, ``dosia(nsites_total, nen)``, ``dosial(nsites_total, 18, nen)`` and the terminators used.
        ``out`` = (dtot, dosia, dosial) raw DEVICE addresses (e.g. ``tensor.data_ptr()``): the images are written there in place."""
        rec, n, nen, ntot, img, ptrs = self._ldos_args(site_offset, nsites_total, out)
        a_inf = np.zeros((18, 18, n), np.float64, order="F")
        b_inf = np.zeros_like(a_inf)
        rec._check(rec._L.rsrec_block_ldos(rec._h, nen, _ptr(self.ene), float(np.real(eta)), float(np.imag(eta)), int(self.sym_term),
                                           int(site_offset), int(ntot), ptrs[0], ptrs[1], ptrs[2], _ptr(a_inf), _ptr(b_inf)))
        return dict(img, a_inf=a_inf, b_inf=b_inf)

    def contour_occupation(self, x, w, e0, kind="block", site_offset=0, nsites_total=None, diag=False, resident=False, coef=None, a_inf=None, b_inf=None):
        """The orbital occupations of bands%calculate_moments_gauss_legendre / calculate_occupation_gauss_legendre (bands.f90:559-586,
        :631-650) on the Gauss-Legendre contour at ``e0`` = ene(fermi_point), in one call (``rsrec_contour_occupation``): returns
        occ (18, nsites_total), then g_ii at every point (18, npts, nsites) if ``diag``.

        ``x, w``: nodes and weights on (0, 1).  ``kind``: "block" (block_green_eta) or "chebyshev" (chebyshev_green_eta, the diagonal
        only).  Chains: ``resident=True`` reads what the last ``recur_b`` / ``chebyshev_recur`` left on the device; else ``coef`` (a_b, b_sqrt) / (mu_n,) if
        given (numpy arrays or device tensors in that memory order, one chain per site of this rank), else the recursion's arrays (a_b,
        b2_b after zsqr / mu_n).  Terminators: ``a_inf, b_inf`` (18,18,nsites) or None (computed on the device, once per chain)."""
        rec = self.recursion
        k = {"block": 0, "chebyshev": 1}[kind] if isinstance(kind, str) else int(kind)
        n, ntot = self._sites(site_offset, nsites_total)
        lld = int(rec.control.lld)
        x, w = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
        if x.ndim != 1 or x.shape != w.shape:
            raise ValueError("x and w must be one-dimensional and alike, got %r and %r" % (x.shape, w.shape))
        ca = cb = None
        if not resident and coef is not None:
            arrs = [a if hasattr(a, "data_ptr") else np.asfortranarray(a, dtype=np.complex128) for a in coef]
            ca, cb = arrs[0], (arrs[1] if len(arrs) > 1 else None)
            n = int(ca.shape[0] if hasattr(ca, "data_ptr") else ca.shape[3])
            lld = int(ca.shape[1] if hasattr(ca, "data_ptr") else ca.shape[2])
            lld = lld if k == 0 else (lld - 2) // 2
            ntot = n + site_offset if nsites_total is None else nsites_total
        elif not resident:
            if k == 0:
                ca = np.asfortranarray(rec.a_b[:, :, :, :n], dtype=np.complex128)
                cb = np.asfortranarray(rec.b2_b[:, :, :, :n], dtype=np.complex128)
            else:
                ca = np.asfortranarray(rec.mu_n[:, :, :, :n], dtype=np.complex128)
        if a_inf is not None:
            a_inf, b_inf = np.asfortranarray(a_inf, dtype=np.float64), np.asfortranarray(b_inf, dtype=np.float64)
        from .exchange import _any_ptr as P             # numpy arrays, device tensors, None
        occ = np.zeros((18, ntot), order="F")
        gd = np.zeros((18, len(x), n), np.complex128, order="F") if diag else None
        rec._check(rec._L.rsrec_contour_occupation(rec._h, k, n, lld, len(x), _ptr(x), _ptr(w), float(e0), int(self.sym_term), float(rec.en.energy_min),
                                                   float(rec.en.energy_max), P(a_inf), P(b_inf), P(ca), P(cb), int(site_offset), int(ntot), _ptr(occ), P(gd)))
        return (occ, gd) if diag else occ

    def chebyshev_green(self, nsites=None):
        """green%chebyshev_green (green.f90:1030-1108): g0 from the Chebyshev moments ``recursion.mu_n``."""
        rec = self.recursion
        n = rec.mu_n.shape[3] if nsites is None else nsites
        lld = (rec.mu_n.shape[2] - 2) // 2
        mu = np.asfortranarray(rec.mu_n[:, :, :, :n])
        g0 = self._g0_buffer(n)
        rec._check(rec._L.rsrec_chebyshev_green(rec._h, n, lld, len(self.ene), _ptr(self.ene), float(rec.en.energy_min), float(rec.en.energy_max),
                                                _ptr(mu), _ptr(g0)))
        return g0

    def chebyshev_ldos(self, site_offset=0, nsites_total=None, out=None):
        """The LDOS stage for the sites of the last ``chebyshev_recur`` call, on the device from the moments that call left there:
        the diagonal of green%chebyshev_green -> the reduction of bands%calculate_fermi (bands.f90:258-268).  Returns a dict with the
        zero-padded images ``dtot(nen)``, ``dosia(nsites_total, nen)``, ``dosial(nsites_total, 18, nen)``, as ``block_ldos`` does.
        ``out`` = (dtot, dosia, dosial) raw DEVICE addresses: the images are written there in place."""
        rec, n, nen, ntot, img, ptrs = self._ldos_args(site_offset, nsites_total, out)
        rec._check(rec._L.rsrec_chebyshev_ldos(rec._h, nen, _ptr(self.ene), float(rec.en.energy_min), float(rec.en.energy_max),
                                               int(site_offset), int(ntot), ptrs[0], ptrs[1], ptrs[2]))
        return img

    def _spectra_args(self, ops, site_offset, nsites_total, out):
        """Operators as complex (nop, 18, 18) C-ordered stacks of column-major matrices are what the library reads: ``ops[k]`` is O_k as
        numpy indexes it (row, column), so each matrix is transposed into column-major storage here.  A device tensor is passed as it is
        and must hold that layout already (``[k][column][row]``, complex128)."""
        import ctypes as C
        rec = self.recursion
        ntot = self._sites(site_offset, nsites_total)[1]
        if hasattr(ops, "data_ptr"):
            nop, keep, optr = int(ops.shape[0]), ops, C.c_void_p(int(ops.data_ptr()))
        else:
            o = np.asarray(ops, dtype=np.complex128)
            if o.ndim == 2:
                o = o[None]
            if o.ndim != 3 or o.shape[1:] != (18, 18):
                raise ValueError("ops must be (nop, 18, 18), got %r" % (o.shape,))
            keep = np.ascontiguousarray(o.transpose(0, 2, 1))           # [k][column][row]
            nop, optr = keep.shape[0], _ptr(keep)
        if out is None:
            spec = np.zeros((nop, len(self.ene), ntot), order="F")
            sptr = _ptr(spec)
        else:
            spec, sptr = None, C.c_void_p(int(out))
        return rec, nop, keep, optr, ntot, spec, sptr

    def block_spectra(self, ops, eta=0.0 + 0.0j, site_offset=0, nsites_total=None, out=None):
        """``spec(k, ie, s) = Im Tr(ops[k] g0(:,:,ie,s))`` for the sites of the last ``recur_b`` call, on the device from the coefficients
        that call left there (zsqr -> get_terminf -> bgreen with the contraction as its epilogue: ``rsrec_block_spectra``).  No g0 is
        formed in memory and no -1/pi is applied.  Returns the zero-padded image (nop, nen, nsites_total); ``out`` = raw DEVICE address of
        such an image (Fortran order), written in place (None is returned)."""
        rec, nop, keep, optr, ntot, spec, sptr = self._spectra_args(ops, site_offset, nsites_total, out)
        rec._check(rec._L.rsrec_block_spectra(rec._h, nop, optr, len(self.ene), _ptr(self.ene), float(np.real(eta)), float(np.imag(eta)),
                                              int(self.sym_term), int(site_offset), int(ntot), sptr))
        return spec

    def chebyshev_spectra(self, ops, site_offset=0, nsites_total=None, out=None):
        """``block_spectra`` for the sites of the last ``chebyshev_recur`` call: g0 is green%chebyshev_green's, formed from the moments on
        the device through the traces ``Tr(ops[k] mu_i)`` (``rsrec_chebyshev_spectra``)."""
        rec, nop, keep, optr, ntot, spec, sptr = self._spectra_args(ops, site_offset, nsites_total, out)
        rec._check(rec._L.rsrec_chebyshev_spectra(rec._h, nop, optr, len(self.ene), _ptr(self.ene), float(rec.en.energy_min), float(rec.en.energy_max),
                                                  int(site_offset), int(ntot), sptr))
        return spec

    def spectra_integrals(self, nv1, nv1_fermi, edel, e1, fermi, spec=None, comb=None, nop=None, nsites=None, site_offset=0, nsites_total=None,
                          want=("mom", "cum"), out=None):
        """The integrals that follow the spectra (``rsrec_spectra_integrals``): for every series ``y = comb . spec`` of every site,
        ``cum(s, i, site)`` = the reference's ``simpson_f`` (Fermi weights, T = 0) up to every mesh energy ``ene[i]`` and
        ``mom(p, s, site)`` = its ``simpson_m`` of order p = 0, 1, 2 up to the Fermi level.  Returns ``(mom, cum)``, the zero-padded images
        (3, nser, nsites_total) and (nser, nen, nsites_total); an entry not in ``want`` is None.

        ``spec``: the image (nop, nen, nsites_total) of ``block_spectra`` / ``chebyshev_spectra``, a numpy array or a device tensor in that
        memory order; None: the image the last of those calls left on the device (``nop`` must then be given).  ``comb``: (nop, nser,
        nsites) as ``bands.series_table`` builds it, numpy or device; None: the rows themselves.  ``nv1``: the mesh's nv1 (the cumulative
        rule reads nv1 + 9 points); ``nv1_fermi, edel, e1, fermi``: bands%nv1, energy%edel, bands%e1, energy%fermi.
        ``out`` = (mom, cum) raw DEVICE addresses (or None each): written in place, None returned in their stead."""
        import ctypes as C
        from .exchange import _any_ptr as P
        rec = self.recursion
        nen = len(self.ene)
        if spec is None:
            if nop is None:
                raise ValueError("nop must be given with the resident image")
            n, ntot = self._sites(site_offset, nsites_total)
            n = n if nsites is None else int(nsites)
        else:
            if not hasattr(spec, "data_ptr"):
                spec = np.asfortranarray(spec, dtype=np.float64)
                if spec.ndim != 3 or spec.shape[1] != nen:
                    raise ValueError("spec must be (nop, %d, nsites_total), got %r" % (nen, spec.shape))
                nop, ntot = spec.shape[0], spec.shape[2]
            else:
                if nop is None or nsites_total is None:
                    raise ValueError("nop and nsites_total must be given with a device image")
                ntot = int(nsites_total)
            n = ntot - site_offset if nsites is None else int(nsites)
        nop = int(nop)
        if comb is None:
            nser = nop
        elif hasattr(comb, "data_ptr"):
            nser = int(comb.numel()) // (nop * n)
        else:
            comb = np.asfortranarray(comb, dtype=np.float64)
            if comb.ndim == 2:
                comb = np.asfortranarray(comb[:, :, None])
            if comb.shape[0] != nop or comb.shape[2] != n:
                raise ValueError("comb must be (%d, nser, %d), got %r" % (nop, n, comb.shape))
            nser = comb.shape[1]
        out = (None, None) if out is None else out
        mom = np.zeros((3, nser, ntot), order="F") if "mom" in want and out[0] is None else None
        cum = np.zeros((nser, nen, ntot), order="F") if "cum" in want and out[1] is None else None
        pm = C.c_void_p(int(out[0])) if out[0] is not None else P(mom)
        pc = C.c_void_p(int(out[1])) if out[1] is not None else P(cum)
        rec._check(rec._L.rsrec_spectra_integrals(rec._h, nop, P(spec), int(nser), P(comb), nen, _ptr(self.ene), int(nv1), int(nv1_fermi), float(edel),
                                                  float(e1), float(fermi), int(n), int(site_offset), int(ntot), pm, pc))
        return mom, cum

    def ldos(self):
        """Orbital-resolved local density of states, -Im g0_jj / pi (density_of_states.f90:248-260)."""
        d = np.arange(18)
        return -self.g0[d, d].imag / np.pi
