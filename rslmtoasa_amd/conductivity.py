"""Drop-in counterpart of ``type(conductivity)`` (conductivity.f90:47-72): the Kubo-Bastin conductivity on the GPU.

calculate_gamma_nm + the loops of calculate_conductivity_tensor (:158-281) become one call, ``rsrec_kubo_integrand``, that never forms
the (nE, cond_ll, cond_ll) array gamma_nm.  The tail of calculate_conductivity_tensor (:283-372) -- the sums over the vectors and the
orbitals and the Fermi-weighted Simpson integral of each of the 38 series up to every energy of the mesh -- is a second call,
``rsrec_kubo_conductivity`` (``tensor``).  Only the formatting of the output files stays with the caller.
``optical`` goes beyond the reference, which stops at DC: the frequency-dependent conductivity sigma(omega) from the same
orbital-diagonal moments (``rsrec_kubo_optical``).
"""
import ctypes as C

import numpy as np

from . import _lib


class Conductivity:
    def __init__(self, recursion):
        self.recursion = recursion
        self.en = recursion.en

    def integrand(self, mu_nm, ene, diag=None):
        """integrand_at(l, l, :, v) of calculate_conductivity_tensor, factor applied: complex (18, nen, nvec), Fortran order.

        ``mu_nm``: complex (18, 18, cond_ll, cond_ll, nvec) in the reference's layout (recursion%mu_nm_stochastic) -- a numpy array
        or a contiguous complex128 torch tensor on the GPU (Fortran order: the tensor's memory must be the reference's array).
        Also the orbital-diagonal moments alone, complex (18, cond_ll, cond_ll[, nvec]) as ``compute_moments_stochastic(diag=True)``
        returns them, or ``None``: the moments that call left resident on the device (``rsrec_kubo_integrand_diag``) -- after
        ``compute_moments_stochastic_multi`` / ``_tensor`` those of all sets, (18, nen, nvec * nout[ * nin]), set outermost.
        ``diag``: True / False says which of the two ``mu_nm`` is.  Left at None the shape decides; the one shape that is both --
        (18, 18, 18, 18): one vector's full moments at cond_ll = 18, or the diagonals of 18 vectors at cond_ll = 18 -- then means the
        full moments, as it always has: pass diag=True for the diagonals.
        ``ene``: energy%ene (channels_ldos + 10 points).  energy_min / energy_max come from the recursion's Energy."""
        ene = np.ascontiguousarray(ene, dtype=np.float64).ravel()
        rec = self.recursion
        if mu_nm is None:
            cond_ll, nvec = getattr(rec, "mu_diag_resident", None) or (1, 1)      # (nothing asked for yet: the library refuses with its message)
            return self._run(rec._L.rsrec_kubo_integrand_diag, nvec, cond_ll, None, ene)
        if hasattr(mu_nm, "data_ptr"):                     # torch tensor: read where it lies (GPU memory is not copied)
            if mu_nm.element_size() != 16 or not mu_nm.is_complex() or not mu_nm.is_contiguous():
                raise ValueError("a mu_nm tensor must be contiguous complex128 (the Fortran array seen from C: shape reversed)")
            if mu_nm.is_cuda:
                import torch
                torch.cuda.synchronize(mu_nm.device)       # the library reads it on its own stream
            shape, ptr, keep = tuple(mu_nm.shape)[::-1], C.c_void_p(mu_nm.data_ptr()), mu_nm
        else:
            keep = np.asfortranarray(mu_nm, dtype=np.complex128)
            shape, ptr = keep.shape, keep.ctypes.data_as(C.c_void_p)
        is_diag = len(shape) in (3, 4) and shape[0] == 18 and shape[1] == shape[2]         # the diagonals: (18, cond_ll, cond_ll[, nvec])
        is_full = len(shape) in (4, 5) and shape[:2] == (18, 18) and shape[2] == shape[3]   # (18, 18, cond_ll, cond_ll[, nvec])
        if diag is None:
            diag = is_diag and not is_full
        if diag:
            if not is_diag:
                raise ValueError("diagonal moments must be (18, cond_ll, cond_ll[, nvec]), got %s" % (shape,))
            if len(shape) == 3:
                shape = shape + (1,)
            out = self._run(rec._L.rsrec_kubo_integrand_diag, shape[3], shape[1], ptr, ene)
            del keep
            return out
        if len(shape) == 4:
            shape = shape + (1,)
        if len(shape) != 5 or shape[0] != 18 or shape[1] != 18 or shape[2] != shape[3]:
            raise ValueError("mu_nm must be (18, 18, cond_ll, cond_ll[, nvec]) or (18, cond_ll, cond_ll[, nvec]), got %s" % (shape,))
        out = self._run(rec._L.rsrec_kubo_integrand, shape[4], shape[2], ptr, ene)
        del keep
        return out

    def _run(self, fn, nvec, cond_ll, ptr, ene):
        out = np.zeros((18, ene.size, nvec), np.complex128, order="F")
        rec = self.recursion
        rec._check(fn(rec._h, int(nvec), int(cond_ll), ptr, ene.size, ene.ctypes.data_as(C.c_void_p),
                      float(self.en.energy_min), float(self.en.energy_max), out.ctypes.data_as(C.c_void_p)))
        return out

    def tensor(self, integrand, ene, nv1=None, per_vector=False, temperature=0.0, series=False):
        """The conductivity of calculate_conductivity_tensor's tail (:283-372): real (38, nen, nsets), Fortran order, with
        sigma[r, i, s] = simpson_f(x, EF = x[i], nv1, S[r, :, s], fermi = .true., T) on the scaled axis x = (ene - b)/a.

        Rows: 0 Re total, 1 Im total, 2-19 Re orbital 1..18, 20-37 Im orbital 1..18.  Sets from 0, as numpy indexes them (the C header and the Fortran side count from 1): set 0 is the sum over the vectors; with
        ``per_vector`` set 1 + v is vector v alone ('per_type').  NOT divided by the number of vectors: the reference divides when it
        prints (:321).  Terms simpson_f would read past the mesh are zero (include/rsrec.h).
        ``integrand``: complex (18, nen[, nvec]) as ``integrand()`` returns it -- a numpy array or a contiguous complex128 torch tensor
        on the GPU (Fortran order: shape reversed), read in place.
        ``nv1``: energy%nv1; left at None the Energy object's, or len(ene) - 9 (the mesh energy%e_mesh makes).
        ``temperature``: in K, the T simpson_f would be given on the unscaled axis; the rule runs on the scaled one, so the library gets T / a.
        ``series``: also return the integrated series S (38, nen, nsets); rows 0-1 of set 0 are fort.123's columns."""
        ene = np.ascontiguousarray(ene, dtype=np.float64).ravel()
        rec = self.recursion
        if hasattr(integrand, "data_ptr"):                 # torch tensor: read where it lies (GPU memory is not copied)
            if integrand.element_size() != 16 or not integrand.is_complex() or not integrand.is_contiguous():
                raise ValueError("an integrand tensor must be contiguous complex128 (the Fortran array seen from C: shape reversed)")
            if integrand.is_cuda:
                import torch
                torch.cuda.synchronize(integrand.device)   # the library reads it on its own stream
            shape, ptr, keep = tuple(integrand.shape)[::-1], C.c_void_p(integrand.data_ptr()), integrand
        else:
            keep = np.asfortranarray(integrand, dtype=np.complex128)
            shape, ptr = keep.shape, keep.ctypes.data_as(C.c_void_p)
        if len(shape) == 2:
            shape = shape + (1,)
        if len(shape) != 3 or shape[0] != 18 or shape[1] != ene.size:
            raise ValueError("integrand must be (18, nen[, nvec]) with nen = len(ene) = %d, got %s" % (ene.size, shape))
        if nv1 is None:
            nv1 = getattr(self.en, "nv1", None)
        if nv1 is None:
            nv1 = ene.size - 9
        nvec = shape[2]
        nsets = 1 + (nvec if per_vector else 0)
        a = (float(self.en.energy_max) - float(self.en.energy_min)) / float(np.float32(2.0) - np.float32(0.3))
        t_scaled = float(temperature) / a if np.isfinite(a) and a > 0 else float(temperature)      # (an empty window: the library refuses it)
        sigma = np.zeros((38, ene.size, nsets), np.float64, order="F")
        ser = np.zeros((38, ene.size, nsets), np.float64, order="F") if series else None
        rec._check(rec._L.rsrec_kubo_conductivity(rec._h, int(nvec), int(bool(per_vector)), ene.size, int(nv1), ene.ctypes.data_as(C.c_void_p),
                                                  float(self.en.energy_min), float(self.en.energy_max), t_scaled,
                                                  ptr, sigma.ctypes.data_as(C.c_void_p), ser.ctypes.data_as(C.c_void_p) if series else None))
        del keep
        return (sigma, ser) if series else sigma

    def optical(self, mu, ene, fermi, nw=None, temperature=0.0):
        """The optical conductivity sigma(omega) from the orbital-diagonal moments (``rsrec_kubo_optical``, include/rsrec.h has the
        formula): complex (18, nw, nfermi, nset), Fortran order; opt[l, k - 1, f, s] belongs to omega_k = k (ene[1] - ene[0]).

        ``mu``: the orbital diagonals, complex (18, cond_ll, cond_ll[, nset]) -- a numpy array or a contiguous complex128 torch tensor
        on the GPU (Fortran order: shape reversed), read in place -- or ``None``: the moments ``compute_moments_stochastic(diag=True)``
        / ``_multi`` / ``_tensor`` left resident on the device, all their sets.  A full (18, 18, cond_ll, cond_ll[, nvec]) array has
        its diagonals taken on the host.  The one shape that is both, (18, 18, 18, 18), means the full moments, as in ``integrand``.
        ``ene``: a uniform increasing mesh.  ``fermi``: one Fermi level or a sequence of up to 16, in the units of ``ene``.
        ``nw``: frequencies omega_1 .. omega_nw; left at None all nen - 1 the mesh holds.
        ``temperature``: in K on the unscaled axis; the weights are formed on the scaled one, so the library gets T / a as in ``tensor``."""
        ene = np.ascontiguousarray(ene, dtype=np.float64).ravel()
        fermi = np.ascontiguousarray(np.atleast_1d(fermi), dtype=np.float64).ravel()
        rec = self.recursion
        if nw is None:
            nw = ene.size - 1
        keep = None
        if mu is None:
            cond_ll, nset = getattr(rec, "mu_diag_resident", None) or (1, 1)      # (nothing asked for yet: the library refuses with its message)
            ptr = None
        else:
            if hasattr(mu, "data_ptr"):                    # torch tensor: read where it lies (GPU memory is not copied)
                if mu.element_size() != 16 or not mu.is_complex() or not mu.is_contiguous():
                    raise ValueError("a mu tensor must be contiguous complex128 (the Fortran array seen from C: shape reversed)")
                shape = tuple(mu.shape)[::-1]
                if len(shape) in (4, 5) and shape[:2] == (18, 18) and shape[2] == shape[3]:
                    mu = mu.cpu().numpy().transpose(tuple(range(len(shape)))[::-1])          # (the full moments: diagonals on the host below)
                elif mu.is_cuda:
                    import torch
                    torch.cuda.synchronize(mu.device)      # the library reads it on its own stream
            if not hasattr(mu, "data_ptr"):
                mu = np.asarray(mu)
                if mu.ndim in (4, 5) and mu.shape[:2] == (18, 18) and mu.shape[2] == mu.shape[3]:
                    idx = np.arange(18)
                    mu = mu[idx, idx]
                keep = np.asfortranarray(mu, dtype=np.complex128)
                shape, ptr = keep.shape, keep.ctypes.data_as(C.c_void_p)
            else:
                keep, ptr = mu, C.c_void_p(mu.data_ptr())
            if len(shape) == 3:
                shape = shape + (1,)
            if len(shape) != 4 or shape[0] != 18 or shape[1] != shape[2]:
                raise ValueError("mu must be (18, cond_ll, cond_ll[, nset]) or (18, 18, cond_ll, cond_ll[, nvec]), got %s" % (shape,))
            cond_ll, nset = shape[1], shape[3]
        a = (float(self.en.energy_max) - float(self.en.energy_min)) / float(np.float32(2.0) - np.float32(0.3))
        t_scaled = float(temperature) / a if np.isfinite(a) and a > 0 else float(temperature)      # (an empty window: the library refuses it)
        out = np.zeros((18, max(int(nw), 0), fermi.size, nset), np.complex128, order="F")
        rec._check(rec._L.rsrec_kubo_optical(rec._h, int(nset), int(cond_ll), ptr, ene.size, ene.ctypes.data_as(C.c_void_p),
                                             float(self.en.energy_min), float(self.en.energy_max), int(nw), fermi.size,
                                             fermi.ctypes.data_as(C.c_void_p), t_scaled, out.ctypes.data_as(C.c_void_p)))
        del keep
        return out

    def _single_shot(self, weights, per_call, pairs, v_a, v_b, energies, cond_ll, vo_a, vo_b, seeds, coefs, atlist):
        """``Recursion.kubo_single_shot`` on the weights ``weights(energies, ...)`` of ``per_call`` energies at a time; ``pairs``: an
        energy is the sum of two adjacent columns."""
        ene = np.atleast_1d(np.asarray(energies, np.float64)).ravel()
        rec = self.recursion
        parts = []
        for i0 in range(0, ene.size, per_call):
            wl, wr = weights(ene[i0:i0 + per_call], cond_ll, float(self.en.energy_min), float(self.en.energy_max))
            s = rec.kubo_single_shot(v_a, v_b, wl, wr, vo_out=vo_a, vo_b=vo_b, seeds=seeds, coefs=coefs, atlist=atlist)[:, :, :, 0]
            parts.append(s[:, 0::2] + s[:, 1::2] if pairs else s)
        if not parts:
            raise ValueError("no energies given")
        return np.asfortranarray(np.concatenate(parts, axis=1))

    def integrand_at(self, v_a, v_b, energies, cond_ll, vo_a=None, vo_b=None, seeds=None, coefs=None, atlist=None):
        """The Kubo-Bastin integrand at a few energies without the moments (``rsrec_kubo_single_shot`` on ``kubo_bastin_weights``): complex
        (18, nE, nvec), what ``integrand(compute_moments_stochastic(v_a, v_b, cond_ll, ..., diag=True), ene)`` gives at those energies,
        to rounding.  Neither a left matrix nor a cond_ll x cond_ll contraction is formed, so cond_ll may be in the thousands on a
        10^5-atom cell.  Runs 8 energies per call (two weight columns each): more energies rerun the chains, once per 8.  A Fermi-sea
        integral over the whole mesh (``tensor``) still needs the moments."""
        from .recursion import kubo_bastin_weights
        return self._single_shot(kubo_bastin_weights, 8, True, v_a, v_b, energies, cond_ll, vo_a, vo_b, seeds, coefs, atlist)

    def greenwood(self, v_a, v_b, energies, cond_ll, vo_a=None, vo_b=None, seeds=None, coefs=None, atlist=None):
        """The Kubo-Greenwood sums s(l, E, v) = sum_{n,m} d(m, E) d(n, E) mu(l, l, n, m, v), the stochastic estimate of the orbital-diagonal
        part of Tr[v_a delta(E - H) v_b delta(E - H)] with the Jackson-damped delta of ``kubo_greenwood_weights``: complex (18, nE, nvec).
        Up to 16 energies per call; more rerun the chains, once per 16.  Prefactors (pi hbar e^2 / volume) and the average over the vectors
        are the caller's."""
        from .recursion import kubo_greenwood_weights
        return self._single_shot(kubo_greenwood_weights, 16, False, v_a, v_b, energies, cond_ll, vo_a, vo_b, seeds, coefs, atlist)

    def spreading(self, evo, energies, energy_min, energy_max, tau, stride, jackson=True):
        """The energy-resolved mean-square spreading of the wave packets of ``Recursion.evolve`` (the Roche-Mayou route to sigma(E)):
        DX^2(E, t_s) = Tr[delta(E - H) (X(t_s) - X)^2] / Tr delta(E - H), estimated on the call's vectors as
        sum_n d_n(E) M_n(s) / sum_n d_n(E) M0_n with M_n(s) = Re sum_{l,v} m_diag(l, n, s, v), M0_n = Re sum_{l,v} m0_diag(l, n, v)
        and d_n(E) = g_n (2 - delta_n1) T_{n-1}(x) / (pi a sqrt(1 - x^2)), x = (E - b) / a: the expansion of delta(E - H) in the mom
        moments of the call, with the Jackson kernel g_n of mom terms (math.f90:1641-1655) unless ``jackson=False``.
        ``evo``: the dict ``Recursion.evolve`` returned with mom > 0; ``energy_min``, ``energy_max``: the window its a, b came from
        (``chebyshev_scaling``); ``tau``, ``stride``: the step and the steps per record of that call, t_s = s stride tau.  Host numpy.
        Returns a dict: ``t`` (nt), ``dos`` (nE) = sum_n d_n M0_n (the sum over the vectors, not their mean), ``dx2`` (nE, nt) and
        ``diffusion`` (nE, nt) = DX^2 / t_s.  sigma(E) = e^2 rho(E) max_t D(E, t) with the caller's rho per volume; where the DOS
        estimate is not positive the ratio is NaN."""
        from .recursion import _chebyshev_t, _scaled_energies
        if "m_diag" not in evo or "m0_diag" not in evo:
            raise ValueError("spreading needs the m_diag and m0_diag of an evolve call with mom > 0")
        md, m0 = np.asarray(evo["m_diag"]), np.asarray(evo["m0_diag"])
        mom, nt = md.shape[1], md.shape[2]
        x, a = _scaled_energies(energies, energy_min, energy_max, 1 << 30, "spreading", window=False)
        n = np.arange(mom, dtype=np.float64)
        if jackson:
            th = np.pi * n / (mom + 1.0)
            kern = ((mom - n + 1.0) * np.cos(th) + np.sin(th) / np.tan(np.pi / (mom + 1.0))) / (mom + 1.0)
        else:
            kern = np.ones(mom)
        kern[1:] *= 2.0
        d = kern[:, None] * _chebyshev_t(x, mom) / (np.pi * abs(a) * np.sqrt(1.0 - x ** 2))[None, :]         # (mom, nE)
        num = d.T @ md.real.sum(axis=(0, 3))                                                                 # (nE, nt)
        dos = d.T @ m0.real.sum(axis=(0, 2))                                                                 # (nE)
        t = np.arange(1, nt + 1, dtype=np.float64) * float(stride) * float(tau)
        with np.errstate(divide="ignore", invalid="ignore"):
            dx2 = np.where(dos[:, None] > 0, num / dos[:, None], np.nan)
        return {"t": t, "dos": dos, "dx2": dx2, "diffusion": dx2 / t[None, :]}

    def timing(self):
        """(device ms of the last call, ms in its kernels): after ``integrand`` the contraction kernels; after ``tensor`` the series and
        integral kernels, which are all of that call's device work, so the two values are equal; after ``optical`` the table kernels and
        the two stages of every chunk."""
        t = self.recursion.timing()
        return t["total_ms"], t["rest_ms"]
