"""Drop-in counterpart of ``type(conductivity)`` (conductivity.f90:47-72): the energy-resolved Kubo-Bastin integrand on the GPU.

calculate_gamma_nm + calculate_conductivity_tensor (:158-268) become one call, ``rsrec_kubo_integrand``, that never forms the
(nE, cond_ll, cond_ll) array gamma_nm.  The Simpson integrations and the output files stay with the caller (host work of O(nE^2)).
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
        returns them, or ``None``: the moments that call left resident on the device (``rsrec_kubo_integrand_diag``).
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

    def timing(self):
        """(device ms of the last call, ms in its contraction kernels)."""
        t = self.recursion.timing()
        return t["total_ms"], t["rest_ms"]
