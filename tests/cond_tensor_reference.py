"""numpy restatement of the conductivity tail, calculate_conductivity_tensor (conductivity.f90:283-372), as rsrec_kubo_conductivity
computes it (rslmtoasa_amd/csrc/kernels_cond.hpp: k_cond_series, k_cond_tensor), in the reference's operation order:

  * the 38 series of every set -- Re and Im of the total and of the 18 orbitals; set 0 the sum over the vectors, set 1 + v vector v;
  * sigma(r, i, s) = simpson_f(x, EF = x(i), nv1, S(r, :, s), fermi = .true., .false., T) (math.f90:1600-1632, fermifun :994-1000),
    every term with an index above nen taken as zero (the reference reads one element past its arrays there).

The loops run over the Simpson index I and are vectorised over (row, limit), so every element sees the reference's sequence of IEEE
operations: no FMA, no reordering.  exp overflows to inf far above the limit by design (1 / (inf + 1) = 0)."""
import numpy as np

from cond_reference import scaling

KB = 0.633362019e-5
NROW = 38


def kbt(T):
    return KB * T + 1.0e-15


def scaled_axis(ene, energy_min, energy_max):
    a, b = scaling(energy_min, energy_max)
    return (np.asarray(ene, np.float64) - b) / a


def series(integ, per_vector):
    """integ: complex (18, nen, nvec) -> real (38, nen, nsets), nsets = 1 + (nvec if per_vector else 0)."""
    integ = np.asarray(integ, np.complex128)
    _, nen, nvec = integ.shape
    nsets = 1 + (nvec if per_vector else 0)
    S = np.zeros((NROW, nen, nsets), order="F")

    def fill(s, re, im):
        tr, ti = np.zeros(nen), np.zeros(nen)
        for l in range(18):
            tr = tr + re[l]
            ti = ti + im[l]
        S[0, :, s], S[1, :, s], S[2:20, :, s], S[20:38, :, s] = tr, ti, re, im

    re, im = np.zeros((18, nen)), np.zeros((18, nen))
    for v in range(nvec):
        re = re + integ[:, :, v].real
        im = im + integ[:, :, v].imag
    fill(0, re, im)
    for v in range(nsets - 1):
        fill(1 + v, integ[:, :, v].real, integ[:, :, v].imag)
    return S


def weights(x, xi, T):
    """f[k, i] = fermifun(x[k], xi[i], kBT) (math.f90:994-1000)."""
    with np.errstate(over="ignore"):
        return 1.0 / (np.exp((x[:, None] - xi[None, :]) / kbt(T)) + 1.0)


def _rule(x, nv1, Y, T, chunk=256):
    """Rows Y (R, nen) -> (R, nen): column i is the sum A of simpson_f with EF = x[i].  The limits are independent of each other and go
    in chunks that stay in cache; the operations on an element are the reference's, one after the other."""
    nen = x.size
    assert Y.shape[1] == nen and nen >= nv1 + 9
    npad = max(nen, nv1 + 10)
    Yp = np.zeros((npad, Y.shape[0], 1))                   # zero from nen on, as the weights
    Yp[:nen, :, 0] = Y.T
    Y4 = 4.0 * Yp
    A = np.zeros((Y.shape[0], nen))
    for c0 in range(0, nen, chunk):
        xi = x[c0:c0 + chunk]
        f = np.zeros((npad, xi.size))
        f[:nen] = weights(x, xi, T)
        a, t = np.zeros((Y.shape[0], xi.size)), np.empty((Y.shape[0], xi.size))
        for I in range(2, nv1 + 10, 2):                    # do I = 2, NPTS + 9, 2:  A = ((A + Y(I-1) f(I-1)) + 4 Y(I) f(I)) + Y(I+1) f(I+1)
            k = I - 1
            for y, w in ((Yp[k - 1], f[k - 1]), (Y4[k], f[k]), (Yp[k + 1], f[k + 1])):
                np.multiply(y, w, out=t)
                a += t
        A[:, c0:c0 + chunk] = a
    return A


def simpson_limits(x, nv1, Y, T=0.0):
    """simpson_f of every row of Y (R, nen) up to every limit: (R, nen)."""
    x, Y = np.asarray(x, np.float64), np.asarray(Y, np.float64)
    return (x[1] - x[0]) * _rule(x, nv1, Y, T) / 3.0


def simpson_abs(x, nv1, Y, T=0.0):
    """(H / 3) sum_k |c_k y_k f_k| of the same sums, c_k the Simpson coefficients as the loop adds them up: the scale of their
    rounding-error bounds (a tolerance, so formed as one matrix product; its own rounding is immaterial)."""
    x, Y = np.asarray(x, np.float64), np.asarray(Y, np.float64)
    nen = x.size
    c = np.zeros(max(nen, nv1 + 10))
    for I in range(2, nv1 + 10, 2):
        c[I - 2:I + 1] += (1.0, 4.0, 1.0)
    return np.abs(x[1] - x[0]) * ((np.abs(Y) * c[:nen]) @ weights(x, x, T)) / 3.0


def n_terms(nv1):
    return 3 * ((nv1 + 9) // 2)


def _by_rows(fn, S, x, nv1, T):
    r, nen, nsets = S.shape
    rows = np.ascontiguousarray(S.transpose(0, 2, 1)).reshape(r * nsets, nen)
    return np.asfortranarray(fn(x, nv1, rows, T).reshape(r, nsets, nen).transpose(0, 2, 1))


def tensor(S, x, nv1, T=0.0):
    """sigma (38, nen, nsets) of the series S (38, nen, nsets) on the scaled axis x."""
    return _by_rows(simpson_limits, S, x, nv1, T)


def tensor_abs(S, x, nv1, T=0.0):
    """The bound scale of every element of tensor()."""
    return _by_rows(simpson_abs, S, x, nv1, T)
