"""numpy restatement of the integrals behind the SCF spectra, as rsrec_spectra_integrals computes them (rslmtoasa_amd/csrc/
kernels_moments.hpp), in the reference's operation order:

  * the series y(s, i, site) = 0.0 + sum_k comb(k, s, site) spec(k, i, site), k ascending;
  * cum(s, i) = simpson_f(ene, EF = ene(i), nv1, y(s, :), fermi = .true., .false., T = 0) (math.f90:1600-1632), every term with an index
    above nen taken as zero -- LIMIT BY LIMIT (cond_tensor_reference.simpson_limits: the whole rule with the Fermi weights of every limit)
    and in the PREFIX form of the kernels (one running sum over the triples below a limit, then the one or two triples that hold it);
  * mom(p, s) = simpson_m(.., H, EF, NPTS, y(s, :), EA, nexp = p, ene) (math.f90:1579-1598).

Loops run over the Simpson index and are vectorised over the rows, so every element sees the reference's sequence of IEEE operations:
no FMA, no reordering."""
import numpy as np

import cond_tensor_reference as CT


def series(spec, comb=None):
    """spec (nop, nen, nsites), comb (nop, nser, nsites) or None -> y (nser, nen, nsites)."""
    spec = np.asarray(spec, np.float64)
    if comb is None:
        return spec.copy()
    comb = np.asarray(comb, np.float64)
    y = np.zeros((comb.shape[1], spec.shape[1], spec.shape[2]))
    for k in range(spec.shape[0]):
        y = y + comb[k][:, None, :] * spec[k][None, :, :]
    return y


def cum_limits(ene, nv1, Y):
    """Rows Y (R, nen) -> (R, nen): simpson_f up to every limit, each limit evaluated on its own over the whole rule."""
    return CT.simpson_limits(ene, nv1, Y, 0.0)


def cum_prefix(ene, nv1, Y):
    """The same numbers from the prefix form: P[t] = the rule's sum after t triples with all weights 1; limit i starts from
    P[min(max((i - 1) // 2, 0), ntrip)] and adds the (at most two) triples that hold it with the weights 1 / 0.5 / 0."""
    ene, Y = np.asarray(ene, np.float64), np.asarray(Y, np.float64)
    R, nen = Y.shape
    assert nen >= nv1 + 9
    itop = nv1 + 9
    ntrip = itop // 2
    Yp = np.zeros((R, max(nen, itop + 1) + 2))
    Yp[:, :nen] = Y
    P = np.zeros((ntrip + 1, R))
    A = np.zeros(R)
    for t in range(ntrip):
        A = ((A + Yp[:, 2 * t]) + 4.0 * Yp[:, 2 * t + 1]) + Yp[:, 2 * t + 2]
        P[t + 1] = A
    out = np.zeros((R, nen))
    for i in range(nen):
        nfull = min(max((i - 1) // 2, 0), ntrip)
        A = P[nfull].copy()
        for I in range(2 * nfull + 2, min(2 * nfull + 4, itop) + 1, 2):
            k = I - 1
            w = [1.0 if q < i else (0.5 if q == i else 0.0) for q in (k - 1, k, k + 1)]
            w[1] = w[1] if k < nen else 0.0
            w[2] = w[2] if k + 1 < nen else 0.0
            A = ((A + Yp[:, k - 1] * w[0]) + 4.0 * Yp[:, k] * w[1]) + Yp[:, k + 1] * w[2]
        out[:, i] = (ene[1] - ene[0]) * A / 3.0
    return out


def n_terms_cum(nv1):
    return CT.n_terms(nv1)


def cum_abs(ene, nv1, Y):
    """(H / 3) sum_k |c_k y_k f_k| of every limit: the scale of the recursive-sum bound."""
    return CT.simpson_abs(ene, nv1, Y, 0.0)


def _power(e, p):
    return np.ones_like(e) if p == 0 else (e if p == 1 else e * e)


def simpson_m(h, ef, npts, Y, ea, nexp, ene):
    """Rows Y (R, nen) -> (R,): the reference's statement, term by term (4.d0*Y(I)*Ene(I)**nexp is (4 Y) (E**nexp))."""
    Y, ene = np.asarray(Y, np.float64), np.asarray(ene, np.float64)
    assert 1 <= npts and npts + 2 <= Y.shape[1]
    ep = _power(ene, nexp)
    A = np.zeros(Y.shape[0])
    for I in range(2, npts, 2):                                # do I = 2, NPTS - 1, 2
        k = I - 1
        A = ((A + Y[:, k - 1] * ep[k - 1]) + 4.0 * Y[:, k] * ep[k]) + Y[:, k + 1] * ep[k + 1]
    A = h * A / 3.0
    if ea != ef:
        n = npts - 1                                           # 0-based index of Y(NPTS)
        A = A + (ef - ea) * ((Y[:, n] * ep[n] + 4.0 * Y[:, n + 1] * ep[n + 1]) + Y[:, n + 2] * ep[n + 2]) / 6.0
    return A


def n_terms_m(npts):
    """terms of the main loop, the three of the end term, and the sum of the two parts"""
    return 3 * ((npts - 1) // 2) + 4


def simpson_m_abs(h, ef, npts, Y, ea, nexp, ene):
    """|H| / 3 sum |c_k y_k E_k^nexp| + |EF - EA| / 6 sum |c y E^nexp| of the end term: the scale of the recursive-sum bound."""
    Y, ene = np.abs(np.asarray(Y, np.float64)), np.asarray(ene, np.float64)
    ep = np.abs(_power(ene, nexp))
    c = np.zeros(Y.shape[1])
    for I in range(2, npts, 2):
        c[I - 2:I + 1] += (1.0, 4.0, 1.0)
    out = abs(h) * ((Y * ep) @ c) / 3.0
    if ea != ef:
        n = npts - 1
        out = out + abs(ef - ea) * (Y[:, n] * ep[n] + 4.0 * Y[:, n + 1] * ep[n + 1] + Y[:, n + 2] * ep[n + 2]) / 6.0
    return out


def integrals(spec, comb, ene, nv1, nv1_fermi, edel, e1, fermi, form=cum_limits):
    """mom (3, nser, nsites), cum (nser, nen, nsites) of an image of sites, as rsrec_spectra_integrals lays them out."""
    y = series(spec, comb)
    nser, nen, ns = y.shape
    mom, cum = np.zeros((3, nser, ns), order="F"), np.zeros((nser, nen, ns), order="F")
    for s in range(ns):
        cum[:, :, s] = form(ene, nv1, y[:, :, s])
        for p in range(3):
            mom[p, :, s] = simpson_m(edel, fermi, nv1_fermi, y[:, :, s], e1, p, ene)
    return mom, cum
