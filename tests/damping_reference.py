"""numpy restatement of the traces of exchange%calculate_gilbert_damping (exchange.f90:674-694) as the reference writes them, for the
tests of rsrec_damping: matmul, transpose(conjg()), rtrace / imtrace of the triple product temp3.

gij / gji come from exchange_reference.intersite_parts (green.f90:446-453 and the Pauli parts, :455-467): the four 9 x 9 spin blocks of
gij are Ginmag + Giz, Gix - i Giy, Gix + i Giy and Ginmag - Giz, which inverts :457-460 up to one rounding of the block's scale.
The prefactor -0.25 * 2 / (pi spin_i) is not part of the traces; `factor` gives it with spin_i started at zero for every pair.
"""
import numpy as np

from exchange_reference import PI, intersite_parts


def gij_gji(g0, same):
    """g0 (18, 18, nE, 4) of the pair's chains -> gij, gji, each (nE, 18, 18)."""
    P = intersite_parts(g0, same)
    out = []
    for s in "ij":
        n, x, y, z = (P["G%s%s" % (s, c)] for c in ("nmag", "x", "y", "z"))
        G = np.zeros((n.shape[0], 18, 18), np.complex128)
        G[:, :9, :9] = n + z
        G[:, 9:, 9:] = n - z
        G[:, :9, 9:] = x - 1j * y
        G[:, 9:, :9] = x + 1j * y
        out.append(G)
    return out


def rtrace(m):
    return np.trace(m).real


def imtrace(m):
    return np.trace(m).imag


def damping_traces(gij, gji, tmati, tmatj):
    """gij, gji (nE, 18, 18); tmati, tmatj (18, 18, 3) -> dtott, dtottim, each (9, nE), m = 3 k + l (l fastest)."""
    nE = gij.shape[0]
    dtott, dtottim = np.zeros((9, nE)), np.zeros((9, nE))
    for nv in range(nE):
        Aij = gij[nv] - np.transpose(np.conj(gji[nv]))
        Aji = gji[nv] - np.transpose(np.conj(gij[nv]))
        m = 0
        for k in range(3):
            for l in range(3):
                temp1 = np.matmul(tmati[:, :, k], Aij)
                temp2 = np.matmul(np.transpose(np.conj(tmatj[:, :, l])), Aji)
                temp3 = np.matmul(temp1, temp2)
                dtott[m, nv] = rtrace(temp3)
                dtottim[m, nv] = imtrace(temp3)
                m += 1
    return dtott, dtottim


def damping_rows(g0, same, tmat):
    """One pair: the 18 rows (18, nE) of rsrec_damping, dtott then dtottim.  tmat: (18, 18, 3, 2), side i then side j."""
    gij, gji = gij_gji(g0, same)
    re, im = damping_traces(gij, gji, tmat[:, :, :, 0], tmat[:, :, :, 1])
    return np.concatenate([re, im])


def total_damping(rows_of_pairs):
    """total_damping (9, nE): dtott of the pairs added in ascending pair order (:690-694)."""
    total = np.zeros_like(rows_of_pairs[0][:9])
    for r in rows_of_pairs:
        total = total + r[:9]
    return total


def factor(ql_up, ql_dn):
    """-0.25 * 2 / (pi spin_i), spin_i = sum_l ql(1, l, 1) - ql(1, l, 2) accumulated from zero in the reference's order (:669-672, :704)."""
    spin = 0.0
    for u, d in zip(ql_up, ql_dn):
        spin = spin + u - d
    return (-0.25) * (2.0 / (PI * spin))
