"""numpy restatement of exchange%calculate_jij_auxgreen (exchange.f90:171-335) and exchange%calculate_jijk (exchange.f90:338-601) as the
reference writes them, for the tests of rsrec_exchange_aux and rsrec_spin_lattice: p_matrix, transform_pmatrix and udisp_matrix
(symbolic_atom.f90:364-472), auxiliary_gij and transform_auxiliary_gij (green.f90:758-885) as matmul of full 18 x 18 matrices, the angle
table, imtrace, and simpson_f with Fermi weights (exchange_reference.simpson_f).

cmplx(x, 0.0_rp) without a KIND is default (single-precision) complex: c + vmad, dele, qpar and the energy pass through float32 before
the double arithmetic.  ``round_energy=False`` leaves the energy unrounded (the tests show the fixture tells the two apart).
"""
import numpy as np

from exchange_reference import simpson_f

PI = 3.14159265358979323846
AUX_SCALE = 1.0e3 / 4.0 / PI
JIJK_SCALE = (1.0e3 / 8.0 / PI) * (13.605693122994 / 1.8897261246)
COMPONENTS = ("xx", "xy", "xz", "yx", "yy", "yz", "zx", "zy", "zz")


def angles():
    """angles(4, 9) of exchange.f90:187-234: theta, theta', phi, phi' per component."""
    a = np.zeros((4, 9))
    h = 0.5 * PI
    table = [(h, h, 0, 0), (h, h, 0, h), (h, 0, 0, 0), (h, h, h, 0), (h, h, h, h), (h, 0, h, 0), (0, h, 0, 0), (0, h, 0, h), (0, 0, 0, 0)]
    for k, row in enumerate(table):
        a[:, k] = row
    return a


def weights():
    """Per component: (cos t cos t', sin t sin t' exp(i (phi' - phi)), sin t sin t' exp(i (phi - phi')))."""
    a = angles()
    cc = np.cos(a[0]) * np.cos(a[1]) * (1 + 0j)
    ss = np.sin(a[0]) * np.sin(a[1])
    return cc, ss * np.exp(1j * (a[3] - a[2])), ss * np.exp(1j * (a[2] - a[3]))


def _c32(x):
    """cmplx(x, 0.0_rp) without a KIND."""
    return np.float32(x).astype(np.float64) + 0j


def _diag18(v):
    """(..., l = 0..2, spin) -> (..., 18, 18) diagonal matrices, index l*l + m + 9 (s - 1)."""
    v = np.asarray(v)
    out = np.zeros(v.shape[:-2] + (18, 18), np.complex128)
    for s in range(2):
        for l in range(3):
            for m in range(2 * l + 1):
                k = l * l + m + 9 * s
                out[..., k, k] = v[..., l, s]
    return out


def p_matrix(cv, dele, ene, round_energy=True):
    """(nE, 18, 18): pmat = (cmplx(e) - cmplx(c + vmad)) / (cmplx(dele) cmplx(dele)).  cv, dele: (3, 2) per l and spin."""
    e = _c32(ene) if round_energy else np.asarray(ene, np.float64) + 0j
    t1, t2 = _c32(cv), _c32(dele)
    return _diag18((e[:, None, None] - t1[None]) / (t2 * t2)[None])


def _dvals(mat):
    return np.diagonal(mat, axis1=-2, axis2=-1)


def transform_pmatrix(pmat, q_in):
    """pmat_out = pmat_in / (1 + (cmplx(q_in) - cmplx(0)) pmat_in) on the diagonal."""
    t1 = _dvals(_diag18(_c32(q_in)))
    p = _dvals(pmat)
    out = np.zeros_like(pmat)
    idx = np.arange(18)
    out[..., idx, idx] = p / ((1 + 0j) + (t1 - (0 + 0j)) * p)
    return out


def auxiliary_gij(g, dele_i, dele_j):
    ci, cj = _diag18(_c32(dele_i)), _diag18(_c32(dele_j))
    return np.matmul(ci, np.matmul(g, cj))


def transform_auxiliary_gij(p_i, p0_i, p_j, p0_j, aux, q_in, same_atom):
    idx = np.arange(18)
    r1, r2, r3 = np.zeros_like(p_i), np.zeros_like(p_i), np.zeros_like(p_i)
    r1[..., idx, idx] = _dvals(p_i) / _dvals(p0_i)
    r2[..., idx, idx] = _dvals(p_j) / _dvals(p0_j)
    if same_atom:
        t1 = _dvals(_diag18(_c32(q_in)))
        r3[..., idx, idx] = ((0 + 0j) - t1) * (_dvals(p_i) / _dvals(p0_i))
    return np.matmul(r1, np.matmul(aux, r2)) + r3


def udisp_matrix(dmat9, pmat):
    """mat = matmul(dmat, pmat) + matmul(pmat, transpose(dmat)) with dmat the spin-diagonal 18 x 18 of the 9 x 9 block."""
    d = np.zeros((18, 18), np.complex128)
    d[:9, :9] = dmat9
    d[9:, 9:] = dmat9
    return np.matmul(d, pmat) + np.matmul(pmat, d.T)


def intersite(g0, same):
    """g0 (18, 18, nE, 4) -> gij, gji (nE, 18, 18) (green.f90:446-453)."""
    g = np.moveaxis(np.asarray(g0), 2, 0)
    if same:
        return g[..., 0], g[..., 0]
    d = g[..., 0] - g[..., 1]
    s = 1.0 / 1j * g[..., 2] - 1.0 / 1j * g[..., 3]
    return (d + s) * 0.5, (d - s) * 0.5


def _imtrace(m):
    return np.trace(m, axis1=-2, axis2=-1).imag


UU, DD = (slice(0, 9), slice(0, 9)), (slice(9, 18), slice(9, 18))


def _blk(m, b):
    return m[(Ellipsis,) + b]


def jij_aux_rows(g0, same, apar, ene, round_energy=True):
    """The 9 rows (9, nE) of one pair: jtot_aux(nv, 1:9), or jtot_00 in row 0 and zeros for an i == j pair.  apar: (2, 3, 2, 2)."""
    gij, gji = intersite(g0, same)
    p_i = p_matrix(apar[0, :, :, 0], apar[1, :, :, 0], ene, round_energy)
    p_j = p_matrix(apar[0, :, :, 1], apar[1, :, :, 1], ene, round_energy)
    aux_ij = auxiliary_gij(gij, apar[1, :, :, 0], apar[1, :, :, 1])
    aux_ji = auxiliary_gij(gji, apar[1, :, :, 1], apar[1, :, :, 0])
    dp_i, dp_j = _blk(p_i, UU) - _blk(p_i, DD), _blk(p_j, UU) - _blk(p_j, DD)
    rows = np.zeros((9, len(ene)))
    if not same:
        t1, t2 = np.matmul(dp_i, _blk(aux_ij, UU)), np.matmul(dp_j, _blk(aux_ji, DD))
        t3, t4 = np.matmul(dp_i, _blk(aux_ij, DD)), np.matmul(dp_j, _blk(aux_ji, UU))
        cc, w2, w3 = weights()
        for k in range(9):
            m = np.matmul(t1, t4) * cc[k] + np.matmul(t3, t4) * w2[k] + np.matmul(t1, t2) * w3[k] + np.matmul(t3, t2) * cc[k]
            rows[k] = _imtrace(m) * 0.5
    else:
        t1, t2 = np.matmul(dp_i, _blk(aux_ij, UU)), np.matmul(dp_j, _blk(aux_ji, DD))
        t3 = np.matmul(dp_i, _blk(aux_ij, UU) - _blk(aux_ji, DD))
        rows[0] = _imtrace(np.matmul(t1, t2) + t3) * (-1.0)
    return rows


def trio_greens(g0s, sames):
    """g0s: the trio's pairs (i,j), (i,k), (j,k), each (18, 18, nE, 4) -> dict of gij, gji, gik, gki, gjk, gkj."""
    G = {}
    for (a, b), g0, sm in zip((("i", "j"), ("i", "k"), ("j", "k")), g0s, sames):
        G[a + b], G[b + a] = intersite(g0, sm)
    return G


def jijk_rows(G, sames, apar, dmat, ene, round_energy=True):
    """The 9 rows (9, nE) of one trio: jijk_tot(nv, 1:9).  G: ``trio_greens``; sames: i == j, i == k, j == k; apar: (3, 3, 2, 3) =
    (c + vmad, dele, qpar) per l, spin and atom i, j, k; dmat: (9, 9), one spin block of disp_matrix of atom k."""
    at = {"i": 0, "j": 1, "k": 2}
    same = {"ij": sames[0], "ji": sames[0], "ik": sames[1], "ki": sames[1], "jk": sames[2], "kj": sames[2]}
    P = {a: p_matrix(apar[0, :, :, n], apar[1, :, :, n], ene, round_energy) for a, n in at.items()}
    P0 = {a: transform_pmatrix(P[a], apar[2, :, :, n]) for a, n in at.items()}
    u_k = udisp_matrix(dmat, P0["k"])
    X = {}
    for ab in ("ij", "ji", "ik", "ki", "jk", "kj"):
        a, b = ab
        aux = auxiliary_gij(G[ab], apar[1, :, :, at[a]], apar[1, :, :, at[b]])
        X[ab] = transform_auxiliary_gij(P[a], P0[a], P[b], P0[b], aux, apar[2, :, :, at[a]], same[ab])
    dp_i, dp_j = _blk(P0["i"], UU) - _blk(P0["i"], DD), _blk(P0["j"], UU) - _blk(P0["j"], DD)
    t1 = np.matmul(_blk(u_k, DD), _blk(X["ki"], DD))
    t2 = np.matmul(_blk(u_k, UU), _blk(X["ki"], UU))
    t3 = np.matmul(dp_i, _blk(X["ij"], UU))
    t4 = np.matmul(dp_j, _blk(X["jk"], UU))
    t5 = np.matmul(_blk(u_k, UU), _blk(X["kj"], UU))
    t6 = np.matmul(_blk(u_k, DD), _blk(X["kj"], DD))
    t7 = np.matmul(dp_j, _blk(X["ji"], UU))
    t8 = np.matmul(dp_i, _blk(X["ij"], DD))
    t9 = np.matmul(dp_j, _blk(X["jk"], DD))
    t10 = np.matmul(dp_j, _blk(X["ji"], DD))
    cc, w2, w3 = weights()
    mm = np.matmul
    rows = np.zeros((9, len(ene)))
    for p in range(9):
        m = (mm(t3, mm(t4, t2)) * cc[p] + mm(t8, mm(t4, t2)) * w2[p] + mm(t3, mm(t9, t1)) * w3[p] + mm(t8, mm(t9, t1)) * cc[p]
             + mm(t3, mm(t5, t10)) * w3[p] + mm(t8, mm(t6, t10)) * cc[p] + mm(t3, mm(t5, t7)) * cc[p] + mm(t8, mm(t6, t7)) * w2[p])
        rows[p] = _imtrace(m) * 0.5
    return rows


def jij_aux_pair(g0, same, apar, ene, fermi, nv1, round_energy=True):
    """One pair: (jaux (9) unscaled, rows (9, nE))."""
    rows = jij_aux_rows(g0, same, apar, np.asarray(ene, np.float64), round_energy)
    return simpson_f(rows, ene, fermi, nv1), rows


def jijk_trio(g0s, sames, apar, dmat, ene, fermi, nv1, round_energy=True):
    """One trio: (jijk (9) unscaled, rows (9, nE))."""
    rows = jijk_rows(trio_greens(g0s, sames), sames, apar, dmat, np.asarray(ene, np.float64), round_energy)
    return simpson_f(rows, ene, fermi, nv1), rows
