"""numpy restatement of the Gauss-Legendre contour stages as the reference writes them, for the tests of rsrec_exchange_contour and
rsrec_contour_occupation.

green%calculate_intersite_gf_eta (green.f90:471-536), then exchange%calculate_exchange_gauss_legendre (exchange.f90:1804-1865) with
dGdG_Jnc / _Dnc / _Anc (:933-1026) as 9 x 9 matrix products of the DENSE dmat and the Pauli parts, the factor applied to the matrices
before the trace as (m * w) / (x * x); and the occupations of bands%calculate_moments_gauss_legendre (bands.f90:559-586).  Input: g of the
chains at the contour points, z_k = e0 + i (1 - x_k) / x_k.

The one deviation, shared with the library: an i == j pair takes gij = gji = g(chain 1), as calculate_intersite_gf does (green.f90:446-448);
the reference's contour routine would combine chain 1 with slots recur_b_ij never writes.
"""
import numpy as np

from exchange_reference import PI, intersite_parts


def contour_eta(x):
    """eta_k = (1 - x_k) / x_k (green.f90:507-508): cmplx(0.0_rp, res) has no KIND, so the value is rounded to single precision."""
    x = np.asarray(x, np.float64)
    return ((1 - x) / x).astype(np.float32).astype(np.float64)


def pauli_parts(g, same):
    """g: (18, 18, npts, 4) of the pair's chains -> the 8 Pauli parts, each (npts, 9, 9) (green.f90:517-532)."""
    P = intersite_parts(g, same)
    return {k: P[k] for k in ("Ginmag", "Gix", "Giy", "Giz", "Gjnmag", "Gjx", "Gjy", "Gjz")}


def gij_gji(g, same):
    """(gij_eta, gji_eta), each (npts, 18, 18) (green.f90:517-521)."""
    g = np.moveaxis(np.asarray(g), 2, 0)
    if same:
        return g[..., 0], g[..., 0]
    d = g[..., 0] - g[..., 1]
    s = 1.0 / 1j * g[..., 2] - 1.0 / 1j * g[..., 3]
    return (d + s) * 0.5, (d - s) * 0.5


def contour_rows(g, same, dmat, x, w):
    """The 13 weighted values per point, (13, npts): jtot, jjtot(1:3), itot(3,3) with k fastest (exchange.f90:1824-1846)."""
    G = pauli_parts(g, same)
    di, dj = np.asarray(dmat[:, :, 0], np.complex128), np.asarray(dmat[:, :, 1], np.complex128)
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    gi = [G["Gix"], G["Giy"], G["Giz"]]
    gj = [G["Gjx"], G["Gjy"], G["Gjz"]]
    mm = np.matmul

    def weighted(m):
        return (m * w[:, None, None]) / (x * x)[:, None, None]

    def rtr(m):
        return np.trace(m, axis1=1, axis2=2).real

    def imtr(m):
        return np.trace(m, axis1=1, axis2=2).imag
    rows = np.zeros((13, len(x)))
    jm = mm(mm(di, G["Ginmag"]), mm(dj, G["Gjnmag"]))
    for k in range(3):
        jm = jm - mm(mm(di, gi[k]), mm(dj, gj[k]))
    rows[0] = rtr(weighted(jm))
    for k in range(3):
        dk = mm(mm(di, G["Ginmag"]), mm(dj, gj[k])) - mm(mm(dj, G["Gjnmag"]), mm(di, gi[k]))
        rows[1 + k] = imtr(weighted(dk))
    for k in range(3):
        for l in range(3):
            a = 0.5 * (mm(mm(di, gi[k]), mm(dj, gj[l])) + mm(mm(dj, gj[k]), mm(di, gi[l])))
            rows[4 + k + 3 * l] = rtr(weighted(a))
    return rows


def ordered_sum(y):
    """sum over the last axis in ascending order, as a Fortran loop adds (numpy's pairwise sum is another order)."""
    s = np.zeros(y.shape[:-1])
    for k in range(y.shape[-1]):
        s = s + y[..., k]
    return s


def xc_from_rows(rows):
    """T_comm_xc (13) of one pair from its rows (exchange.f90:1848-1865)."""
    s = ordered_sum(rows)
    sign = np.array([-1.0] + [1.0] * 3 + [-1.0] * 9)
    return sign * s * 1.0e3 / 4.0 / PI


def contour_pair(g, same, dmat, x, w):
    """(xc (13), rows (13, npts)) of one pair."""
    rows = contour_rows(g, same, dmat, x, w)
    return xc_from_rows(rows), rows


def occupation(gdiag, x, w):
    """occ (18, nsites) from the diagonal of g at the points, gdiag (18, npts, nsites) (bands.f90:572-585)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    y = (np.real(gdiag) * w[None, :, None]) / (x * x)[None, :, None]
    occ = np.zeros((18, gdiag.shape[2]))
    for k in range(len(x)):
        occ = occ + y[:, k, :] / PI
    return occ + 0.5


def jackson_kernel(nm):
    """math.f90:1641-1655, with mu_ng(:,:,2:) *= 2 folded in."""
    ll = np.arange(1, nm + 1, dtype=np.float64)
    th = PI * (ll - 1.0) / (nm + 1.0)
    k = ((nm - (ll - 1.0) + 1.0) * np.cos(th) + np.sin(th) / np.tan(PI / (nm + 1.0))) / (nm + 1.0)
    k[1:] *= 2.0
    return k


def chebyshev_green_eta(mu, e0, eta, energy_min, energy_max):
    """chebyshev_green_ij_eta (green.f90:960-1023) for every chain and point: mu (18, 18, nm, nchains), eta (npts) real ->
    g (18, 18, npts, nchains).  a uses the reference's default-REAL literals 2 and 0.3."""
    a = (energy_max - energy_min) / float(np.float32(2.0) - np.float32(0.3))
    b = (energy_max + energy_min) / 2
    nm = mu.shape[2]
    kern = jackson_kernel(nm)
    g = np.zeros((18, 18, len(eta), mu.shape[3]), np.complex128)
    for k, et in enumerate(eta):
        z = (e0 + 1j * et) - b
        th = np.arccos(z / a)
        for i in range(nm):
            g[:, :, k, :] += mu[:, :, i, :] * kern[i] * (-1j * np.exp(-1j * i * th))
        g[:, :, k, :] /= np.sqrt(a ** 2 - z ** 2)
    return g
