"""numpy restatement of the exchange workflow as the reference writes it, for the tests of rsrec_exchange.

green%calculate_intersite_gf (green.f90:425-469) and _twoindex (:386-423), then the integrands of exchange%calculate_exchange
(exchange.f90:1437-1615, dGdG_Jnc / _Dnc / _Anc :933-1026) and calculate_exchange_twoindex (:1032-1435) as 9x9 matrix products of
d_matrix (symbolic_atom.f90:241-265) and the intersite parts, and simpson_f (math.f90:1600-1632) with fermi = .true., T = 0.  The one
deviation, shared with the library: the element simpson_f reads past the end of its arrays (Y(nv1 + 10)) is taken as zero.
"""
import numpy as np

PI = 3.14159265358979323846


def d_matrix(q, e):
    """d_matrix of one atom at energies e: (nE, 9, 9) complex.  q: (4, 3) = (c_up + vmad, c_dn + vmad, dele_up, dele_dn) per l."""
    e = np.asarray(e, np.float64)
    mat = np.zeros((len(e), 9, 9), np.complex128)
    for l in range(3):
        # cmplx(x, 0.0d0) without KIND is default (single-precision) complex: the parameters are rounded to float first
        cu, cd, wu, wd = (complex(float(np.float32(x))) for x in q[:, l])
        wuwd = wu * wd
        wu, wd = wu * wu, wd * wd
        de = (cd * wu - cu * wd + 1.0 * (wd - wu) * e) / wuwd
        for m in range(2 * l + 1):
            ml = l * l + m
            mat[:, ml, ml] = de
    return mat


def intersite_parts(g0, same):
    """g0: (18, 18, nE, 4) of the pair's chains -> dict of the 8 Pauli parts and 16 two-index parts, each (nE, 9, 9)."""
    g = np.moveaxis(np.asarray(g0), 2, 0)                                  # (nE, 18, 18, 4)
    if same:
        gij = gji = g[..., 0]
    else:
        d = g[..., 0] - g[..., 1]
        s = 1.0 / 1j * g[..., 2] - 1.0 / 1j * g[..., 3]
        gij, gji = (d + s) * 0.5, (d - s) * 0.5
    P = {}
    for nm, G in (("i", gij), ("j", gji)):
        P["G%snmag" % nm] = (G[:, :9, :9] + G[:, 9:, 9:]) * 0.5
        P["G%sz" % nm] = 0.5 * (G[:, :9, :9] - G[:, 9:, 9:])
        P["G%sy" % nm] = 0.5 * (1j * G[:, :9, 9:] - 1j * G[:, 9:, :9])
        P["G%sx" % nm] = 0.5 * (G[:, :9, 9:] + G[:, 9:, :9])
    nE = g.shape[0]
    names = ["G00ij", "G01ij", "G00ji", "G01ji"] + ["G%s%sij" % (c, b) for b in "10" for c in "xyz"] + ["G%s%sji" % (c, b) for b in "10" for c in "xyz"]
    Q = {n: np.zeros((nE, 9, 9), np.complex128) for n in names}
    for j in range(1, 10):
        for k in range(1, 10):
            l1, l2 = int((k - 0.9) ** 0.5), int((j - 0.9) ** 0.5)
            k0, j0 = l1 * (l1 + 1) + 1, l2 * (l2 + 1) + 1
            s = (-1) ** (k + j)
            a, b, rj, rk = k - 1, j - 1, 2 * j0 - j - 1, 2 * k0 - k - 1
            Q["G00ij"][:, a, b] += 0.5 * (P["Ginmag"][:, a, b] + s * P["Gjnmag"][:, rj, rk])
            Q["G01ij"][:, a, b] += 0.5 * (P["Ginmag"][:, a, b] - s * P["Gjnmag"][:, rj, rk])
            Q["G00ji"][:, a, b] += 0.5 * (P["Gjnmag"][:, a, b] + s * P["Ginmag"][:, rj, rk])
            Q["G01ji"][:, a, b] += 0.5 * (P["Gjnmag"][:, a, b] - s * P["Ginmag"][:, rj, rk])
            for c in "xyz":
                Q["G%s1ij" % c][:, a, b] += 0.5 * (P["Gi" + c][:, a, b] - s * P["Gj" + c][:, rj, rk])
                Q["G%s0ij" % c][:, a, b] += 0.5 * (P["Gi" + c][:, a, b] + s * P["Gj" + c][:, rj, rk])
                Q["G%s1ji" % c][:, a, b] += 0.5 * (P["Gj" + c][:, a, b] - s * P["Gi" + c][:, rj, rk])
                Q["G%s0ji" % c][:, a, b] += 0.5 * (P["Gj" + c][:, a, b] + s * P["Gi" + c][:, rj, rk])
    P.update(Q)
    return P


def _imtr(m):
    return np.trace(m, axis1=1, axis2=2).imag


def _rtr(m):
    return np.trace(m, axis1=1, axis2=2).real


def integrands(g0, same, dpar, ene):
    """The 41 integrand rows (41, nE) in the library's order (kernels_exchange.hpp)."""
    G = intersite_parts(g0, same)
    di, dj = d_matrix(dpar[:, :, 0], ene), d_matrix(dpar[:, :, 1], ene)

    def dGdG(a, b):
        return np.matmul(np.matmul(di, a), np.matmul(dj, b))

    xyz = "xyz"
    rows = np.zeros((41, len(ene)))
    J = dGdG(G["Ginmag"], G["Gjnmag"])
    for c in xyz:
        J = J - dGdG(G["Gi" + c], G["Gj" + c])
    rows[0] = _imtr(J)
    for k, c in enumerate(xyz):
        rows[1 + k] = _rtr(dGdG(G["Ginmag"], G["Gj" + c]) - np.matmul(np.matmul(dj, G["Gjnmag"]), np.matmul(di, G["Gi" + c])))
    for l, cl in enumerate(xyz):
        for k, ck in enumerate(xyz):
            t3 = dGdG(G["Gi" + ck], G["Gj" + cl])
            t4 = np.matmul(np.matmul(dj, G["Gj" + ck]), np.matmul(di, G["Gi" + cl]))
            rows[4 + k + 3 * l] = _imtr(0.5 * (t3 + t4))
    rows[13] = _imtr(dGdG(G["G00ij"], G["G00ji"]))
    rows[15] = _imtr(dGdG(G["G01ij"], G["G01ji"]))
    rows[14] = _imtr(sum(dGdG(G["G%s0ij" % c], G["G%s0ji" % c]) for c in xyz))
    rows[16] = _imtr(sum(dGdG(G["G%s1ij" % c], G["G%s1ji" % c]) for c in xyz))
    for k, c in enumerate(xyz):
        rows[20 + k] = _rtr(dGdG(G["G00ij"], G["G%s1ji" % c]))      # dsc
        rows[17 + k] = _rtr(dGdG(G["G01ij"], G["G%s0ji" % c]))      # dcc
    for l, cl in enumerate(xyz):
        for k, ck in enumerate(xyz):
            rows[23 + k + 3 * l] = _imtr(dGdG(G["G%s0ij" % ck], G["G%s0ji" % cl]))   # isd
            rows[32 + k + 3 * l] = _imtr(dGdG(G["G%s1ij" % ck], G["G%s1ji" % cl]))   # isc
    return rows


def fermifun(e, ef, kbt):
    with np.errstate(over="ignore"):
        return 1.0 / (np.exp((e - ef) / kbt) + 1.0)


def simpson_f(y, ene, ef, nv1):
    """simpson_f(fermi = .true., T = 0) of the rows of y (..., nE); Y and Ene past nE are zero."""
    y = np.asarray(y, np.float64)
    nE = y.shape[-1]
    pad = np.zeros(y.shape[:-1] + (2,))
    yy = np.concatenate([y, pad], axis=-1)
    f = np.concatenate([fermifun(np.asarray(ene, np.float64), ef, 0.633362019e-5 * 0.0 + 1.0e-15), np.zeros(2)])
    A = np.zeros(y.shape[:-1] + np.shape(ef)[:1])
    fe = f if np.ndim(ef) == 0 else None
    for I in range(2, nv1 + 10, 2):
        k = I - 1
        if fe is not None:
            A = A + yy[..., k - 1] * fe[k - 1] + 4.0 * yy[..., k] * fe[k] + yy[..., k + 1] * fe[k + 1]
        else:
            raise ValueError("scalar ef only")
    return (ene[1] - ene[0]) * A / 3.0


def combos(rows):
    """rows (41, nE) -> the 67 integrands of xc, so, fo, parts, with their scale factors (67,)."""
    jcd, jsd, jcc, jsc = rows[13], rows[14], rows[15], rows[16]
    dcc, dsc, isd, isc = rows[17:20], rows[20:23], rows[23:32], rows[32:41]
    y = np.concatenate([rows[0:13],
                        [jcd - jsd + jcc - jsc], 2 * (dsc + dcc), isd + isc,
                        [jcd + jsd - jcc - jsc], 2 * (dsc - dcc), -isd + isc,
                        rows[13:41]])
    scale = np.full(67, 1.0e3)
    scale[39 + 4:39 + 10] = 2.0e3
    return y, scale


def exchange_pair(g0, same, dpar, ene, fermi, nv1, cumulative=True):
    """One pair: (xc (13), so (13), fo (13), parts (28), jcum (nE) or None, rows (41, nE))."""
    ene = np.asarray(ene, np.float64)
    rows = integrands(g0, same, dpar, ene)
    y, scale = combos(rows)
    v = simpson_f(y, ene, fermi, nv1)
    v = v * scale / 4.0 / PI
    jcum = None
    if cumulative:
        jcum = np.array([simpson_f(y[13:14], ene, ef, nv1)[0] for ef in ene]) * 1.0e3 / 4.0 / PI
    return v[0:13], v[13:26], v[26:39], v[39:67], jcum, rows


def fixture_g0(z, p):
    """g0 (18,18,nE,4) of pair p of an exchange fixture from its coefficients, with the C oracle (bgreen / chebyshev_green per chain,
    terminators from get_terminf; eta = 0 as block_green_ij).  Chains an i == j pair does not read are left zero."""
    from oracle import oracle as o
    ene = np.asarray(z["ene"], np.float64)
    g0 = np.zeros((18, 18, len(ene), 4), np.complex128, order="F")
    nch = 1 if int(z["same"][p]) else 4
    for c in range(nch):
        s = 4 * p + c
        if str(z["kind"]) == "block":
            a, b = z["a_b"][:, :, :, s:s + 1], z["b_sqrt"][:, :, :, s:s + 1]
            ai, bi, _, _ = o.terminator(a, b)
            g0[:, :, :, c] = o.block_green(a[..., 0], b[..., 0], ene, ai[..., 0], bi[..., 0])
        else:
            g0[:, :, :, c] = o.chebyshev_green(z["mu_n"][:, :, :, s], ene, float(z["emin"]), float(z["emax"]))
    return g0
