"""Host-side mirror of what the reference's ``bands`` type takes from the on-site Green function after the Fermi level is known
(bands.f90: calculate_magnetic_moments :791, calculate_orbital_moments :1075, calculate_moments :409, calculate_orbital_quadrupoles :870).

Every one of those routines reads ``g0(18,18,nE,site)`` through a handful of linear functionals ``Im Tr(O g0)``.  ``moment_operators``
names the operators; ``Green.block_spectra`` / ``Green.chebyshev_spectra`` evaluate the functionals on the device without forming g0;
the functions below turn that image ``spec(nop, nen, nsites)`` into the reference's energy-resolved arrays and integrals.  Plain numpy,
no GPU.

Orbital order of the 18 x 18 blocks: spin up 0..8 (s, p x3, d x5), spin down 9..17.
"""
from collections import OrderedDict

import numpy as np

ORBITALS = OrderedDict([("s", (0,)), ("p", (1, 2, 3)), ("d", (4, 5, 6, 7, 8))])
COMPONENTS = ("0", "x", "y", "z")
P_NAMES = tuple("P%s%s" % (c, l) for c in COMPONENTS for l in ORBITALS)
L_NAMES = ("Lx", "Ly", "Lz")
Q_NAMES = ("Qxx", "Qyy", "Qzz", "Qxy", "Qyz", "Qzx")
#: the operators an SCF iteration needs (12 P + 3 L), and all 21, in the order ``stack`` lays them out
SCF_OPERATORS = P_NAMES + L_NAMES
ALL_OPERATORS = SCF_OPERATORS + Q_NAMES


def _cartesian_l():
    """L_x, L_y, L_z on the nine real (cubic) harmonics s, p, d in the reference's order (math.f90:133-165), 9 x 9 complex."""
    r3 = np.sqrt(3.0)
    entries = {   # (row, column): value, 1-based as the reference indexes them; the whole table is multiplied by -i
        "x": {(4, 3): -1, (3, 4): 1, (7, 5): -1, (8, 6): -1, (9, 6): -r3, (5, 7): 1, (6, 8): 1, (6, 9): r3},
        "y": {(4, 2): 1, (2, 4): -1, (6, 5): 1, (5, 6): -1, (8, 7): -1, (9, 7): r3, (7, 8): 1, (7, 9): -r3},
        "z": {(3, 2): -1, (2, 3): 1, (8, 5): 2, (7, 6): 1, (6, 7): -1, (5, 8): -2},
    }
    out = {}
    for c, tab in entries.items():
        m = np.zeros((9, 9), np.complex128)
        for (i, j), v in tab.items():
            m[i - 1, j - 1] = v
        out[c] = m * (-1j)
    return out


def _cart2sph_matrix():
    """The unitary V of the reference's ``hcpx`` (math.f90:1508-1575): ``cart2sph`` is ``V^H M V``."""
    c = 1.0 / np.sqrt(2.0)
    tab = {(1, 1): 1, (2, 4): -c, (2, 2): c, (3, 4): 1j * c, (3, 2): 1j * c, (4, 3): 1, (5, 5): 1j * c, (5, 9): -1j * c, (6, 6): 1j * c,
           (6, 8): 1j * c, (7, 6): c, (7, 8): -c, (8, 5): c, (8, 9): c, (9, 7): 1}
    v = np.zeros((9, 9), np.complex128)
    for (i, j), x in tab.items():
        v[i - 1, j - 1] = x
    return v


def _spin_doubled(m9):
    m = np.zeros((18, 18), np.complex128)
    m[:9, :9] = m9
    m[9:, 9:] = m9
    return m


def moment_operators():
    """The named 18 x 18 complex operators, ``ops[name][row, column]``:

    ``P{0,x,y,z}{s,p,d}``: ``Im Tr(P g)`` is the bracket of bands.f90:449-452 with that spin component, summed over the orbitals of l:
    ``Im(g_oo + g_o+9,o+9)``, ``Im(g_o,o+9 + g_o+9,o)``, ``Im(i g_o,o+9 - i g_o+9,o)``, ``Im(g_oo - g_o+9,o+9)``.  Their sums over l are the
    brackets of calculate_projected_dos (:1175-1177).
    ``Lx, Ly, Lz``: the cartesian L matrices through ``cart2sph``, the same block in both spins (:1094-1111).
    ``Qab``: ``Lx^2, Ly^2, Lz^2`` and the symmetrised products (:949-955)."""
    ops = OrderedDict()
    for c in COMPONENTS:
        for l, orbs in ORBITALS.items():
            p = np.zeros((18, 18), np.complex128)
            for o in orbs:
                if c == "0":
                    p[o, o] = 1.0; p[o + 9, o + 9] = 1.0
                elif c == "z":
                    p[o, o] = 1.0; p[o + 9, o + 9] = -1.0
                elif c == "x":                     # Tr(P g) = sum P[j, i] g[i, j]: g[o, o+9] meets P[o+9, o]
                    p[o + 9, o] = 1.0; p[o, o + 9] = 1.0
                else:
                    p[o + 9, o] = 1j; p[o, o + 9] = -1j
            ops["P%s%s" % (c, l)] = p
    v = _cart2sph_matrix()
    lc = _cartesian_l()
    L = {c: _spin_doubled(v.conj().T @ (lc[c] @ v)) for c in "xyz"}
    for c in "xyz":
        ops["L" + c] = L[c]
    ops["Qxx"] = L["x"] @ L["x"]
    ops["Qyy"] = L["y"] @ L["y"]
    ops["Qzz"] = L["z"] @ L["z"]
    ops["Qxy"] = 0.5 * (L["x"] @ L["y"] + L["y"] @ L["x"])
    ops["Qyz"] = 0.5 * (L["y"] @ L["z"] + L["z"] @ L["y"])
    ops["Qzx"] = 0.5 * (L["z"] @ L["x"] + L["x"] @ L["z"])
    return ops


def stack(names=SCF_OPERATORS, ops=None):
    """The operators ``names`` as one (nop, 18, 18) array: the ``ops`` argument of ``Green.block_spectra`` / ``chebyshev_spectra``."""
    ops = moment_operators() if ops is None else ops
    return np.stack([ops[n] for n in names])


def traces(ops, g0):
    """``Im Tr(ops[k] g0[:, :, ie, s])`` in numpy: (nop, nen, nsites) from g0 (18, 18, nen, nsites)."""
    return np.einsum("kji,ijes->kes", np.asarray(ops), np.asarray(g0)).imag


def _row(spec, name, names):
    return np.asarray(spec)[names.index(name)]


def projected_dos(spec, names=SCF_OPERATORS):
    """dx, dy, dz (nen, nsites) of calculate_projected_dos (bands.f90:1168-1180) from the image of the ``P`` operators."""
    out = []
    for c in "xyz":
        b = sum(_row(spec, "P%s%s" % (c, l), names) for l in ORBITALS)
        out.append(-b / np.pi)
    return tuple(out)


def spin_resolved_dos(spec, mom, names=SCF_OPERATORS):
    """dspd (6, nen, nsites) of calculate_moments (bands.f90:437-470): rows l + 3 (isp - 1), l = s, p, d.  ``mom`` (3, nsites) are the
    unit vectors potential%mom of the sites."""
    spec, mom = np.asarray(spec), np.asarray(mom, dtype=np.float64).reshape(3, -1)
    nen, ns = spec.shape[1:]
    dspd = np.zeros((6, nen, ns))
    for isp in range(2):
        isgn = (-1.0) ** isp
        for il, l in enumerate(ORBITALS):
            b0, bx, by, bz = (_row(spec, "P%s%s" % (c, l), names) for c in COMPONENTS)
            dspd[il + 3 * isp] = -b0 - isgn * mom[2][None, :] * bz - isgn * mom[1][None, :] * by - isgn * mom[0][None, :] * bx
    return dspd * 0.5 / np.pi


def orbital_integrands(spec, names=SCF_OPERATORS):
    """lxi, lyi, lzi (nen, nsites) of calculate_orbital_moments (bands.f90:1123-1127); the moment is ``-simpson_m(...) / pi``."""
    return tuple(_row(spec, n, names) for n in L_NAMES)


def simpson_m(h, ef, npts, y, ea, nexp, ene):
    """The reference's Simpson rule for ``integral of E^nexp y(E)`` up to the Fermi level (math.f90:1579-1598): composite rule over the first
    ``npts`` mesh points (npts odd in the reference's use), plus the closing panel from ``ea`` to ``ef`` on points npts .. npts + 2."""
    y, ene = np.asarray(y, dtype=np.float64), np.asarray(ene, dtype=np.float64)
    f = y * ene ** nexp
    aint = 0.0
    for i in range(2, npts, 2):                    # Fortran I = 2, NPTS - 1, 2 (1-based)
        aint = aint + f[i - 2] + 4.0 * f[i - 1] + f[i]
    aint = h * aint / 3.0
    if ea != ef:
        aint = aint + (ef - ea) * (f[npts - 1] + 4.0 * f[npts] + f[npts + 1]) / 6.0
    return aint


def spin_moments(spec, h, ef, npts, ea, ene, names=SCF_OPERATORS):
    """mx, my, mz and mom1 (3, nsites) of calculate_magnetic_moments (bands.f90:807-832)."""
    d = projected_dos(spec, names)
    ns = d[0].shape[1]
    m0 = np.array([[simpson_m(h, ef, npts, d[c][:, s], ea, 0, ene) for s in range(ns)] for c in range(3)])
    m1 = np.array([[simpson_m(h, ef, npts, d[c][:, s], ea, 1, ene) for s in range(ns)] for c in range(3)])
    return m0, m1


def orbital_moments(spec, h, ef, npts, ea, ene, names=SCF_OPERATORS):
    """lmom (3, nsites) of calculate_orbital_moments (bands.f90:1129-1154)."""
    li = orbital_integrands(spec, names)
    ns = li[0].shape[1]
    return np.array([[-(simpson_m(h, ef, npts, li[c][:, s], ea, 0, ene) / np.pi) for s in range(ns)] for c in range(3)])


def band_moments(dspd, h, ef, npts, ea, ene, vmad=0.0):
    """occ (6, nsites), gravity_center (6, nsites) and the second moment ql(3) (6, nsites) of calculate_moments (bands.f90:486-495)."""
    ns = dspd.shape[2]
    occ, cg, q3 = np.zeros((6, ns)), np.zeros((6, ns)), np.zeros((6, ns))
    vm = np.broadcast_to(np.asarray(vmad, dtype=np.float64), (ns,))
    for s in range(ns):
        for i in range(6):
            sg, pm, sm = (simpson_m(h, ef, npts, dspd[i, :, s], ea, n, ene) for n in (0, 1, 2))
            occ[i, s] = sg
            cg[i, s] = (pm / sg) - vm[s]
            q3[i, s] = sm - 2.0 * (pm / sg) * pm + ((pm / sg) ** 2) * sg
    return occ, cg, q3


#: the series groups of ``series_table`` and the rows each adds
SERIES_GROUPS = OrderedDict([("spin", ("dx", "dy", "dz")), ("dspd", tuple("dspd%d" % i for i in range(1, 7))), ("orbital", L_NAMES),
                             ("quadrupole", Q_NAMES)])


def series_table(mom, names=SCF_OPERATORS, groups=("spin", "dspd", "orbital"), scaled=False):
    """The ``comb`` argument of ``Green.spectra_integrals``: (nop, nser, nsites), ``y(s, i, site) = sum_k comb[k, s, site] spec[k, i, site]``,
    and the names of its series.  ``mom`` (3, nsites): the unit vectors potential%mom of the sites.  Groups, in the order asked for:

    ``spin``: dx, dy, dz, the s + p + d sums of the x, y, z brackets (``projected_dos``);
    ``dspd``: the six rows l + 3 (isp - 1) of ``spin_resolved_dos`` with the site's moment direction;
    ``orbital``: the Lx, Ly, Lz rows (``orbital_integrands``);  ``quadrupole``: the six Q rows.

    The integrals are linear, so the reference's constant factors can be applied to a series or to its integrals.  ``scaled=False`` (what
    the Fortran drop-in passes) leaves them to the caller: -1/pi on ``spin``, 0.5/pi on ``dspd``.  ``scaled=True`` puts them into the table:
    ``comb . spec`` then equals ``projected_dos`` / ``spin_resolved_dos`` / ``orbital_integrands`` up to the rounding of the products."""
    mom = np.asarray(mom, dtype=np.float64).reshape(3, -1)
    ns = mom.shape[1]
    names = list(names)
    ser = [n for g in groups for n in SERIES_GROUPS[g]]
    comb = np.zeros((len(names), len(ser), ns), order="F")
    for g in groups:
        for n in SERIES_GROUPS[g]:
            s = ser.index(n)
            if g == "spin":
                for l in ORBITALS:
                    comb[names.index("P%s%s" % (n[1], l)), s, :] = -1.0 / np.pi if scaled else 1.0
            elif g == "dspd":
                i = int(n[4:]) - 1
                isgn, l = (-1.0) ** (i // 3), list(ORBITALS)[i % 3]
                f = 0.5 / np.pi if scaled else 1.0
                comb[names.index("P0" + l), s, :] = -f
                for c, m in zip("xyz", mom):
                    comb[names.index("P%s%s" % (c, l)), s, :] = -isgn * m * f
            else:
                comb[names.index(n), s, :] = 1.0
    return comb, ser
