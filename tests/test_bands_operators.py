"""The operator set of rslmtoasa_amd.bands (moment_operators): for the compiled reference's g0 (tests/golden/*_green.npz, every 40th
energy of its mesh) ``Im Tr(O g0)`` must reproduce the expressions the reference's routines evaluate on g0, written out here as the
index loops of bands.f90:449-452 (calculate_moments), :1175-1177 (calculate_projected_dos), :1124-1126 (calculate_orbital_moments) and
:986-992 (calculate_orbital_quadrupoles).

Bound: 1e-13 of the largest magnitude of the quantity over the energies and sites of the fixture -- both sides add the same at most
324 products, in a different order.  That bound cannot hold where the quantity is a difference of nearly equal terms or vanishes by
symmetry: P_z of non-magnetic fcc Cu (spin up minus spin down; measured here: error 2.7e-15 against a largest value of 5.1e-7, while the
terms are of order 10), d_x, d_y and Im Tr(L g0) of collinear runs without spin-orbit coupling (rounding noise on both sides).  The
error of a re-ordered sum is bounded by the size of its TERMS, (n - 1) eps sum|O_ji||g_ij| with n <= 324, i.e. 3.6e-14 of that sum;
every comparison below is therefore held to 1e-13 of  max(largest |quantity|, 1e-3 largest sum_ij |O_ji||g_ij|)  -- the first wherever the
quantity does not cancel (then it is the issue's bound), the second, three decades below the size of the terms, where it does.  No GPU."""
import os

import numpy as np
import pytest

from helpers import GOLD
from rslmtoasa_amd import bands

CASES = ["bccFe_nsp2_block", "bccFe_nsp4_block", "B2FeCo_block_hoh", "fccCu001_block_hoh"]
TOL = 1e-13
L_ORBS = {"s": [1], "p": [2, 3, 4], "d": [5, 6, 7, 8, 9]}            # o = (l - 1)**2 + m, 1-based (bands.f90:445-447)


def load_g0(name):
    with np.load(os.path.join(GOLD, name + "_green.npz"), allow_pickle=False) as z:
        return z["g0"]                                                # (18, 18, nen, nsites)


@pytest.fixture(scope="module")
def ops():
    return bands.moment_operators()


def terms(op, g0):
    """Largest sum_ij |O_ji| |g_ij| over energies and sites: the size of what Im Tr(O g0) adds up."""
    return np.einsum("ji,ijes->es", np.abs(op), np.abs(g0)).max()


def close(a, b, what, floor=0.0):
    """|a - b| <= 1e-13 max(largest |b|, 1e-3 floor), floor = terms(O, g0) (module docstring)."""
    scale = max(np.abs(b).max(), 1e-3 * floor)
    err = np.abs(a - b).max()
    print("%s: err %.3e scale %.3e" % (what, err, scale))
    assert err <= TOL * scale, (what, err, scale)


def reference_brackets(g0):
    """The four bracketed sums of bands.f90:449-452 per l: dict (component, l) -> (nen, nsites)."""
    nen, ns = g0.shape[2:]
    out = {(c, l): np.zeros((nen, ns)) for c in "0xyz" for l in L_ORBS}
    for na in range(ns):
        for l, orbs in L_ORBS.items():
            for o1 in orbs:
                o = o1 - 1
                for ie in range(nen):
                    g = g0[:, :, ie, na]
                    out["0", l][ie, na] += (g[o, o] + g[o + 9, o + 9]).imag
                    out["z", l][ie, na] += (g[o, o] - g[o + 9, o + 9]).imag
                    out["y", l][ie, na] += (1j * g[o, o + 9] - 1j * g[o + 9, o]).imag
                    out["x", l][ie, na] += (g[o, o + 9] + g[o + 9, o]).imag
    return out


def reference_projected_dos(g0):
    """bands.f90:1168-1180."""
    nen, ns = g0.shape[2:]
    dx, dy, dz = np.zeros((nen, ns)), np.zeros((nen, ns)), np.zeros((nen, ns))
    for na in range(ns):
        for ie in range(nen):
            g = g0[:, :, ie, na]
            for i in range(9):
                dz[ie, na] = dz[ie, na] - (g[i, i] - g[i + 9, i + 9]).imag / np.pi
                dy[ie, na] = dy[ie, na] - (1j * g[i, i + 9] - 1j * g[i + 9, i]).imag / np.pi
                dx[ie, na] = dx[ie, na] - (g[i, i + 9] + g[i + 9, i]).imag / np.pi
    return dx, dy, dz


def imtrace_matmul(op, g0):
    """imtrace(matmul(op, g0(:, :, ie, na))) for every energy and site (bands.f90:1124, :986)."""
    nen, ns = g0.shape[2:]
    out = np.zeros((nen, ns))
    for na in range(ns):
        for ie in range(nen):
            m = op @ g0[:, :, ie, na]
            out[ie, na] = sum(m[i, i].imag for i in range(18))
    return out


@pytest.mark.parametrize("name", CASES)
def test_operators_reproduce_reference_expressions(name, ops):
    g0 = load_g0(name)
    spec = bands.traces(bands.stack(bands.ALL_OPERATORS, ops), g0)
    assert spec.shape == (21,) + g0.shape[2:]
    row = {n: spec[i] for i, n in enumerate(bands.ALL_OPERATORS)}
    br = reference_brackets(g0)
    for (c, l), v in br.items():
        close(row["P%s%s" % (c, l)], v, "%s P%s%s" % (name, c, l), floor=terms(ops["P%s%s" % (c, l)], g0))
    # the brackets of calculate_projected_dos are the sums over l, and projected_dos applies its -1/pi
    dref = reference_projected_dos(g0)
    for c, got, ref in zip("xyz", bands.projected_dos(spec[:15]), dref):
        close(got, ref, "%s d%s" % (name, c), floor=terms(sum(ops["P%s%s" % (c, l)] for l in "spd"), g0) / np.pi)
    lref = [imtrace_matmul(ops[n], g0) for n in bands.L_NAMES]
    for n, got, ref in zip(bands.L_NAMES, bands.orbital_integrands(spec[:15]), lref):
        close(got, ref, "%s %s" % (name, n), floor=terms(ops[n], g0))
    for n in bands.Q_NAMES:
        close(row[n], imtrace_matmul(ops[n], g0), "%s %s" % (name, n), floor=terms(ops[n], g0))
    if name == "bccFe_nsp4_block":
        # the spin-off-diagonal and L paths carry signal in the non-collinear run with spin-orbit coupling: not a vacuous case
        scale = np.abs(dref[2]).max()
        assert max(np.abs(dref[0]).max(), np.abs(dref[1]).max()) > 1e-8 * scale or np.abs(lref[2]).max() > 1e-8 * scale


@pytest.mark.parametrize("name", ["bccFe_nsp4_block", "fccCu001_block_hoh"])
def test_spin_resolved_dos(name, ops):
    """dspd of bands.f90:437-470 written out with its loops, for moment directions that are not along z."""
    g0 = load_g0(name)
    nen, ns = g0.shape[2:]
    rng = np.random.default_rng(5)
    mom = rng.normal(size=(3, ns))
    mom /= np.linalg.norm(mom, axis=0)
    dspd = np.zeros((6, nen, ns))
    for na in range(ns):
        for isp in (1, 2):
            isgn = (-1.0) ** (isp - 1)
            soff = 3 * (isp - 1)
            for l in (1, 2, 3):
                for m in range(1, 2 * l):
                    o = (l - 1) ** 2 + m - 1
                    for ie in range(nen):
                        g = g0[:, :, ie, na]
                        dspd[l + soff - 1, ie, na] = dspd[l + soff - 1, ie, na] - (g[o, o] + g[o + 9, o + 9]).imag \
                            - isgn * mom[2, na] * (g[o, o] - g[o + 9, o + 9]).imag \
                            - isgn * mom[1, na] * (1j * g[o, o + 9] - 1j * g[o + 9, o]).imag \
                            - isgn * mom[0, na] * (g[o, o + 9] + g[o + 9, o]).imag
    dspd = dspd * 0.5 / np.pi
    got = bands.spin_resolved_dos(bands.traces(bands.stack(ops=ops), g0), mom)
    assert got.shape == dspd.shape
    close(got, dspd, name + " dspd")
    # the six rows add up to the site's density of states -Im Tr g0 / pi
    d = np.arange(18)
    close(got.sum(axis=0), -g0[d, d].imag.sum(axis=0) / np.pi, name + " sum dspd")


def test_angular_momentum_algebra(ops):
    """Lx, Ly, Lz are Hermitian, act alike in both spins, do not mix l, and satisfy [Lx, Ly] = i Lz (and cyclic) with L^2 = l (l + 1)
    on each l block."""
    L = [ops[n] for n in bands.L_NAMES]
    for m in L:
        assert np.abs(m - m.conj().T).max() <= 1e-15
        assert np.array_equal(m[:9, :9], m[9:, 9:]) and np.all(m[:9, 9:] == 0) and np.all(m[9:, :9] == 0)
    blocks = {0: slice(0, 1), 1: slice(1, 4), 2: slice(4, 9)}
    mask = np.zeros((9, 9), bool)
    for sl in blocks.values():
        mask[sl, sl] = True
    for m in L:
        assert np.all(m[:9, :9][~mask] == 0)
    for l, sl in blocks.items():
        lx, ly, lz = (m[sl, sl] for m in L)
        for a, b, c in ((lx, ly, lz), (ly, lz, lx), (lz, lx, ly)):
            assert np.abs(a @ b - b @ a - 1j * c).max() <= 4e-15
        l2 = lx @ lx + ly @ ly + lz @ lz
        assert np.abs(l2 - l * (l + 1) * np.eye(2 * l + 1)).max() <= 1e-14
        # Lz is diagonal in the spherical basis, with the eigenvalues m = -l .. l
        assert np.abs(lz - np.diag(np.diag(lz))).max() <= 1e-15 and np.abs(np.sort(np.diag(lz).real) - np.arange(-l, l + 1)).max() <= 1e-15
    q = {n: ops[n] for n in bands.Q_NAMES}
    assert np.abs(q["Qxy"] - 0.5 * (L[0] @ L[1] + L[1] @ L[0])).max() == 0 and np.abs(q["Qzz"] - L[2] @ L[2]).max() == 0


def test_simpson_m():
    """simpson_m (math.f90:1579-1598) against the rule written out: exact for cubics on the closed panels, and the closing panel of width
    (ef - ea) / 2 per interval added only where ea /= ef."""
    h, n = 0.01, 41
    ene = -0.3 + h * np.arange(n + 2)
    y = 1.0 + ene - 2.0 * ene ** 2
    ea = ene[n - 1]
    full = bands.simpson_m(h, ea, n, y, ea, 0, ene)
    F = lambda e: e + e ** 2 / 2 - 2 * e ** 3 / 3
    assert abs(full - (F(ea) - F(ene[0]))) <= 1e-14
    ef = ea + 0.6 * h
    tail = bands.simpson_m(h, ef, n, y, ea, 0, ene) - full
    assert abs(tail - (ef - ea) * (y[n - 1] + 4 * y[n] + y[n + 1]) / 6.0) <= 1e-16
    # nexp weights the integrand with E^nexp
    assert abs(bands.simpson_m(h, ea, n, y, ea, 1, ene) - bands.simpson_m(h, ea, n, y * ene, ea, 0, ene)) <= 1e-15
