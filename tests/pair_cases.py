"""What the pair-call tests (tests/test_gpu_exchange.py, _damping.py, _aux.py, _contour.py) and their device scripts share: the energy
mesh, pair lists and seeded recursion of a case, the 1e-12 rule, g0 of the chains, the random inputs and restated checks of every call,
and the runner of a device script in its own process.  Not a test module."""
import os
import subprocess
import sys

import numpy as np

import aux_reference as R
from contour_reference import contour_pair, ordered_sum
from damping_reference import damping_rows, total_damping
from exchange_reference import PI, exchange_pair
from helpers import objects_from, supercell_problem
from rslmtoasa_amd.exchange import disp_matrix, exchange_dpar, trio_pairs
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.recursion import Recursion

TOL = 1e-12
FERMI = -0.05
EMIN, EMAX = -3.0, 1.8         # the recursion's energy window in ``setup`` (the Chebyshev scaling)
TRIOS = np.array([(1, 2, 9), (5, 60, 17), (1, 2, 1)], np.int32)          # the last repeats an atom: its pair (i,k) is an i == k pair


def mesh(channels_ldos, emin=-0.6, emax=0.4, fermi=-0.05):
    """energy%ene and nv1 as e_mesh builds them (energy.f90:184-207)."""
    if channels_ldos % 2 == 0:
        nv1 = channels_ldos + 1
    else:
        nv1, channels_ldos = channels_ldos, channels_ldos - 1
    edel = (emax - emin) / channels_ldos
    edel = (fermi - emin) / round((fermi - emin) / edel)
    ene = emin + edel * np.arange(channels_ldos + 10)
    return ene, nv1


def pair_list(kk, n, rng):
    """n pairs of a kk-atom cell, the first an i == j pair, the rest a mix of near and distant atoms."""
    pairs = [(1, 1)]
    for _ in range(n - 1):
        i = int(rng.integers(1, kk + 1))
        j = int(rng.integers(1, kk + 1))
        pairs.append((i, j))
    return np.array(pairs, np.int32)


def setup(pairs, lld=10, hoh=False, dims=(4, 4, 4), channels=300, kind="block", fermi=-0.05):
    p = supercell_problem(dims, hoh=hoh)
    ham, lat, ctl, en = objects_from(p, [1], lld, emin=EMIN, emax=EMAX)
    lat.ijpair = pairs
    rec = Recursion(ham, lat, ctl, en)
    if kind == "block":
        rec.recur_b_ij()
    else:
        rec.chebyshev_recur_ij()
    ene, nv1 = mesh(channels, fermi=fermi)
    g = Green(rec, ene)
    ntype = 1
    c = np.array([[[-0.02, 0.05], [0.31, 0.36], [-0.12, 0.01]]])[:ntype]
    dele = np.array([[[0.21, 0.20], [0.12, 0.11], [0.045, 0.052]]])[:ntype]
    dpar = exchange_dpar(c, dele, np.array([0.013]), p["iz"], pairs)
    return rec, g, ene, nv1, dpar


def onsite(kind, lld, sites=(1, 30, 64), hoh=False):
    p = supercell_problem((4, 4, 4), hoh=hoh)
    ham, lat, ctl, en = objects_from(p, list(sites), lld, emin=EMIN, emax=EMAX)
    rec = Recursion(ham, lat, ctl, en)
    if kind == "block":
        rec.recur_b()
    else:
        rec.chebyshev_recur()
    return rec


def close(mine, ref, floor, tol=TOL):
    """max deviation relative to the largest magnitude of the compared set, or to `floor` (the largest quantity of the same kind of
    the pair) where that is larger: quantities that vanish by symmetry are judged on the pair's scale."""
    mine, ref = np.asarray(mine), np.asarray(ref)
    scale = max(np.abs(ref).max(), floor, 1e-300)
    return np.abs(mine - ref).max() / scale <= tol


def chain_g0(rec, g, kind, n, zsqr=True):
    """g0 (18, 18, nE, n) of the first n chain slots from the library's Green kernels, which test_gpu_green pins to the reference
    (block: zsqr on the recursion's b2_b unless done already)."""
    if kind == "block":
        if zsqr:
            rec.zsqr()
        a_inf, b_inf, _, _ = g.terminator(nsites=n)
        return g.block_green(a_inf, b_inf, nsites=n).copy()
    return g.chebyshev_green(nsites=n).copy()


DEVICE_PRELUDE = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np, torch
torch.cuda.init(); torch.cuda.set_device(0)          # torch's HIP runtime before librsrec's (as bench.py does)
import pair_cases as T
mode = sys.argv[2]
"""


def run_device_script(script, mode, ok):
    """``DEVICE_PRELUDE + script`` in its own process, which has to print `ok`: torch's HIP runtime has to be initialised before
    librsrec's (the other tests of this session have started it)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", DEVICE_PRELUDE + script, root, mode], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and ok in r.stdout, (r.stdout + r.stderr)[-3000:]
    print(r.stdout)


# ---- rsrec_exchange

def exchange_restated(rec, g, ene, nv1, dpar, fermi, kind, pairs, cumulative=True, zsqr=True):
    """Restated outputs of every pair, from g0 of the library's Green kernels."""
    g0 = chain_g0(rec, g, kind, 4 * len(pairs), zsqr)
    out = [exchange_pair(g0[..., 4 * q:4 * q + 4], pairs[q, 0] == pairs[q, 1], dpar[..., q], ene, fermi, nv1, cumulative) for q in range(len(pairs))]
    return out, g0


def check_exchange(res, out, with_jcum=True):
    xc, so, fo, parts = res[:4]
    for q, (rxc, rso, rfo, rparts, rj, rrows) in enumerate(out):
        fv = max(np.abs(np.concatenate([rxc, rso, rfo, rparts])).max() * 1e-2, 1e-14)
        for grp in (slice(0, 1), slice(1, 4), slice(4, 13)):
            assert close(xc[grp, q], rxc[grp], fv) and close(so[grp, q], rso[grp], fv) and close(fo[grp, q], rfo[grp], fv), q
        for grp in (slice(0, 4), slice(4, 10), slice(10, 28)):
            assert close(parts[grp, q], rparts[grp], fv), q
        if with_jcum:
            assert close(res[4][:, q], rj, 0.0), q
        integ = res[-1]
        fr = np.abs(rrows).max() * 1e-2
        for r in range(41):
            assert close(integ[r, :, q], rrows[r], fr), (q, r)


# ---- rsrec_damping

def random_tmat(npairs, seed=21):
    """Random complex torque matrices per pair and side: nothing of the kernel may lean on the structure of a physical tmat."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal((18, 18, 3, 2, npairs)) + 1j * rng.standard_normal((18, 18, 3, 2, npairs)))


def damping_restated(g0, pairs, tmat):
    return [damping_rows(g0[..., 4 * q:4 * q + 4], pairs[q, 0] == pairs[q, 1], tmat[..., q]) for q in range(len(pairs))]


def ordered_total(rows):
    """total_damping from the device's own rows, the pairs added in ascending order."""
    t = np.zeros((9, rows.shape[1]))
    for q in range(rows.shape[2]):
        t = t + rows[:9, :, q]
    return t


def check_damping(res, ref, ief, col0=0):
    at_ef, total, rows = res
    assert rows.shape[2] == len(ref)
    for q, rr in enumerate(ref):
        floor = np.abs(rr).max()                      # a row that vanishes by symmetry is judged on the pair's largest row
        worst = max(np.abs(rows[r, :, q] - rr[r]).max() for r in range(18)) / max(floor, 1e-300)
        print("pair %d: largest row %.3e, worst deviation / floor %.2e" % (q, floor, worst))
        for r in range(18):
            assert close(rows[r, :, q], rr[r], floor), (q, r)
        assert close(at_ef[:, col0 + q], rr[:, ief - 1], floor), q
        assert np.array_equal(at_ef[:, col0 + q], rows[:, ief - 1, q]), q
    rt = total_damping(ref)
    assert close(total, rt, max(np.abs(rr[:9]).max() for rr in ref))
    assert np.array_equal(total, ordered_total(rows))
    assert np.abs(rows).max() > 0


# ---- rsrec_exchange_aux and rsrec_spin_lattice

def random_apar(n, nq, seed):
    """(c + vmad, dele[, qpar]) per l, spin and side / atom, random and different everywhere: a swap of sides, spins or atoms shows."""
    rng = np.random.default_rng(seed)
    out = np.zeros((nq, 3, 2, nq, n), order="F")
    out[0] = rng.uniform(-0.15, 0.4, out[0].shape)
    out[1] = rng.uniform(0.04, 0.22, out[1].shape)
    if nq == 3:
        out[2] = rng.uniform(0.01, 0.45, out[2].shape)
    return out


def random_trio_dmat(ntrios, seed=5):
    """disp_matrix of a random displacement per trio (a dense complex 9 x 9 with the reference's zero pattern), plus an imaginary part
    the reference's matrix does not have, so that the complex arithmetic is exercised."""
    rng = np.random.default_rng(seed)
    out = np.zeros((9, 9, ntrios), np.complex128, order="F")
    for t in range(ntrios):
        out[:, :, t] = disp_matrix(rng.normal(size=3), 2.6) * (1.0 + 0.3j)
    return out


def aux_reference(g0, pairs, apar, ene, nv1):
    return [R.jij_aux_pair(g0[..., 4 * q:4 * q + 4], pairs[q, 0] == pairs[q, 1], apar[..., q], ene, FERMI, nv1) for q in range(len(pairs))]


def jijk_reference(g0, trios, apar, dmat, ene, nv1):
    pairs = trio_pairs(trios)
    out = []
    for t in range(len(trios)):
        gs = [g0[..., 4 * q:4 * q + 4] for q in range(3 * t, 3 * t + 3)]
        sames = [bool(pairs[q, 0] == pairs[q, 1]) for q in range(3 * t, 3 * t + 3)]
        out.append(R.jijk_trio(gs, sames, apar[..., t], dmat[..., t], ene, FERMI, nv1))
    return out


def check_aux(res, ref):
    """Integrals and rows of every pair / trio, relative to its largest row (integrals: to its largest integral)."""
    val, rows = res
    for q, (rv, rr) in enumerate(ref):
        print(q, np.abs(val[:, q] - rv).max() / np.abs(rv).max(), np.abs(rows[:, :, q] - rr).max() / np.abs(rr).max())
        assert close(val[:, q], rv, 0.0), q
        assert close(rows[:, :, q], rr, 0.0), q
        assert np.abs(rr).max() > 1e-6


# ---- rsrec_exchange_contour

def random_contour_dmat(npairs, seed=33):
    """Random dense real matrices per pair and side: nothing of the kernel may lean on the structure of a physical dmat, and the two sides
    differ, so a swap of the sides changes the values."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal((9, 9, 2, npairs)))


def block_g_at_points(rec, e0, eta, nchains, a_inf, b_inf):
    """g (18, 18, npts, nchains) from one single-energy Green.block_green call per point: the loop the contour calls replace."""
    g1 = Green(rec, np.array([e0]))
    out = np.zeros((18, 18, len(eta), nchains), np.complex128)
    for k, et in enumerate(eta):
        out[:, :, k, :] = g1.block_green(a_inf, b_inf, eta=1j * et, nsites=nchains)[:, :, 0, :]
    return out


def check_contour_pairs(xc, rows, g, pairs, dmat, x, w, col0=0):
    for q in range(len(pairs)):
        rxc, rrows = contour_pair(g[..., 4 * q:4 * q + 4], pairs[q, 0] == pairs[q, 1], dmat[..., q], x, w)
        floor = np.abs(rrows).max()
        worst = np.abs(rows[:, :, q] - rrows).max() / max(floor, 1e-300)
        print("pair %d, %d points: largest row %.3e, worst row deviation / floor %.2e, xc deviation / scale %.2e"
              % (q, len(x), floor, worst, np.abs(xc[:, col0 + q] - rxc).max() / (floor * 1.0e3 / 4.0 / PI)))
        for r in range(13):
            assert close(rows[r, :, q], rrows[r], floor), (q, r)
        assert close(xc[:, col0 + q], rxc, floor * 1.0e3 / 4.0 / PI), q
        # the device's sum over the points is the ordered sum of its own rows, bit for bit
        sign = np.array([-1.0] + [1.0] * 3 + [-1.0] * 9)
        assert np.array_equal(xc[:, col0 + q], sign * ordered_sum(rows[:, :, q]) * 1.0e3 / 4.0 / PI), q
    assert np.abs(rows).max() > 0
