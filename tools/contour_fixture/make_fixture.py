"""Writes tests/golden/contour_{block,cheb}.npz: the compiled reference's own Gauss-Legendre contour flow (tools/contour_fixture/
contour_driver.f90, run once per pair) on the reference's pair coefficients of the sc_4x4x8 pair fixtures (recur_b_ij /
chebyshev_recur_ij on the 4x4x8 bcc Fe cell, lld 12): green%calculate_intersite_gf_eta, exchange%calculate_exchange_gauss_legendre,
recursion%get_terminf and block_green_eta / chebyshev_green_eta with the pair's four chains taken as four sites.

    bash tools/contour_fixture/build.sh && python tools/contour_fixture/make_fixture.py

Each fixture holds x, w, ene, fermi, fermi_point, the coefficients of the i /= j pairs (block: a_b, b_sqrt after zsqr, a_inf, b_inf;
Chebyshev: mu_n), ee of the two atom types and dmat, and per pair the reference's gij_eta / gji_eta, its scaled jij, dmi, aij
(= T_comm_xc, full precision; gij_eta / gji_eta at the points ``eta_points`` only, to stay under the size limit of a committed file) and the diagonal of g of the four chains at the 64 points.  The i == j pair of the source fixture is left
out (the reference defines no result there).  Every pair is run twice and the two runs must agree bit for bit."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from helpers import load_golden  # noqa: E402
from rslmtoasa_amd.exchange import contour_dmat  # noqa: E402

DRIVER = os.path.join(ROOT, "oracle", "_ref", "contour_driver.x")
CHANNELS, FERMI, EMIN, EMAX = 100, -0.0517, -0.6, 0.4
LLD = 10                                  # the source chains have 12 levels; their first 10 are the lld = 10 recursion (moments: 2 lld + 2)
ETA_POINTS = np.arange(0, 64, 6)          # gij_eta / gji_eta are kept at these points (0-based) and the last: the file-size limit
ETA_POINTS = np.append(ETA_POINTS, 63)


def two_type_ee():
    """hamiltonian%ee(:,:,1,1:2): the on-site block of the bcc Fe fixture, and a second type with its spin blocks scaled apart."""
    e1 = np.asarray(load_golden("bccFe_nsp2_block")["ee"][:, :, 0, 0], np.complex128)
    e2 = e1.copy()
    e2[:9, :9] *= 1.06
    e2[9:, 9:] *= 0.95
    return np.asfortranarray(np.stack([e1, e2], axis=2)[:, :, None, :])


def run_pair(kind, lld, ee, coef, sym_term=0):
    out = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "input.nml"), "w").close()
            with open(os.path.join(d, "ct_in.bin"), "wb") as f:
                np.array([kind, lld, CHANNELS, sym_term], np.int32).tofile(f)
                np.array([FERMI, EMIN, EMAX], np.float64).tofile(f)
                np.asfortranarray(ee, dtype=np.complex128).ravel(order="F").tofile(f)
                np.asfortranarray(np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25]]).T).ravel(order="F").tofile(f)
                for a in coef:
                    np.asfortranarray(a, dtype=np.complex128).ravel(order="F").tofile(f)
            r = subprocess.run([DRIVER], cwd=d, capture_output=True, text=True)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            out.append(open(os.path.join(d, "ct_out.bin"), "rb").read())
    assert out[0] == out[1], "two runs of the reference differ"
    b, o = out[0], [0]

    def take(dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = np.frombuffer(b, dtype, int(np.prod(shape)), o[0]).reshape(shape, order="F").copy()
        o[0] += n
        return a
    z = dict(x=take(np.float64, (64,)), w=take(np.float64, (64,)))
    nen, fp = take(np.int32, (2,))
    z["fermi_point"] = int(fp)
    z["ene"] = take(np.float64, (int(nen),))
    z["gij_eta"], z["gji_eta"] = take(np.complex128, (64, 18, 18)), take(np.complex128, (64, 18, 18))
    z["xc"] = take(np.float64, (13,))
    if kind == 0:
        z["b_sqrt"] = take(np.complex128, (18, 18, lld, 4))
        z["a_inf"], z["b_inf"] = take(np.float64, (18, 18, 4)), take(np.float64, (18, 18, 4))
    z["gdiag"] = take(np.complex128, (18, 64, 4))
    assert o[0] == len(b)
    return z


def make(name, src, kind):
    g = load_golden(src)
    lld = LLD
    assert lld <= int(g["lld"])
    g = dict(g)
    if kind == 0:
        g["a_b"], g["b2_b"] = g["a_b"][:, :, :lld], g["b2_b"][:, :, :lld]
    else:
        g["mu_n"] = g["mu_n"][:, :, :2 * lld + 2]
    allpairs = np.asarray(g["pairs"], np.int32)
    keep = [p for p in range(len(allpairs)) if allpairs[p, 0] != allpairs[p, 1]]
    ee = two_type_ee()
    res = []
    for p in keep:
        sl = slice(4 * p, 4 * p + 4)
        coef = (g["a_b"][..., sl], g["b2_b"][..., sl]) if kind == 0 else (g["mu_n"][..., sl],)
        res.append(run_pair(kind, lld, ee, coef))
    z = dict(kind=kind, lld=lld, pairs=allpairs[keep], fermi=FERMI, emin=EMIN, emax=EMAX, channels_ldos=CHANNELS, ee=ee, source=src,
             dmat=contour_dmat(ee, [1, 2], np.array([(1, 2)] * len(keep))))
    for key in ("x", "w", "ene", "fermi_point"):
        assert all(np.array_equal(r[key], res[0][key]) for r in res)
        z[key] = res[0][key]
    for r in res:
        r["gij_eta"], r["gji_eta"] = r["gij_eta"][ETA_POINTS], r["gji_eta"][ETA_POINTS]
    z["eta_points"] = ETA_POINTS
    for key in ("gij_eta", "gji_eta", "xc", "gdiag") + (("a_inf", "b_inf") if kind == 0 else ()):
        z[key] = np.stack([r[key] for r in res], axis=-1)
    if kind == 0:
        z["a_b"] = np.concatenate([g["a_b"][..., 4 * p:4 * p + 4] for p in keep], axis=3)
        z["b_sqrt"] = np.concatenate([r["b_sqrt"] for r in res], axis=3)
        z["a_inf"] = z["a_inf"].reshape(18, 18, -1, order="F")
        z["b_inf"] = z["b_inf"].reshape(18, 18, -1, order="F")
    else:
        z["mu_n"] = np.concatenate([g["mu_n"][..., 4 * p:4 * p + 4] for p in keep], axis=3)
    path = os.path.join(ROOT, "tests", "golden", "contour_%s.npz" % name)
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes", "xc of pair 0:", z["xc"][:4, 0])


if __name__ == "__main__":
    make("block", "sc_4x4x8_block_ij", 0)
    make("cheb", "sc_4x4x8_cheb_ij", 1)
