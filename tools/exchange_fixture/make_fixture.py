"""Writes tests/golden/exchange_{block,cheb,cheb_hoh}.npz: the compiled reference's own exchange flow (tools/exchange_fixture/
exchange_driver.f90, run once per pair) on the reference's pair coefficients of the sc_4x4x8 pair fixtures (recur_b_ij /
chebyshev_recur_ij, one i == j pair among them).  g0 of the chains comes from the C oracle (block_green_ij / chebyshev_green_ij:
bgreen / chebyshev_green per chain, pinned to the reference elsewhere); the driver feeds it to the reference's calculate_intersite_gf.

    bash tools/exchange_fixture/build.sh && python tools/exchange_fixture/make_fixture.py

Each fixture holds the coefficients (block: a_b and b2_b after zsqr; Chebyshev: mu_n), ene, fermi, nv1, dpar (rsrec_exchange's
layout), the atoms' potential parameters, and per pair the reference's full-precision members after calculate_exchange (xc) and
calculate_exchange_twoindex (fo, parts), its printed second-order row (jijso/dijso/aijso.out, 7 digits) and fort.150.  The driver gives
energy%ene two more points far above every Fermi level, so the element simpson_f reads past its arrays carries Fermi weight 0; every
pair is run twice and the two runs must agree bit for bit."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from helpers import load_golden  # noqa: E402
from exchange_reference import fixture_g0  # noqa: E402

DRIVER = os.path.join(ROOT, "oracle", "_ref", "exchange_driver.x")
# potential parameters of the two atom types (c, dele per l = 0..2 and spin; vmad), bcc-Fe-like magnitudes
C_PAR = np.array([[[-0.0213, 0.0488], [0.3114, 0.3587], [-0.1209, 0.0103]], [[-0.0187, 0.0452], [0.3061, 0.3532], [-0.1154, 0.0146]]])
DELE = np.array([[[0.2143, 0.2011], [0.1207, 0.1123], [0.0452, 0.0519]], [[0.2102, 0.1987], [0.1188, 0.1109], [0.0447, 0.0508]]])
VMAD = np.array([0.0131, -0.0042])


def mesh(channels_ldos=300, emin=-0.6, emax=0.4, fermi=-0.0517):
    """energy%ene, nv1 as e_mesh builds them (energy.f90:184-207)."""
    nv1 = channels_ldos + 1
    edel = (emax - emin) / channels_ldos
    edel = (fermi - emin) / round((fermi - emin) / edel)
    return emin + edel * np.arange(channels_ldos + 10), nv1, fermi


def run_pair(g0, same, ene, fermi, cr):
    out = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "xc_in.bin"), "wb") as f:
                np.array([len(ene) - 10, int(same)], np.int32).tofile(f)
                np.array([fermi], np.float64).tofile(f)
                np.asarray(ene, np.float64).tofile(f)
                for a in (C_PAR.transpose(1, 2, 0), DELE.transpose(1, 2, 0), VMAD, cr):
                    np.asfortranarray(a, dtype=np.float64).ravel(order="F").tofile(f)
                np.asfortranarray(g0, dtype=np.complex128).ravel(order="F").tofile(f)
            r = subprocess.run([DRIVER], cwd=d, capture_output=True, text=True)
            assert r.returncode == 0, r.stdout + r.stderr
            v = np.fromfile(os.path.join(d, "xc_out.bin"), np.float64)
            so = [np.loadtxt(os.path.join(d, n), ndmin=1)[5:-1] for n in ("jijso.out", "dijso.out", "aijso.out")]
            f150 = np.loadtxt(os.path.join(d, "fort.150"))
            out.append((v, np.concatenate(so), f150))
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1])), "two runs of the reference differ"
    v, so, f150 = out[0]
    xc = v[:13]
    fo = v[13:26]
    parts = v[26:54]
    return xc, fo, parts, so, f150


def make(name, src, kind):
    g = load_golden(src)
    ene, nv1, fermi = mesh()
    pairs = np.asarray(g["pairs"], np.int32)
    z = dict(kind=kind, lld=int(g["lld"]), emin=float(g["emin"]), emax=float(g["emax"]), pairs=pairs, ene=ene, nv1=nv1, fermi=fermi,
             c=C_PAR, dele=DELE, vmad=VMAD, source=src)
    if kind == "block":
        import oracle.oracle as o
        z["a_b"], z["b_sqrt"] = g["a_b"], o.zsqr(g["b2_b"])
    else:
        z["mu_n"] = g["mu_n"]
    np_ = len(pairs)
    dpar = np.zeros((4, 3, 2, np_), order="F")
    for side in range(2):                               # atom i is of type 1, atom j of type 2 (the driver's numbering)
        dpar[0, :, side] = (C_PAR[side, :, 0] + VMAD[side])[:, None]
        dpar[1, :, side] = (C_PAR[side, :, 1] + VMAD[side])[:, None]
        dpar[2, :, side] = DELE[side, :, 0][:, None]
        dpar[3, :, side] = DELE[side, :, 1][:, None]
    same = pairs[:, 0] == pairs[:, 1]
    for p in range(np_):
        if same[p]:                                     # calculate_intersite_gf reads chain 1 only, with atom i on both sides
            dpar[:, :, 1, p] = dpar[:, :, 0, p]
    z["dpar"], z["same"] = dpar, same.astype(np.int32)
    cr = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25]]).T
    res = [run_pair(fixture_g0(z, p), same[p], ene, fermi, cr) for p in range(np_)]
    for k, key in enumerate(("xc", "fo", "parts", "so_printed", "fort150")):
        z[key] = np.stack([r[k] for r in res], axis=-1)
    path = os.path.join(ROOT, "tests", "golden", "exchange_%s.npz" % name)
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    make("block", "sc_4x4x8_block_ij", "block")
    make("cheb", "sc_4x4x8_cheb_ij", "chebyshev")
    make("cheb_hoh", "sc_4x4x8_cheb_ij_hoh", "chebyshev")
