"""Writes tests/golden/aux_jijk_block.npz: the compiled reference's own calculate_jij_auxgreen and calculate_jijk
(tools/aux_fixture/aux_driver.f90) on Green functions of the reference's own pair chains of a real trio.

    bash tools/exchange_case_fixture/build.sh && bash tools/aux_fixture/build.sh && python tools/aux_fixture/make_fixture.py

The chains come from the reference's recur_b_ij (+ zsqr) on the bcc Fe input of tests/golden/jijk_dropin/inputs/bccFe, whose namelist
sets njijk = 1 (the reference then derives the pairs (i,j), (i,k), (j,k) itself, lattice.f90:644-651), at lld 6: once for the trio
(1, 2634, 2635), three distinct i /= j pairs, and once for (1, 2634, 2634), whose pair (j,k) is an i == j pair
(tools/exchange_case_fixture/case_dump.f90 replays the program up to the pair recursion and dumps them).  g0 of every chain comes from
the C oracle (bgreen per chain, pinned to the reference elsewhere) on 12 energies and IS stored; the driver feeds it to the reference's
calculate_intersite_gf, pair by pair.  Four runs, each twice (the runs must agree bit for bit): the pair (1, 2634), the pair
(2634, 2634), and the two trios.  bcc Fe has one atom type, which would hide a swap of atoms; the driver therefore gives the three
atoms different potential parameters (c, dele, qpar per l and spin, vmad; more than 24 significant bits, so that the single-precision
rounding of the reference's cmplx() is visible).  It is the routines under test that read them, not the recursion.

Holds: trio, trio_jkk (atoms), lld, ene, fermi, nv1, g0_trio (18,18,12,12: the chains of the trio's three pairs), g0_same (18,18,12: the
one chain of (2634, 2634)), c, dele, qpar, vmad, wav, disp, dmat (9, 9) = one spin block of the reference's disp_matrix, and the members
jij_aux (9) of the pair (i,j), jij00_aux of (j,j), jijk (9), jijk_jkk (9) at full precision."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from exchange_reference import fixture_g0  # noqa: E402

DRIVER = os.path.join(ROOT, "oracle", "_ref", "aux_driver.x")
DUMP = os.path.join(ROOT, "oracle", "_ref", "exchange_case_dump.x")
INPUTS = os.path.join(ROOT, "tests", "golden", "jijk_dropin", "inputs", "bccFe")
LLD = 6
# potential parameters of the three atom types (l = 0..2, spin), bcc-Fe-like magnitudes
C_PAR = np.array([[[-0.0213, 0.0488], [0.3114, 0.3587], [-0.1209, 0.0103]], [[-0.0187, 0.0452], [0.3061, 0.3532], [-0.1154, 0.0146]],
                  [[-0.0241, 0.0517], [0.3175, 0.3621], [-0.1263, 0.0071]]])
DELE = np.array([[[0.2143, 0.2011], [0.1207, 0.1123], [0.0452, 0.0519]], [[0.2102, 0.1987], [0.1188, 0.1109], [0.0447, 0.0508]],
                 [[0.2171, 0.2034], [0.1219, 0.1137], [0.0461, 0.0527]]])
QPAR = np.array([[[0.4312, 0.4287], [0.0968, 0.0931], [0.0153, 0.0139]], [[0.4279, 0.4251], [0.0947, 0.0916], [0.0149, 0.0133]],
                 [[0.4338, 0.4302], [0.0981, 0.0944], [0.0158, 0.0142]]])
VMAD = np.array([0.0131, -0.0042, 0.0077])
WAV = 2.6391
DISP = np.array([1.0, 0.5, 0.25])


def mesh():
    """12 energies below and just above the Fermi level: nv1 = 3, so simpson_f runs I = 2 .. 12."""
    return -0.6 + 0.05 * np.arange(12), 3, -0.0517


def chains(trio):
    """The reference's pair chains of one trio: exchange_case_dump.x on a scratch copy of the input."""
    import importlib.util
    import shutil
    from oracle.make_fixtures import patch_namelist
    from rslmtoasa_amd._proc import run_with_unlimited_stack
    spec = importlib.util.spec_from_file_location("case_fixture", os.path.join(ROOT, "tools", "exchange_case_fixture", "make_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    scratch = tempfile.mkdtemp(prefix="rsrec_jijk_")
    try:
        for fn in os.listdir(INPUTS):
            shutil.copyfile(os.path.join(INPUTS, fn), os.path.join(scratch, fn))
        inp = os.path.join(scratch, "input.nml")
        txt = patch_namelist(open(inp).read(), {"control": {"lld": str(LLD)}, "energy": {"channels_ldos": "20"}})
        txt = txt.replace("ijktrio(1, :) = 1, 2634, 2635,", "ijktrio(1, :) = %d, %d, %d," % tuple(trio))
        assert "ijktrio(1, :) = %d, %d, %d," % tuple(trio) in txt
        open(inp, "w").write(txt)
        r = run_with_unlimited_stack([DUMP], cwd=scratch, env={"OMP_NUM_THREADS": "8"})
        assert r.returncode == 0 and os.path.exists(os.path.join(scratch, "case.bin")), r.stdout[-3000:] + r.stderr[-3000:]
        z = mod.read_case(os.path.join(scratch, "case.bin"))
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    i, j, k = trio
    assert z["pairs"].tolist() == [[i, j], [i, k], [j, k]] and z["lld"] == LLD and z["kind"] == "block", z["pairs"]
    z["same"] = (z["pairs"][:, 0] == z["pairs"][:, 1]).astype(np.int32)
    return z


def run(g0, pairs, ntrio, ene, fermi):
    out = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "aux_in.bin"), "wb") as f:
                np.array([len(ene) - 10, len(pairs), ntrio], np.int32).tofile(f)
                np.asfortranarray(pairs, dtype=np.int32).ravel(order="F").tofile(f)
                np.array([fermi, WAV] + list(DISP), np.float64).tofile(f)
                np.asarray(ene, np.float64).tofile(f)
                for a in (C_PAR, DELE, QPAR):
                    np.asfortranarray(a.transpose(1, 2, 0), dtype=np.float64).ravel(order="F").tofile(f)
                VMAD.tofile(f)
                np.asfortranarray(g0, dtype=np.complex128).ravel(order="F").tofile(f)
            r = subprocess.run([DRIVER], cwd=d, capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS="1"))
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            with open(os.path.join(d, "aux_out.bin"), "rb") as f:
                v = np.fromfile(f, np.float64, 19)
                dm = np.fromfile(f, np.complex128, 324).reshape(18, 18, order="F")
            out.append((v, dm))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), "two runs of the reference differ"
    return out[0]


def main():
    ene, nv1, fermi = mesh()
    trio, trio_jkk = (1, 2634, 2635), (1, 2634, 2634)
    za, zb = chains(trio), chains(trio_jkk)
    za["ene"] = zb["ene"] = ene
    g_trio = np.concatenate([fixture_g0(za, p) for p in range(3)], axis=3)
    gb = [fixture_g0(zb, p) for p in range(3)]
    # (1, 2634) is the pair (i,j) and the pair (i,k) of the second trio: the first run's chains serve for both (the two runs of the
    # threaded recursion agree to rounding, not bit for bit, so only one of them is stored)
    assert np.abs(gb[0] - g_trio[..., 0:4]).max() <= 1e-10 * np.abs(gb[0]).max() and not gb[2][..., 1:].any()
    gb[0] = gb[1] = g_trio[..., 0:4]
    v_ne, _ = run(g_trio[..., 0:4], [(1, 2)], 0, ene, fermi)
    v_eq, _ = run(gb[2], [(2, 2)], 0, ene, fermi)
    v_tr, dm = run(g_trio, [(1, 2), (1, 3), (2, 3)], 1, ene, fermi)
    v_jkk, dm2 = run(np.concatenate(gb, axis=3), [(1, 2), (1, 2), (2, 2)], 1, ene, fermi)
    assert np.array_equal(dm, dm2)
    assert np.array_equal(dm[:9, :9], dm[9:, 9:]) and not dm[:9, 9:].any() and not dm[9:, :9].any()
    z = dict(trio=np.array(trio), trio_jkk=np.array(trio_jkk), lld=LLD, ene=ene, fermi=fermi, nv1=nv1, g0_trio=g_trio, g0_same=gb[2][..., 0],
             c=C_PAR, dele=DELE, qpar=QPAR, vmad=VMAD, wav=WAV, disp=DISP, dmat=dm[:9, :9], jij_aux=v_ne[0:9], jij00_aux=v_eq[9], jijk=v_tr[10:19],
             jijk_jkk=v_jkk[10:19])
    path = os.path.join(ROOT, "tests", "golden", "aux_jijk_block.npz")
    np.savez(path, **z)
    print(path, os.path.getsize(path), "bytes")
    for k in ("jij_aux", "jij00_aux", "jijk", "jijk_jkk"):
        print(k, z[k])


if __name__ == "__main__":
    main()
