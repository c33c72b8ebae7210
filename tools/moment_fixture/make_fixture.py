"""Writes tests/golden/moment_integrals.npz: the compiled reference's own math_mod::simpson_f (fermi = .true., T = 0, every limit
EF = ene(i)) and math_mod::simpson_m (nexp = 0, 1, 2) on random series of small meshes (tools/moment_fixture/moment_driver.f90).

    bash tools/moment_fixture/build.sh && python tools/moment_fixture/make_fixture.py

Shapes (nen, nv1): nv1 = 1 and 2 at nen = nv1 + 9, the shape energy%e_mesh makes, where the element the rule reads past the mesh is the
driver's zero padding (both parities of that read); nen = nv1 + 12, where that element lies inside the mesh; two larger meshes.  Three
series per shape with magnitudes mixed over 1e-3 ... 1e3.  Fermi-level cases per shape: npts = 1, 2, 3 (the main loop of simpson_m
empty, empty, run once), a middle one and npts = nen - 2, each with e1 == fermi (no end term) and with fermi 0.37 steps above e1.
Every shape is run twice and the runs must agree bit for bit.
Keys, per shape s = "<nen>_<nv1>": ene_s (nen), edel_s, y_s (3, nen), cum_s (3, nen): [series, limit];
npts_s (ncase), e1_s (ncase), fermi_s (ncase), mom_s (ncase, 3, 3): [case, series, nexp]."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DRIVER = os.path.join(ROOT, "oracle", "_ref", "moment_driver.x")
SHAPES = [(10, 1), (11, 2), (14, 2), (31, 22), (35, 23)]
NSER = 3


def run(ene, edel, y, nv1, cases):
    out = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "moment_in.bin"), "wb") as f:
                np.array([ene.size, nv1, y.shape[0], len(cases)], np.int32).tofile(f)
                np.array([edel], np.float64).tofile(f)
                ene.tofile(f)
                np.ascontiguousarray(y).tofile(f)
                for npts, e1, fermi in cases:
                    np.array([npts], np.int32).tofile(f)
                    np.array([e1, fermi], np.float64).tofile(f)
            r = subprocess.run([DRIVER], cwd=d, capture_output=True, text=True)
            assert r.returncode == 0, r.stdout + r.stderr
            raw = np.fromfile(os.path.join(d, "moment_out.bin"), np.float64)
            ncum = y.size
            cum = raw[:ncum].reshape(y.shape)                                       # Fortran (nen, nser) = C [series][limit]
            mom = raw[ncum:].reshape(len(cases), y.shape[0], 3)                     # Fortran (3, nser, ncase) = C [case][series][nexp]
            out.append((cum, mom))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), "two runs of the reference differ"
    return out[0]


def main():
    rng = np.random.default_rng(20250214)
    z = {"shapes": np.array(SHAPES, np.int32)}
    for nen, nv1 in SHAPES:
        s = "%d_%d" % (nen, nv1)
        edel = 1.9 / (nen + 1)
        ene = -1.13 + edel * np.arange(nen)                                         # crosses zero: Ene**nexp changes sign for nexp = 1
        y = rng.standard_normal((NSER, nen)) * 10.0 ** rng.uniform(-3, 3, (NSER, nen))
        cases = []
        for npts in sorted({1, 2, 3, (nen - 2) // 2, nen - 2}):
            e1 = float(ene[npts - 1])
            cases += [(npts, e1, e1), (npts, e1, e1 + 0.37 * edel)]
        cum, mom = run(ene, edel, y, nv1, cases)
        z["ene_" + s], z["edel_" + s], z["y_" + s], z["cum_" + s] = ene, edel, y, cum
        z["npts_" + s] = np.array([c[0] for c in cases], np.int32)
        z["e1_" + s], z["fermi_" + s] = np.array([c[1] for c in cases]), np.array([c[2] for c in cases])
        z["mom_" + s] = mom
    path = os.path.join(ROOT, "tests", "golden", "moment_integrals.npz")
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
