"""Writes tests/golden/cond_tensor_simpson.npz: the compiled reference's own math_mod::simpson_f (tools/cond_tensor_fixture/
simpson_driver.f90) with fermi = .true. on random series, for every limit EF = x(i) of small meshes.

    bash tools/cond_tensor_fixture/build.sh && python tools/cond_tensor_fixture/make_fixture.py

Shapes (nen, nv1): nv1 odd and even; nen = nv1 + 9, the shape energy%e_mesh makes, where the element the rule reads past the mesh is the
driver's zero padding; nen = nv1 + 12, where that element lies inside the mesh.  Three series per shape with magnitudes mixed over
1e-3 ... 1e3, at T = 0 and at one T whose kBT is about three mesh steps.  Every case is run twice and the runs must agree bit for bit.
Keys, per shape s = "<nen>_<nv1>": x_s (nen), y_s (3, nen), T_s, aint0_s and aintT_s (3, nen): [series, limit]."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DRIVER = os.path.join(ROOT, "oracle", "_ref", "simpson_driver.x")
SHAPES = [(12, 3), (31, 22), (32, 23), (35, 23)]
NSER = 3
KB = 0.633362019e-5


def run(x, y, nv1, T):
    out = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "simpson_in.bin"), "wb") as f:
                np.array([x.size, nv1, y.shape[0]], np.int32).tofile(f)
                np.array([T], np.float64).tofile(f)
                x.tofile(f)
                np.ascontiguousarray(y).tofile(f)
            r = subprocess.run([DRIVER], cwd=d, capture_output=True, text=True)
            assert r.returncode == 0, r.stdout + r.stderr
            out.append(np.fromfile(os.path.join(d, "simpson_out.bin"), np.float64).reshape(y.shape))
    assert np.array_equal(out[0], out[1]), "two runs of the reference differ"
    return out[0]


def main():
    rng = np.random.default_rng(20240611)
    z = {"shapes": np.array(SHAPES, np.int32)}
    for nen, nv1 in SHAPES:
        s = "%d_%d" % (nen, nv1)
        h = 1.7 / (nen + 1)
        x = -0.83 + h * np.arange(nen)                                  # a scaled axis inside (-1, 1)
        y = rng.standard_normal((NSER, nen)) * 10.0 ** rng.uniform(-3, 3, (NSER, nen))
        T = 3.0 * h / KB
        z["x_" + s], z["y_" + s], z["T_" + s] = x, y, T
        z["aint0_" + s], z["aintT_" + s] = run(x, y, nv1, 0.0), run(x, y, nv1, T)
    path = os.path.join(ROOT, "tests", "golden", "cond_tensor_simpson.npz")
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
