"""Writes tests/golden/eig18_roots.npz: the exact square roots of the prescribed-spectrum inputs of tests/eig18_cases.py.

    python tools/eig18_fixture/make_fixture.py            # write the fixture
    python tools/eig18_fixture/make_fixture.py --check    # recompute and compare every array with the committed file, bit for bit

For every input S (the ROUNDED double matrix, exactly Hermitian) mpmath's Hermitian eigen-solver at 50 digits gives V, lambda; the
root V sqrt(lambda) V^H is stored as a double-double pair root_hi + root_lo (106 bits: it squares back to S to about 1e-31, which
tests/test_eig18_cases.py checks in integer arithmetic).  Needs mpmath (1.3.0 was used); the tests do not.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eig18_cases as EC   # noqa: E402


def exact_root(S):
    import mpmath as mp
    mp.mp.dps = 50
    n = S.shape[0]
    A = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            A[i, j] = mp.mpc(float(S[i, j].real), float(S[i, j].imag))
    lam, V = mp.eighe(A)
    assert min(lam) > 0
    R = V * mp.diag([mp.sqrt(x) for x in lam]) * V.H
    hi = np.zeros((n, n), np.complex128)
    lo = np.zeros((n, n), np.complex128)
    for i in range(n):
        for j in range(n):
            z = (R[i, j] + mp.conj(R[j, i])) / 2
            parts = []
            for x in (mp.re(z), mp.im(z)):
                h = float(x)
                parts.append((h, float(x - mp.mpf(h))))
            hi[i, j] = complex(parts[0][0], parts[1][0])
            lo[i, j] = complex(parts[0][1], parts[1][1])
    return hi, lo


def compute():
    cases = EC.spectrum_cases()
    names = np.array([n for n, _ in cases])
    S = np.stack([s for _, s in cases], axis=2)
    roots = [exact_root(s) for _, s in cases]
    return dict(names=names, S=S, root_hi=np.stack([r[0] for r in roots], axis=2), root_lo=np.stack([r[1] for r in roots], axis=2))


def main():
    new = compute()
    if "--check" in sys.argv[1:]:
        with np.load(EC.GOLDEN, allow_pickle=False) as z:
            assert sorted(z.files) == sorted(new)
            assert [str(n) for n in z["names"]] == [str(n) for n in new["names"]]
            for k in ("S", "root_hi", "root_lo"):
                assert EC.same_bits(z[k], new[k]), k
        print("eig18_roots.npz reproduced bit for bit (%d matrices)" % len(new["names"]))
        return
    np.savez_compressed(EC.GOLDEN, **new)
    print("wrote %s: %d matrices, %d bytes" % (os.path.relpath(EC.GOLDEN, ROOT), len(new["names"]), os.path.getsize(EC.GOLDEN)))


if __name__ == "__main__":
    main()
