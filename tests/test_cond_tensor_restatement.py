"""The numpy restatement of the conductivity tail's Simpson rule (tests/cond_tensor_reference.py) against the compiled reference's own
math_mod::simpson_f (tests/golden/cond_tensor_simpson.npz, written by tools/cond_tensor_fixture): every limit EF = x(i) of four small
meshes, at T = 0 and at a T whose kBT is about three mesh steps.

Bound, per element, from the inputs: the result is a recursive sum of n = 3 ((nv1 + 9) / 2) terms c_k y_k f_k times H / 3, so two
evaluations that differ only in rounding (the compiled reference may contract multiply-adds, numpy does not) lie within
n 2^-52 (H / 3) sum |c_k y_k f_k| of each other -- the standard bound of a recursive sum, the few roundings of the products and of
H A / 3 included in its slack.  At T > 0 the two exp implementations (each within 1-4 ulp, and the weight inherits that error
relatively) add 16 2^-52 times the same sum.  Where the element past the mesh is the driver's zero (nen = nv1 + 9) and where it lies
inside the mesh (nen = nv1 + 12) the same bound holds: the restatement takes terms above nen as zero, the mesh's own otherwise."""
import numpy as np
import pytest

import cond_tensor_reference as CT
from helpers import load_golden

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def golden():
    return load_golden("cond_tensor_simpson")


def test_fixture_covers_the_shapes(golden):
    shapes = [tuple(s) for s in golden["shapes"]]
    assert shapes == [(12, 3), (31, 22), (32, 23), (35, 23)]
    assert {nen - nv1 for nen, nv1 in shapes} == {9, 12} and {nv1 % 2 for _, nv1 in shapes} == {0, 1}


@pytest.mark.parametrize("hot", [False, True])
@pytest.mark.parametrize("nen,nv1", [(12, 3), (31, 22), (32, 23), (35, 23)])
def test_restatement_matches_compiled_simpson_f(nen, nv1, hot, golden):
    s = "%d_%d" % (nen, nv1)
    x, y, T = golden["x_" + s], golden["y_" + s], float(golden["T_" + s]) if hot else 0.0
    ref = golden[("aintT_" if hot else "aint0_") + s]
    assert x.size == nen and y.shape == (3, nen) and ref.shape == (3, nen) and np.isfinite(ref).all()
    if hot:
        assert 2.5 < CT.kbt(T) / (x[1] - x[0]) < 3.5
    got = CT.simpson_limits(x, nv1, y, T)
    scale = CT.simpson_abs(x, nv1, y, T)
    bound = (CT.n_terms(nv1) + (16 if hot else 0)) * EPS * scale
    err = np.abs(got - ref)
    print("simpson_f restatement", s, "T", T, "max err / bound", (err / np.maximum(bound, 1e-300)).max(), "max |ref|", np.abs(ref).max())
    assert np.abs(ref).max() > 0 and (scale > 0).all()
    assert (err <= bound).all()


def test_zero_temperature_weights_are_exact():
    """kBT = 1e-15 against mesh steps of 1e-3 and more: the weights come out as 1 below the limit, 0.5 at it, 0 above, so the rule at
    T = 0 is the plain Simpson sum with those weights."""
    x = -0.9 + 0.05 * np.arange(31)
    y = np.random.default_rng(3).standard_normal((2, 31))
    got = CT.simpson_limits(x, 22, y, 0.0)
    k = np.arange(31)
    for i in (0, 1, 7, 30):
        w = np.where(k < i, 1.0, np.where(k == i, 0.5, 0.0))
        A = np.zeros(2)
        for I in range(2, 32, 2):
            kk = I - 1
            A = ((A + y[:, kk - 1] * w[kk - 1]) + 4.0 * y[:, kk] * w[kk]) + (y[:, kk + 1] * w[kk + 1] if kk + 1 < 31 else 0.0)
        assert np.array_equal(got[:, i], (x[1] - x[0]) * A / 3.0)


def test_series_rows_and_order():
    rng = np.random.default_rng(11)
    integ = rng.standard_normal((18, 5, 3)) + 1j * rng.standard_normal((18, 5, 3))
    S = CT.series(integ, True)
    assert S.shape == (38, 5, 4)
    re = (integ[:, :, 0].real + integ[:, :, 1].real) + integ[:, :, 2].real
    assert np.array_equal(S[2:20, :, 0], re) and np.array_equal(S[20:38, :, 2], integ[:, :, 1].imag)
    tot = np.zeros(5)
    for l in range(18):
        tot = tot + re[l]
    assert np.array_equal(S[0, :, 0], tot)
    assert np.array_equal(CT.series(integ, False)[:, :, 0], S[:, :, 0]) and CT.series(integ, False).shape == (38, 5, 1)
