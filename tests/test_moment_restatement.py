"""The numpy restatement of the moment integrals (tests/moment_reference.py) against the compiled reference's own math_mod::simpson_f
and math_mod::simpson_m (tests/golden/moment_integrals.npz, written by tools/moment_fixture), and its prefix form of the cumulative
integrals against its limit-by-limit form.

Bound against the compiled reference, per element, from the inputs -- the bound tests/test_cond_tensor_restatement.py uses: a result is a
recursive sum of n terms c_k y_k f_k times H / 3, so two evaluations that differ only in rounding (the compiled reference may contract
multiply-adds, numpy does not) lie within n 2^-52 (H / 3) sum |c_k y_k f_k| of each other.  For simpson_m the terms are
c_k y_k Ene_k**nexp, and the end term (EF - EA) / 6 (..) adds its three terms and its own scale.

The prefix form and the limit-by-limit form are the same sequence of operations on every element up to terms that add an exact zero
(tests/moment_reference.py): np.array_equal."""
import numpy as np
import pytest

import moment_reference as MR
from helpers import load_golden

EPS = 2.0 ** -52
SHAPES = [(10, 1), (11, 2), (14, 2), (31, 22), (35, 23)]


@pytest.fixture(scope="module")
def golden():
    return load_golden("moment_integrals")


def test_fixture_covers_the_shapes(golden):
    shapes = [tuple(s) for s in golden["shapes"]]
    assert shapes == SHAPES
    assert {nen - nv1 for nen, nv1 in shapes} == {9, 12} and {nv1 % 2 for nen, nv1 in shapes if nen == nv1 + 9} == {0, 1}
    for nen, nv1 in shapes:
        s = "%d_%d" % (nen, nv1)
        npts, e1, fermi = golden["npts_" + s], golden["e1_" + s], golden["fermi_" + s]
        assert {1, 2, 3, nen - 2} <= set(int(v) for v in npts)
        for v in set(int(v) for v in npts):
            assert sorted((e1 == fermi)[npts == v]) == [False, True]


@pytest.mark.parametrize("nen,nv1", SHAPES)
def test_cumulative_restatement_matches_compiled_simpson_f(nen, nv1, golden):
    s = "%d_%d" % (nen, nv1)
    ene, y, ref = golden["ene_" + s], golden["y_" + s], golden["cum_" + s]
    assert ene.size == nen and y.shape == (3, nen) and ref.shape == (3, nen) and np.isfinite(ref).all()
    got = MR.cum_limits(ene, nv1, y)
    bound = MR.n_terms_cum(nv1) * EPS * MR.cum_abs(ene, nv1, y)
    err = np.abs(got - ref)
    print("simpson_f restatement", s, "max err / bound", (err / np.maximum(bound, 1e-300)).max(), "max |ref|", np.abs(ref).max())
    assert np.abs(ref).max() > 0 and (bound > 0).all()
    assert (err <= bound).all()


@pytest.mark.parametrize("nen,nv1", SHAPES)
def test_fermi_level_restatement_matches_compiled_simpson_m(nen, nv1, golden):
    s = "%d_%d" % (nen, nv1)
    ene, edel, y, ref = golden["ene_" + s], float(golden["edel_" + s]), golden["y_" + s], golden["mom_" + s]
    npts, e1, fermi = golden["npts_" + s], golden["e1_" + s], golden["fermi_" + s]
    assert ref.shape == (npts.size, 3, 3) and np.isfinite(ref).all()
    worst = 0.0
    for c in range(npts.size):
        for p in range(3):
            args = (edel, float(fermi[c]), int(npts[c]), y, float(e1[c]), p, ene)
            got = MR.simpson_m(*args)
            bound = MR.n_terms_m(int(npts[c])) * EPS * MR.simpson_m_abs(*args)
            err = np.abs(got - ref[c, :, p])
            if int(npts[c]) < 3 and e1[c] == fermi[c]:
                assert np.array_equal(ref[c, :, p], np.zeros(3)) and np.array_equal(got, np.zeros(3))   # empty loop, no end term
                continue
            assert (bound > 0).all()
            worst = max(worst, (err / bound).max())
            assert (err <= bound).all(), (c, p, err, bound)
    print("simpson_m restatement", s, "max err / bound", worst)


def _meshes():
    rng = np.random.default_rng(5)
    for nen, nv1 in SHAPES + [(255, 246), (256, 247), (257, 248), (269, 257)]:
        ene = -0.9 + (1.7 / nen) * np.arange(nen)
        y = rng.standard_normal((4, nen)) * 10.0 ** rng.uniform(-3, 3, (4, nen))
        y[2, :nen // 3] = 0.0                                    # leading zeros
        y[3] = np.abs(y[3]) * np.where(np.arange(nen) < nen // 2, 1.0, -1.0)   # one sign change
        yield nen, nv1, ene, y


def test_prefix_form_equals_limit_by_limit_form():
    for nen, nv1, ene, y in _meshes():
        a, b = MR.cum_prefix(ene, nv1, y), MR.cum_limits(ene, nv1, y)
        assert np.array_equal(a, b), (nen, nv1, np.abs(a - b).max())
        assert np.abs(a).max() > 0


def test_existing_simpson_m_helper_agrees():
    """rslmtoasa_amd.bands.simpson_m forms y E**nexp first and then 4 (y E**nexp); a product with 4 is exact, so the bits are the same."""
    from rslmtoasa_amd import bands as B
    for nen, nv1, ene, y in list(_meshes())[:5]:
        for npts in (1, 2, 3, nen - 2):
            for ef in (ene[npts - 1], ene[npts - 1] + 0.01):
                for p in range(3):
                    got = MR.simpson_m(0.05, ef, npts, y, ene[npts - 1], p, ene)
                    ref = np.array([B.simpson_m(0.05, ef, npts, y[r], ene[npts - 1], p, ene) for r in range(y.shape[0])])
                    assert np.array_equal(got, ref)


def test_series_table_matches_the_band_helpers():
    from rslmtoasa_amd import bands as B
    rng = np.random.default_rng(9)
    spec = rng.standard_normal((15, 12, 3))
    mom = rng.standard_normal((3, 3))
    mom /= np.linalg.norm(mom, axis=0)
    comb, names = B.series_table(mom, scaled=True)
    assert comb.shape == (15, 12, 3) and names[:3] == ["dx", "dy", "dz"] and names[9:] == list(B.L_NAMES)
    y = MR.series(spec, comb)
    ref = np.concatenate([np.stack(B.projected_dos(spec)), B.spin_resolved_dos(spec, mom), np.stack(B.orbital_integrands(spec))])
    assert np.abs(y - ref).max() <= 8 * EPS * np.abs(spec).max()          # at most four products of magnitude below |spec| and their sum
    assert np.array_equal(y[9:], spec[12:15])
    raw, _ = B.series_table(mom, scaled=False)
    assert np.allclose(raw[:, :3] * (-1.0 / np.pi), comb[:, :3], rtol=1e-15, atol=0) and np.allclose(raw[:, 3:9] * (0.5 / np.pi), comb[:, 3:9], rtol=1e-15, atol=0)
    q, qn = B.series_table(mom, names=B.ALL_OPERATORS, groups=("quadrupole",))
    assert qn == list(B.Q_NAMES) and np.array_equal(q[15:, :, 0], np.eye(6)) and not q[:15].any()
