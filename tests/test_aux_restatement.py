"""The numpy restatement of calculate_jij_auxgreen and calculate_jijk (aux_reference.py) against the compiled reference's own members
(tests/golden/aux_jijk_block.npz, tools/aux_fixture), and the properties of the two routines the GPU kernels rely on."""
import numpy as np
import pytest

import aux_reference as R
from helpers import load_golden
from rslmtoasa_amd.exchange import aux_apar, disp_matrix, trio_apar, trio_pairs

# Measured deviations of the restatement from the fixture, relative to the largest of the nine components (both sides double precision
# on the same stored g0, differing in summation order only): jij_aux 5.6e-16, jij00_aux 9.5e-16, jijk 8.6e-15, jijk of the trio with a
# repeated atom 8.9e-15.  The bound is 10 x the largest of them, far below the project's parity bar of 1e-10.
BOUND = 8.9e-14
assert BOUND <= 1e-10


@pytest.fixture(scope="module")
def fx():
    z = dict(load_golden("aux_jijk_block"))
    iz = np.array([1, 2, 3])
    g = z["g0_trio"]
    same = np.zeros_like(g[..., 0:4])
    same[..., 0] = z["g0_same"]
    z["g_ne"], z["g_same"] = g[..., 0:4], same
    z["g_trio"] = [g[..., 0:4], g[..., 4:8], g[..., 8:12]]
    z["g_jkk"] = [g[..., 0:4], g[..., 0:4], same]                    # (1, 2634, 2634): (i,j) and (i,k) are the same pair, (j,k) is j == k
    z["apar_ne"] = aux_apar(z["c"], z["dele"], z["vmad"], iz, [(1, 2)])[..., 0]
    z["apar_same"] = aux_apar(z["c"], z["dele"], z["vmad"], iz, [(2, 2)])[..., 0]
    z["apar_trio"] = trio_apar(z["c"], z["dele"], z["vmad"], z["qpar"], iz, [(1, 2, 3)])[..., 0]
    z["apar_jkk"] = trio_apar(z["c"], z["dele"], z["vmad"], z["qpar"], iz, [(1, 2, 2)])[..., 0]
    z["args"] = (z["ene"], float(z["fermi"]), int(z["nv1"]))
    return z


def rel(mine, ref):
    return np.abs(np.asarray(mine) - ref).max() / np.abs(ref).max()


def test_restatement_gives_the_reference_members(fx):
    """Measured: jij_aux 5.6e-16, jij00_aux 9.5e-16, jijk 8.6e-15, jijk of the trio with a repeated atom 8.9e-15 (bound: 8.9e-14)."""
    d = {"jij_aux": rel(R.jij_aux_pair(fx["g_ne"], False, fx["apar_ne"], *fx["args"])[0], fx["jij_aux"]),
         "jij00_aux": rel(R.jij_aux_pair(fx["g_same"], True, fx["apar_same"], *fx["args"])[0][:1], fx["jij00_aux"]),
         "jijk": rel(R.jijk_trio(fx["g_trio"], [0, 0, 0], fx["apar_trio"], fx["dmat"], *fx["args"])[0], fx["jijk"]),
         "jijk_jkk": rel(R.jijk_trio(fx["g_jkk"], [0, 0, 1], fx["apar_jkk"], fx["dmat"], *fx["args"])[0], fx["jijk_jkk"])}
    print(d)
    assert max(d.values()) <= BOUND, d
    assert np.abs(fx["jij_aux"]).max() > 1e-3 and np.abs(fx["jijk"]).max() > 1e-3 and abs(fx["jij00_aux"]) > 1e-3


def test_energy_rounding_is_visible(fx):
    """p_matrix rounds the energy to single precision; a restatement that does not misses the fixture by far more than the bound."""
    miss = [rel(R.jij_aux_pair(fx["g_ne"], False, fx["apar_ne"], *fx["args"], round_energy=False)[0], fx["jij_aux"]),
            rel(R.jij_aux_pair(fx["g_same"], True, fx["apar_same"], *fx["args"], round_energy=False)[0][:1], fx["jij00_aux"]),
            rel(R.jijk_trio(fx["g_trio"], [0, 0, 0], fx["apar_trio"], fx["dmat"], *fx["args"], round_energy=False)[0], fx["jijk"])]
    print(miss)
    assert min(miss) > 1e3 * BOUND, miss


def test_angle_table_gives_xx_to_zz():
    """Component p = 3 a + b couples direction a of atom i to direction b of atom j: the unit vectors of (theta, phi) and (theta', phi')."""
    a = R.angles()
    unit = lambda t, p: np.array([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)])
    for p, name in enumerate(R.COMPONENTS):
        assert np.allclose(unit(a[0, p], a[2, p]), np.eye(3)["xyz".index(name[0])], atol=1e-15)
        assert np.allclose(unit(a[1, p], a[3, p]), np.eye(3)["xyz".index(name[1])], atol=1e-15)


def test_gik_is_never_read(fx):
    G = R.trio_greens(fx["g_trio"], [0, 0, 0])
    ene = np.asarray(fx["ene"])
    rows = R.jijk_rows(G, [0, 0, 0], fx["apar_trio"], fx["dmat"], ene)
    G["ik"] = np.full_like(G["ik"], np.nan)
    assert np.array_equal(R.jijk_rows(G, [0, 0, 0], fx["apar_trio"], fx["dmat"], ene), rows)
    G["ki"] = G["ki"] * 1.5
    assert not np.array_equal(R.jijk_rows(G, [0, 0, 0], fx["apar_trio"], fx["dmat"], ene), rows)


def test_trio_pair_order(fx):
    """(i,j), (i,k), (j,k) per trio (lattice.f90:644-651), and the fixture's trio of three distinct pairs tells every order apart."""
    assert trio_pairs([(1, 2, 9), (5, 60, 17)]).tolist() == [[1, 2], [1, 9], [2, 9], [5, 60], [5, 17], [60, 17]]
    g = fx["g_trio"]
    for order in ((0, 2, 1), (1, 0, 2), (2, 1, 0), (1, 2, 0), (2, 0, 1)):
        swapped = R.jijk_trio([g[q] for q in order], [0, 0, 0], fx["apar_trio"], fx["dmat"], *fx["args"])[0]
        assert rel(swapped, fx["jijk"]) > 1e3 * BOUND, order


def test_same_atom_additive_term(fx):
    """The trio (1, 2634, 2634): its pair (j,k) is a j == k pair, and transform_auxiliary_gij adds (0 - qpar) P / P0 on the diagonals of
    gjk and gkj.  The same Green functions without the term miss the fixture."""
    with_term = R.jijk_trio(fx["g_jkk"], [0, 0, 1], fx["apar_jkk"], fx["dmat"], *fx["args"])[0]
    assert rel(with_term, fx["jijk_jkk"]) <= BOUND
    # a j /= k pair whose chains give the same gjk = gkj = g(chain 1): twice chain 1, chains 2..4 zero ((2 g - 0) * 0.5 is exact)
    g = [np.array(x) for x in fx["g_jkk"]]
    g[2][..., 0] = 2.0 * g[2][..., 0]
    no_term = R.jijk_trio(g, [0, 0, 0], fx["apar_jkk"], fx["dmat"], *fx["args"])[0]
    assert rel(no_term, fx["jijk_jkk"]) > 1e3 * BOUND


def test_disp_matrix_matches_the_reference(fx):
    """The numpy disp_matrix against the reference's own (the fixture's dmat), to the rounding of the Gaunt quadrature."""
    assert np.abs(disp_matrix(fx["disp"], float(fx["wav"])) - fx["dmat"]).max() <= 1e-14 * np.abs(fx["dmat"]).max()
