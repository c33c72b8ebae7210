"""Parity of the HIP path (through the C ABI) with the CPU oracle and with the reference's golden vectors.

Bar (BASELINE.json north_star): recursion coefficients / moments within 1e-10 relative of the reference.
All arithmetic is FP64; differences come only from summation order (MFMA / tree reductions vs BLAS).
"""
import os

import numpy as np
import pytest

from helpers import (assert_within_reference_spread, BLOCK_CASES, CHEB_CASES, GOLD, PAIR_CASES, RTOL, SCALAR_CASES, load_golden, load_golden_with_inputs, objects_from,
                     problem_dict, rel_err, rel_err_rows, supercell_problem)
from rslmtoasa_amd.lattice import spread_sites
from rslmtoasa_amd.recursion import Recursion

pytestmark = pytest.mark.gpu

KERNELS = [1, 2]   # 1 = VALU reference kernels, 2 = MFMA kernels (both are HIP; both must meet the bar)
# "ci": matrix-core kernels with the large-launch SpMM (k_spmm5, CI vector layout) forced on the small fixtures too
BLOCK_VARIANTS = [1, 2, "ci"]


def select_kernels(rec, variant):
    if variant == "ci":
        rec.set_option("kernels", 2)
        rec.set_option("spmm5", 2)
    else:
        rec.set_option("kernels", variant)
        rec.set_option("spmm5", 1)          # by launch size: these small fixtures then run the cooperative k_spmm4<4> on LayoutRM (the default is k_spmm5 always)


def make(p, irec, lld, **kw):
    ham, lat, ctl, en = objects_from(p, irec, lld, **kw)
    return Recursion(ham, lat, ctl, en, device=0)


@pytest.mark.parametrize("kernels", BLOCK_VARIANTS)
@pytest.mark.parametrize("name", BLOCK_CASES)
def test_block_lanczos_golden(name, kernels, oracle_lib):
    g = load_golden(name)
    rec = make(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"])
    select_kernels(rec, kernels)
    rec.recur_b()
    n = g["nrec"]
    assert rel_err(rec.a_b[:, :, :, :n], g["a_b"]) < RTOL
    assert rel_err(rec.b2_b[:, :, :, :n], g["b2_b"]) < RTOL
    assert np.all(rec.a_b[:, :, -1] == 0)                               # recursion.f90:1836
    assert np.array_equal(rec.b2_b[:, :, 0, 0], np.eye(18))             # :1837
    d = np.arange(18)
    assert np.array_equal(rec.a[: g["lld"], :, 0, 0], rec.a_b[d, d, :, 0].real.T)   # :1850
    if kernels == 2:
        # against the oracle on the same inputs (once per fixture: the oracle itself is pinned by tests/test_oracle_golden.py)
        o = oracle_lib.Oracle(problem_dict(g))
        a_o, b_o = o.block_lanczos(g["irec"], g["lld"])
        assert rel_err(rec.a_b[:, :, :, :n], a_o) < RTOL and rel_err(rec.b2_b[:, :, :, :n], b_o) < RTOL
    rec.close()


@pytest.mark.parametrize("kernels", BLOCK_VARIANTS)
@pytest.mark.parametrize("name", CHEB_CASES)
def test_chebyshev_golden(name, kernels):
    g = load_golden(name)
    rec = make(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"], emin=g["emin"], emax=g["emax"])
    select_kernels(rec, kernels)
    rec.chebyshev_recur()
    assert rel_err(rec.mu_n[:, :, :, : g["nrec"]], g["mu_n"]) < RTOL
    rec.close()


@pytest.mark.parametrize("name", CHEB_CASES)
def test_chebyshev_golden_unfused(name):
    """k_spmm5 on CI vectors with cheb_fused = 0: the SpMM leaves plain H psi and k_mfma_cheb forms the new vector."""
    g = load_golden(name)
    rec = make(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"], emin=g["emin"], emax=g["emax"])
    rec.set_option("kernels", 2)
    rec.set_option("spmm5", 2)
    rec.set_option("cheb_fused", 0)
    rec.chebyshev_recur()
    assert rel_err(rec.mu_n[:, :, :, : g["nrec"]], g["mu_n"]) < RTOL
    rec.close()


@pytest.mark.parametrize("name", SCALAR_CASES)
def test_scalar_lanczos_golden(name):
    g = load_golden(name)
    rec = make(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"], llsp=g["a"].shape[0])
    rec.recur()
    assert rel_err_rows(rec.a[:, :, :, 0], g["a"]) < RTOL
    assert rel_err_rows(rec.b2[:, :, :, 0], g["b2"]) < RTOL
    rec.close()


@pytest.mark.parametrize("kernels", BLOCK_VARIANTS)
def test_chebyshev_surface_full_depth(kernels):
    """SURVEY C4 at its real depth: fccCu(001), three atom types, two sites, lld = 50 (102 moments) against the compiled reference."""
    g = load_golden_with_inputs("fccCu001_cheb50")
    rec = make(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"], emin=g["emin"], emax=g["emax"])
    select_kernels(rec, kernels)
    rec.chebyshev_recur()
    assert rel_err(rec.mu_n[:, :, :, : g["nrec"]], g["mu_n"]) < RTOL
    rec.close()


def test_scalar_noop_unless_nsp1():
    g = load_golden("bccFe_nsp2_block")
    rec = make(problem_dict(g), g["irec"], 6, nsp=2)
    rec.recur()
    b2 = rec.b2[:, :, 0, 0]
    assert np.all(rec.a == 0) and np.all(b2[0] == 1) and np.all(b2[1:3] == 0) and np.all(np.isnan(b2[3:6]))
    rec.close()


@pytest.mark.parametrize("kernels", KERNELS)
@pytest.mark.parametrize("name", ["sc_4x4x8_block", "sc_4x4x8_block_hoh"])
def test_config0_supercell_block(name, kernels):
    """BASELINE.json configs[0]: 128-atom periodic supercell, LL=30, vs the compiled reference routines."""
    g = load_golden(name)
    rec = make(supercell_problem(g["dims"], hoh=bool(g["hoh"])), g["irec"], int(g["lld"]))
    rec.set_option("kernels", kernels)
    rec.recur_b()
    n = len(g["irec"])
    # per level: 1e-10 wherever the reference agrees with itself, else 8x the reference's own thread-count spread (helpers.spread_tolerance)
    assert_within_reference_spread(name, "a_b", rec.a_b[:, :, :, :n], g["a_b"])
    assert_within_reference_spread(name, "b2_b", rec.b2_b[:, :, :, :n], g["b2_b"])
    rec.close()


def test_config0_supercell_chebyshev():
    g = load_golden("sc_4x4x8_cheb")
    rec = make(supercell_problem(g["dims"]), g["irec"], int(g["lld"]), emin=float(g["emin"]), emax=float(g["emax"]))
    rec.chebyshev_recur()
    assert rel_err(rec.mu_n[:, :, :, :1], g["mu_n"]) < RTOL
    rec.close()


@pytest.mark.parametrize("kernels", KERNELS)
def test_config1_full_size_vs_reference(kernels):
    """BASELINE.json configs[1]: 22^3 = 10 648 atoms, LL=50, one site, against the compiled reference's output."""
    g = load_golden("sc_22_block")
    p = supercell_problem(g["dims"])
    sites = np.concatenate([g["irec"], spread_sites(p["nn"].shape[0], 4)[1:]])
    rec = make(p, sites, int(g["lld"]))
    rec.set_option("kernels", kernels)
    rec.recur_b()
    assert rel_err(rec.a_b[:, :, :, :1], g["a_b"]) < RTOL
    assert rel_err(rec.b2_b[:, :, :, :1], g["b2_b"]) < RTOL
    # size-independent properties on the full-size run ------------------------------------------------
    a_b, b2_b = rec.a_b, rec.b2_b
    # (1) translation invariance of the periodic lattice: every site gives the same coefficients
    for s in range(1, len(sites)):
        assert rel_err(a_b[:, :, :, s], a_b[:, :, :, 0]) < RTOL
        assert rel_err(b2_b[:, :, :, s], b2_b[:, :, :, 0]) < RTOL
    # (2) A_n and B_n^2 are Hermitian, B_n^2 positive definite
    for ll in range(int(g["lld"])):
        A, S = a_b[:, :, ll, 0], b2_b[:, :, ll, 0]
        assert np.abs(A - A.conj().T).max() < 1e-12
        assert np.abs(S - S.conj().T).max() < 1e-12
        assert np.linalg.eigvalsh(S).min() > 0
    # (3) zsqr: (sqrt(B^2))^2 == B^2, Hermitian
    b2_before = b2_b.copy()
    rec.zsqr()
    for ll in range(int(g["lld"])):
        m = rec.b2_b[:, :, ll, 0]
        assert np.abs(m @ m - b2_before[:, :, ll, 0]).max() < 1e-13
        assert np.abs(m - m.conj().T).max() < 1e-13
    rec.close()


def test_config2_size_1e5_atoms():
    """BASELINE.json configs[2] size: 46^3 = 97 336 atoms, LL=50, the sites one GPU of eight would own in a small run.
    No reference output exists at this size (the reference's O(kk^2) cluster builder does not get there), so the check is by
    properties that do not depend on the size: (1) until a chain can feel the periodic images (level < 11 in the 22^3 cell: a
    coefficient of level n sums closed paths of at most 2n+1 hops) the 46^3 coefficients equal the compiled reference's
    22^3 ones; (2) translation invariance; (3) Hermitian A_n, Hermitian positive definite B_n^2 at every level."""
    g = load_golden("sc_22_block")
    p = supercell_problem((46, 46, 46))
    kk = p["nn"].shape[0]
    assert kk == 97336
    sites = spread_sites(kk, 4)
    rec = make(p, sites, int(g["lld"]))
    rec.recur_b()
    a_b, b2_b = rec.a_b, rec.b2_b
    assert rel_err(a_b[:, :, :10, 0], g["a_b"][:, :, :10, 0]) < RTOL
    assert rel_err(b2_b[:, :, :10, 0], g["b2_b"][:, :, :10, 0]) < RTOL
    for s in range(1, len(sites)):
        assert rel_err(a_b[:, :, :, s], a_b[:, :, :, 0]) < RTOL
        assert rel_err(b2_b[:, :, :, s], b2_b[:, :, :, 0]) < RTOL
    for ll in range(int(g["lld"])):
        A, S = a_b[:, :, ll, 0], b2_b[:, :, ll, 0]
        assert np.abs(A - A.conj().T).max() < 1e-12
        assert np.abs(S - S.conj().T).max() < 1e-12
        assert np.linalg.eigvalsh(S).min() > 0
    rec.close()


@pytest.mark.parametrize("opts", [{"spmm5": 0}, {"spmm5": 2}, {"spmm5": 2, "side_stream": 0}, {"spmm5": 0, "side_stream": 0}, {"batch": 1},
                                  {"spmm5": 2, "chain_fold": 2}, {"spmm5": 2, "s5_cap": 8}, {"spmm5": 2, "s5_queue": 2}, {"spmm5": 2, "s5_queue": 0}, {"spmm5": 2, "s5_lds": 0}])
@pytest.mark.parametrize("name", ["bccFe_nsp2_block", "B2FeCo_block"])
def test_every_block_pipeline_variant(name, opts):
    """Both SpMM kernels of the matrix-core set (small-launch k_spmm4<4> on LayoutRM vectors, k_spmm5 on CI vectors), with and without
    the side stream, meet the bar on a bulk and an impurity fixture."""
    g = load_golden(name)
    rec = make(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"])
    rec.set_option("kernels", 2)
    for k, v in opts.items():
        rec.set_option(k, v)
    rec.recur_b()
    n = g["nrec"]
    assert rel_err(rec.a_b[:, :, :, :n], g["a_b"]) < RTOL
    assert rel_err(rec.b2_b[:, :, :, :n], g["b2_b"]) < RTOL
    rec.close()


def test_batching_is_invisible():
    """Chains advanced one at a time and all together give bit-identical coefficients (fixed-order reductions)."""
    g = load_golden("fccCu001_block_hoh")
    rec = make(problem_dict(g), g["irec"], g["lld"])
    rec.recur_b()
    a1 = rec.a_b.copy()
    rec.set_option("batch", 1)
    rec.recur_b()
    assert np.array_equal(a1, rec.a_b)
    rec.close()


@pytest.mark.parametrize("hoh", [False, True])
def test_side_stream_is_invisible(hoh):
    """The B_{n+1} reduction / eigen-solve on the side stream (overlapped with the next H|u>) changes scheduling only: the
    coefficients are bit-identical with the option off, on a launch wide enough for the two-stage partial sums (11^3 cell)."""
    p = supercell_problem((11, 11, 11), hoh=hoh)
    sites = np.array([1, 700, 1331], dtype=np.int32)
    rec = Recursion(*objects_from(p, sites, 12, emin=-3.0, emax=1.8))
    rec.recur_b()
    a1, b1 = rec.a_b.copy(), rec.b2_b.copy()
    rec.set_option("side_stream", 0)
    rec.recur_b()
    assert np.array_equal(a1, rec.a_b) and np.array_equal(b1, rec.b2_b)
    assert np.isfinite(a1).all() and np.abs(b1[:, :, 1:, :]).max() > 0.0
    # the same for the Chebyshev moments (their reduction runs under the next level's SpMM)
    rec.chebyshev_recur()
    m0 = rec.mu_n.copy()
    rec.set_option("side_stream", 1)
    rec.chebyshev_recur()
    assert np.array_equal(m0, rec.mu_n) and np.abs(m0).max() > 0.0
    rec.close()


@pytest.mark.parametrize("kernels", BLOCK_VARIANTS)
@pytest.mark.parametrize("name", PAIR_CASES)
def test_pair_variants_golden(name, kernels):
    """recur_b_ij / chebyshev_recur_ij (recursion.f90:1655 / :2376): four chains per pair, against the compiled reference."""
    g = load_golden(name)
    p = supercell_problem(g["dims"], hoh=bool(g["hoh"]))
    ham, lat, ctl, en = objects_from(p, [1], int(g["lld"]), emin=float(g["emin"]), emax=float(g["emax"]))
    lat.ijpair = np.asarray(g["pairs"], dtype=np.int32)
    rec = Recursion(ham, lat, ctl, en)
    select_kernels(rec, kernels)
    if "cheb" in name:
        rec.chebyshev_recur_ij()
        assert rel_err(rec.mu_n, g["mu_n"]) < RTOL
    else:
        rec.recur_b_ij()
        assert rel_err(rec.a_b, g["a_b"]) < RTOL and rel_err(rec.b2_b, g["b2_b"]) < RTOL
        assert np.all(rec.a_b[:, :, :, 5:8] == 0)          # pair (7,7): slots 2..4 untouched (:1705-1706)
    rec.close()


def test_errors_are_loud():
    g = load_golden("bccFe_nsp2_cheb")
    # an energy window far too narrow makes the moments blow up: the reference calls g_logger%fatal (recursion.f90:2594)
    rec = make(problem_dict(g), g["irec"], g["lld"], emin=-0.05, emax=0.05)
    from rslmtoasa_amd._lib import ERR_DIVERGED, RsrecError
    with pytest.raises(RsrecError) as ei:
        rec.chebyshev_recur()
    assert ei.value.code == ERR_DIVERGED and "did not converge" in str(ei.value)
    rec.close()


def test_refused_lattice_leaves_the_engine_usable():
    """rsrec_set_lattice validates before it touches the handle: after a refused table the old lattice still answers, bit for bit."""
    from rslmtoasa_amd._lib import ERR_ARG, RsrecError
    g = load_golden("bccFe_nsp2_block")
    rec = make(problem_dict(g), g["irec"], g["lld"])
    rec.recur_b()
    a0, b0 = rec.a_b.copy(), rec.b2_b.copy()
    good = rec.lattice.nn
    bad = np.array(good, copy=True, order="F")
    bad[bad.shape[0] // 2, 2] = bad.shape[0] + 7             # a neighbour index outside the cluster, found after half the rows were converted
    rec.lattice.nn = bad
    with pytest.raises(RsrecError) as ei:
        rec.update_lattice()
    assert ei.value.code == ERR_ARG and "outside" in str(ei.value)
    rec.lattice.nn = good
    rec.update_lattice()
    rec.restore_to_default()
    rec.recur_b()
    assert np.array_equal(rec.a_b, a0) and np.array_equal(rec.b2_b, b0)
    rec.close()


@pytest.mark.parametrize("name", ["Pt2MnGa_nsp4_local_axis", "Pt2MnGa_nsp4_local_axis_hoh"])
def test_local_axis_batched_block_lanczos(name):
    """hamiltonian%local_axis = T (recursion.f90:1830-1832): four sites (Mn, Ga, Pt1, Pt2) with four different moment directions,
    every chain in ITS spin frame.  The reference rotates all blocks per site and runs the sites one by one; here all four chains
    go in one call on the global-frame blocks (per-chain on-site l.s term + conjugation of the outputs).  Fixture: the compiled
    reference's coefficients in each site's local frame, its global-frame blocks and rotation matrices."""
    g = load_golden(name)
    assert int(g["local_axis"]) == 1 and g["nrec"] == 4
    moms = g["mom"].T
    assert len({tuple(np.round(m, 6)) for m in moms}) == 4                 # four inequivalent directions
    rec = make(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"])
    rec.recur_b_local_axis(g["rot"])
    n = g["nrec"]
    assert rel_err(rec.a_b[:, :, :, :n], g["a_b"]) < RTOL
    assert rel_err(rec.b2_b[:, :, :, :n], g["b2_b"]) < RTOL
    assert np.all(rec.a_b[:, :, -1] == 0) and np.array_equal(rec.b2_b[:, :, 0, 0], np.eye(18))
    # running in the global frame instead (what a run without local_axis would give) is a DIFFERENT result for the tilted sites
    rec.recur_b()
    assert rel_err(rec.a_b[:, :, :, :1], g["a_b"][:, :, :, :1]) > 1e-6
    rec.close()
