"""rsrec_chebyshev_lattice (kernels_lattice.hpp): Chebyshev moments from whole-lattice seeds, M_g(n) = sum_{j in g} conj(c_j) [T_n(H~) x]_j,
and its Python front ends (chebyshev_lattice, bloch_average, bloch_average_spectral, cell_moments).

References: the dense numpy restatement (lattice_seed_reference.lattice_moments), the chain-free oracle T_n(H~(k)) on a periodic one-type
cell (bloch_reference.bloch_hamiltonian_moments) and M_ii of rsrec_chebyshev_pairs_direct.  Deviations are judged at helpers.RTOL (1e-10) of
the largest element of an image; the LDOS stage behind the call at the tolerances tests/test_gpu_cheb_ldos.py gives it."""
import ctypes as C
import functools

import numpy as np
import pytest

from bloch_reference import bloch_hamiltonian_moments, commensurate_k, stencil_column, supercell_cell
from helpers import RTOL, objects_from, random_vec_coefficients, supercell_problem
from kubo_cases import same_bits
from lattice_seed_reference import ALLOY_K, ALLOY_LLD, alloy_case, lattice_moments, plane_wave_seeds
from pair_direct_reference import dense_h
from rslmtoasa_amd import _lib
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.lattice import supercell_positions
from rslmtoasa_amd.recursion import Recursion, chebyshev_scaling
from test_gpu_ldos import ldos_from_g0
from test_gpu_spmm_random import random_problem

pytestmark = pytest.mark.gpu

KERNEL_SETS = [1, 2]            # VALU kernels on the reference's layout; matrix-core kernels on CI vectors
NGROUP_MAX = 16                 # RSREC_LATTICE_NGROUP_MAX (include/rsrec.h)


def make_rec(p, lld, emin, emax, kernels=None, pairs=None):
    ham, lat, ctl, en = objects_from(p, [1], lld, emin=emin, emax=emax)
    if pairs is not None:
        lat.ijpair = np.asarray(pairs, np.int32).reshape(-1, 2)
    rec = Recursion(ham, lat, ctl, en, device=0)
    if kernels is not None:
        rec.set_option("kernels", kernels)
    return rec


def alloy_rec(hoh=False, kernels=None, lld=ALLOY_LLD):
    dims, p, H, a, b, emin, emax, cr, cell = alloy_case(hoh)
    return make_rec(p, lld, emin, emax, kernels), dims, p, H, a, b, cr


def image_errors(mine, ref):
    """Largest deviation of every (group, chain) image relative to the largest element of that image of ``ref``; an image that is all
    zero in ``ref`` must be all zero."""
    def one(m, r):
        scale = np.abs(r).max()
        if scale == 0:
            return 0.0 if np.all(m == 0) else np.inf
        return float(np.abs(m - r).max() / scale)
    assert mine.shape == ref.shape
    return [[one(mine[..., g, c], ref[..., g, c]) for g in range(ref.shape[3])] for c in range(ref.shape[4])]


def worst(mine, ref):
    return max(max(row) for row in image_errors(mine, ref))


def alloy_groups(p):
    """By type, and by type with a fifth of the atoms left out."""
    by_type = p["iz"].astype(np.int32)
    partial = by_type.copy()
    partial[::5] = 0
    return by_type, partial


@functools.lru_cache(maxsize=None)
def alloy_reference(hoh):
    """The dense restatement of the alloy calls, computed once: (k, by type, with a fifth of the atoms in group 0)."""
    dims, p, H, a, b, _, _, cr, _ = alloy_case(hoh)
    k = commensurate_k(dims, ALLOY_K)
    seeds, coefs = plane_wave_seeds(k, cr)
    refs = [lattice_moments(H, a, b, seeds, coefs, ALLOY_LLD, g, 2) for g in alloy_groups(p)]
    for r in refs:
        r.setflags(write=False)
    return k, refs[0], refs[1]


@pytest.mark.parametrize("kernels", KERNEL_SETS)
@pytest.mark.parametrize("hoh", [False, True])
def test_alloy_bloch_average(hoh, kernels):
    """Cases 1 and 2: two-type 4x4x8 alloy (with hoh: the hoh stencil duplicated along the type axis), lld 5, three commensurate k with
    Gamma, ngroup = 2 by type, against the restatement; again with a fifth of the atoms in group 0."""
    rec, dims, p, H, a, b, cr = alloy_rec(hoh, kernels)
    k, ref_type, ref_part = alloy_reference(hoh)
    by_type, partial = alloy_groups(p)
    m_type = rec.bloch_average(k, cr, group=by_type)
    t = rec.timing()
    m_part = rec.bloch_average(k, cr, group=partial)
    rec.close()
    assert m_type.shape == (18, 18, 2 * ALLOY_LLD + 2, 2, 3)
    e_type, e_part = worst(m_type, ref_type), worst(m_part, ref_part)
    print("hoh %s kernels %d: by type %.2e, a fifth left out %.2e" % (hoh, kernels, e_type, e_part))
    assert e_type <= RTOL and e_part <= RTOL
    # the normalisation the docstrings state: tr M_g(1) = 18 N_g / kk
    for g in (1, 2):
        assert np.allclose(np.trace(m_type[:, :, 0, g - 1, :]).real, 18.0 * (by_type == g).sum() / 128, rtol=1e-13, atol=0)
    assert t["hop_launches"] == (2 if hoh else 1) * (2 * ALLOY_LLD + 1) and t["total_ms"] > 0 and t["hop_ms"] > 0 and t["rest_ms"] > 0


@pytest.mark.parametrize("kernels", KERNEL_SETS)
@pytest.mark.parametrize("hoh", [False, True])
def test_ragged_lattice_with_per_atom_blocks(hoh, kernels):
    """Case 3: a random ragged lattice of 75 atoms (odd), two types, 9 atoms with their own operator blocks; three random-phase vectors
    in the random_vec convention, three random groups with 0, against the restatement.  a bounds the operator norm as in
    kubo_cases.ragged_case."""
    rng = np.random.default_rng(4243 + int(hoh))
    kk, lld, emin, emax = 75, 4, -51.0, 51.0
    p = random_problem(rng, kk, 5, 2, 9, hoh, False)
    if hoh:
        p["eeo"] = np.asfortranarray(p["eeo"] * 0.1)
        p["hallo"] = np.asfortranarray(p["hallo"] * 0.1)
    seeds, coefs = random_vec_coefficients(rng.random((kk, 3)))
    group = rng.integers(0, 4, kk).astype(np.int32)
    assert all((group == g).sum() > 0 for g in range(4))
    a, b = chebyshev_scaling(emin, emax)
    ref = lattice_moments(dense_h(p), a, b, seeds, coefs, lld, group, 3)
    rec = make_rec(p, lld, emin, emax, kernels)
    m = rec.chebyshev_lattice(seeds, coefs, group=group)
    m_py = rec.cell_moments(np.zeros((kk, 1)), group=group)
    rec.close()
    assert min(np.abs(ref[..., g, c]).max() for g in range(3) for c in range(3)) > 0
    err = worst(m, ref)
    print("hoh %s kernels %d: ragged lattice %.2e" % (hoh, kernels, err))
    assert err <= RTOL
    assert m_py.shape == (18, 18, 2 * lld + 2, 3, 1)


@functools.lru_cache(maxsize=None)
def cube_case():
    """One-type 9x9x9 cell (729 atoms, odd), three layer groups of 162, 243 and 324 atoms: 10, 15 and 20 splits, each with a remainder."""
    dims, lld, emin, emax = (9, 9, 9), 6, -3.0, 1.8
    p = supercell_problem(dims)
    cr, cell = supercell_positions(dims), supercell_cell(dims)
    k = commensurate_k(dims, [(0, 0, 0), (4, 0, 0), (1, 2, 3), (8, 5, 7)])
    a, b = chebyshev_scaling(emin, emax)
    ref = bloch_hamiltonian_moments(stencil_column(p, 365), a, b, 365, lld, cr, cell, k)      # (18,18,nmom,nk)
    ref.setflags(write=False)
    layer = np.arange(729) // 81
    group = np.where(layer < 2, 1, np.where(layer < 5, 2, 3)).astype(np.int32)
    return dims, p, lld, emin, emax, cr, k, group, ref


@pytest.mark.parametrize("kernels", KERNEL_SETS)
def test_layer_groups_against_the_bloch_hamiltonian(kernels):
    """Case 4: plane-wave seeds at commensurate k: every image equals (N_g / N) T_n(H~(k)).  No dense matrix is formed."""
    dims, p, lld, emin, emax, cr, k, group, ref = cube_case()
    rec = make_rec(p, lld, emin, emax, kernels)
    m = rec.bloch_average(k, cr, group=group)
    rec.close()
    assert m.shape == (18, 18, 2 * lld + 2, 3, 4)
    errs = []
    for g in (1, 2, 3):
        want = (group == g).sum() / 729.0 * ref
        errs.append(max(np.abs(m[:, :, :, g - 1, q] - want[..., q]).max() / np.abs(want[..., q]).max() for q in range(4)))
    print("kernels %d: 9x9x9 layer groups %s" % (kernels, " ".join("%.2e" % e for e in errs)))
    assert max(errs) <= RTOL


@pytest.mark.parametrize("kernels", KERNEL_SETS)
def test_one_atom_seed_against_the_pair_call(kernels):
    """Case 5: a seed on one atom with coefficient 1 gives M_ii of rsrec_chebyshev_pairs_direct."""
    dims, p, H, a, b, emin, emax, cr, cell = alloy_case(False)
    rec = make_rec(p, ALLOY_LLD, emin, emax, kernels, pairs=[[37, 37], [90, 90]])
    m_pair = rec.chebyshev_recur_ij_direct(both_ends=False)
    m = rec.chebyshev_lattice([[37], [90]], [[1.0], [1.0]])
    rec.close()
    for c in range(2):
        ref = m_pair[:, :, :, 0, c]
        err = np.abs(m[:, :, :, 0, c] - ref).max() / np.abs(ref).max()
        print("kernels %d: atom %d against M_ii %.2e" % (kernels, (37, 90)[c], err))
        assert err <= RTOL


@pytest.mark.parametrize("kernels", KERNEL_SETS)
def test_bitwise(kernels):
    """Case 6: the images of a chain and group do not depend on the run, on lattice_vbatch, on the order of the chains, on the labels of
    the atoms outside the group, or on what an unrelated Kubo call left in the buffers."""
    rec, dims, p, H, a, b, cr = alloy_rec(False, kernels)
    kk = 128
    rng = np.random.default_rng(19)
    seeds, coefs = random_vec_coefficients(rng.random((kk, 9)))             # 9 chains: a full batch of 8 and a short one
    group = rng.integers(0, 4, kk).astype(np.int32)
    first = rec.chebyshev_lattice(seeds, coefs, group=group)
    assert min(np.abs(first[..., g, c]).max() for g in range(3) for c in range(9)) > 0
    assert same_bits(first, rec.chebyshev_lattice(seeds, coefs, group=group))                       # two runs of the same call
    rec.set_option("lattice_vbatch", 1)
    assert same_bits(first, rec.chebyshev_lattice(seeds, coefs, group=group))                       # lattice_vbatch 1 against 8
    rec.set_option("lattice_vbatch", 0)
    rev = rec.chebyshev_lattice(seeds[::-1], coefs[::-1], group=group)                              # the chains in reversed order
    assert same_bits(first, rev[..., ::-1])
    relabel = group.copy()                                                                          # group 1 keeps its atoms, the others swap theirs
    relabel[group == 0] = 3
    relabel[group == 2] = 0
    relabel[group == 3] = 2
    other = rec.chebyshev_lattice(seeds, coefs, group=relabel)
    assert same_bits(first[:, :, :, 0, :], other[:, :, :, 0, :]) and same_bits(first[:, :, :, 2, :], other[:, :, :, 1, :])
    v = np.asfortranarray(0.1 * (rng.standard_normal(p["ee"].shape) + 1j * rng.standard_normal(p["ee"].shape)))
    rec.compute_moments_stochastic(v, v, 3, seeds=seeds[:2], coefs=coefs[:2], diag=True)            # an unrelated Kubo call
    assert same_bits(first, rec.chebyshev_lattice(seeds, coefs, group=group))
    rec.close()


def test_resident_image_feeds_pack_and_ldos(oracle_lib):
    """Case 7: with m_g = NULL rsrec_pack_moments gives the bits of a downloading call, and rsrec_chebyshev_ldos on
    nsites_total = nchains * ngroup images agrees with the CPU sum on the downloaded moments."""
    rec, dims, p, H, a, b, cr = alloy_rec(False, None)
    k, _, _ = alloy_reference(False)
    by_type, _ = alloy_groups(p)
    m = rec.bloch_average(k, cr, group=by_type)
    assert rec.bloch_average(k, cr, group=by_type, download=False) is None
    nimg, nmom = 2 * 3, 2 * ALLOY_LLD + 2
    img = np.full((18, 18, nmom, nimg + 3), 7.0 + 0j, order="F")
    rec.pack_moments(2, nimg + 3, img)
    mu = m.reshape(18, 18, nmom, nimg, order="F")
    assert same_bits(img[..., 2:2 + nimg], mu) and np.all(img[..., :2] == 0) and np.all(img[..., 2 + nimg:] == 0)
    ene = np.linspace(rec.en.energy_min + 0.4, rec.en.energy_max - 0.4, 41)
    gr = Green(rec, ene)
    r = gr.chebyshev_ldos(nsites_total=nimg)
    g0_cpu = np.stack([oracle_lib.chebyshev_green(mu[..., i], ene, rec.en.energy_min, rec.en.energy_max) for i in range(nimg)], axis=3)
    dt, da, dl = ldos_from_g0(g0_cpu)
    scale = np.abs(dl).max()
    e_l, e_a, e_t = np.abs(r["dosial"] - dl).max(), np.abs(r["dosia"] - da).max(), np.abs(r["dtot"] - dt).max()
    print("ldos on the resident image against the CPU sum: dosial %.2e dosia %.2e dtot %.2e of %.3e" % (e_l, e_a, e_t, scale))
    assert scale > 0 and e_l <= 1e-10 * scale and e_a <= 1e-10 * scale and e_t <= 1e-10 * nimg * scale
    # the Python front end returns the same numbers, reshaped
    spec = rec.bloch_average_spectral(gr, k, cr, group=by_type)
    rec.close()
    assert spec.shape == (2, 3, 18, 41)
    assert np.array_equal(spec, r["dosial"].reshape((2, 3, 18, 41), order="F"))


def test_errors_leave_the_handle_usable():
    """Case 8: every RSREC_ERR_ARG of the header, each followed by a good call on the same handle; nchains = 0."""
    rec, dims, p, H, a, b, cr = alloy_rec(False, None)
    k, _, _ = alloy_reference(False)
    seeds, coefs = plane_wave_seeds(k, cr)
    coefs = np.ascontiguousarray(coefs)
    good = rec.chebyshev_lattice(seeds, coefs)
    L, h = rec._L, rec._h
    P = lambda arr: None if arr is None else arr.ctypes.data_as(C.c_void_p)
    grp = np.ones(128, np.int32)
    out = np.zeros_like(good)

    def call(nchains=3, nseed=128, atoms=seeds, coef=coefs, lld=ALLOY_LLD, a_=a, ngroup=1, group=None, m_g=out):
        return L.rsrec_chebyshev_lattice(h, nchains, nseed, P(atoms), P(coef), lld, a_, b, ngroup, P(group), P(m_g))
    assert call() == 0 and np.array_equal(out, good)
    bad_group = grp.copy(); bad_group[17] = 2
    neg_group = grp.copy(); neg_group[0] = -1
    big_atom = seeds.copy(); big_atom[1, 5] = 129
    neg_atom = seeds.copy(); neg_atom[2, 0] = -1
    no_seed = seeds.copy(); no_seed[1, :] = 0
    cases = dict(ngroup_zero=dict(ngroup=0, group=grp), ngroup_large=dict(ngroup=NGROUP_MAX + 1, group=grp), group_value=dict(group=bad_group),
                 group_negative=dict(group=neg_group), group_missing=dict(ngroup=2), atom_large=dict(atoms=big_atom), atom_negative=dict(atoms=neg_atom),
                 chain_without_seed=dict(atoms=no_seed), nseed_zero=dict(nseed=0), nseed_large=dict(nseed=129), no_atoms=dict(atoms=None),
                 no_coefs=dict(coef=None), lld_zero=dict(lld=0), a_zero=dict(a_=0.0), nchains_negative=dict(nchains=-1))
    for name, kw in cases.items():
        assert call(**kw) == _lib.ERR_ARG, name
        buf = C.create_string_buffer(512)
        L.rsrec_last_error(h, buf, 512)
        assert b"rsrec_chebyshev_lattice" in buf.value, name
        out[:] = 0
        assert call() == 0 and np.array_equal(out, good), name    # the handle still works
    assert call(nchains=0) == 0 and call(nchains=0, atoms=None, coef=None, m_g=None) == 0
    rec.close()


def test_a_window_too_narrow_diverges():
    """Case 8: a window a tenth of the spectrum's width is an error return, and the handle goes on working."""
    rec, dims, p, H, a, b, cr = alloy_rec(False, None)
    k, ref_type, _ = alloy_reference(False)
    by_type, _ = alloy_groups(p)
    good_window = rec.en.energy_min, rec.en.energy_max
    width = good_window[1] - good_window[0]
    rec.en.energy_min, rec.en.energy_max = -0.05 * width, 0.05 * width
    with pytest.raises(_lib.RsrecError) as ei:
        rec.bloch_average(k, cr, group=by_type)
    assert ei.value.code == _lib.ERR_DIVERGED
    rec.en.energy_min, rec.en.energy_max = good_window
    m = rec.bloch_average(k, cr, group=by_type)
    rec.close()
    assert worst(m, ref_type) <= RTOL
