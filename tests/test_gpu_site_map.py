"""rsrec_chebyshev_site_map (kernels_sitemap.hpp): the 18 x 18 block of ne functions of H on every atom from whole-lattice seeds,
D(:,:,e,j) = sum_n w(n,e) sum_v conj(c^v_j) [T_{n-1}(H~) x^v]_j, and its Python front ends (site_map, site_ldos, site_occupations).

References: the dense numpy restatement (site_map_reference.site_map), the dense on-site blocks (onsite_function), the chain-free oracle
T_n(H~(k)) on a periodic one-type cell (bloch_reference.bloch_hamiltonian_moments), M_ii of rsrec_chebyshev_pairs_direct and the group
moments of rsrec_chebyshev_lattice.  Deviations are judged at helpers.RTOL (1e-10) of the largest element of the reference output, as the
sibling tests judge; the bitwise statements are those of the header's reproducibility contract and no more."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import RTOL, random_vec_coefficients
from kubo_cases import ptr, same_bits, torch_first  # noqa: F401  (torch_first: autouse fixture)
from lattice_seed_reference import ALLOY_K, ALLOY_LLD, alloy_case, plane_wave_seeds
from bloch_reference import commensurate_k
from pair_direct_reference import dense_h
from rslmtoasa_amd import _lib
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.lattice import supercell_colouring
from rslmtoasa_amd.recursion import chebyshev_fermi_weights, chebyshev_scaling, probing_seeds
from site_map_reference import onsite_function, site_map, worst
from test_gpu_lattice_seed import alloy_rec, cube_case, make_rec
from test_gpu_spmm_random import random_problem

pytestmark = pytest.mark.gpu

KERNEL_SETS = [1, 2]
NAME = b"rsrec_chebyshev_site_map"


def random_weights(seed, lld, ne):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal((2 * lld + 2, ne)) + 1j * rng.standard_normal((2 * lld + 2, ne)))


def raw(rec, seeds, coefs, lld, a, b, w, full="host", diag="host", norm=True, **kw):
    """The library call itself: (rc, d_full, d_diag, cnorm) with each output in host memory, device memory (a torch tensor, returned as
    numpy) or absent (None).  ``kw`` overrides single arguments (nvec, nseed, ne, atoms, coef, w_arg)."""
    sd = np.ascontiguousarray(seeds, np.int32)
    cf = np.ascontiguousarray(coefs, np.complex128).reshape(sd.shape)
    w = None if w is None else np.asfortranarray(w, dtype=np.complex128)
    ne = kw.get("ne", 0 if w is None else w.shape[1])
    kk = rec.lattice.kk

    def alloc(kind, shape):
        if kind is None:
            return None
        if kind == "host":
            return np.zeros(shape, np.complex128, order="F")
        import torch
        return torch.zeros(shape[::-1], dtype=torch.complex128, device="cuda")
    nw = max(1, min(ne, 16))
    d_full, d_diag = alloc(full, (18, 18, nw, kk)), alloc(diag, (18, nw, kk))
    cnorm = np.zeros(kk) if norm else None
    rc = rec._L.rsrec_chebyshev_site_map(rec._h, kw.get("nvec", sd.shape[0]), kw.get("nseed", sd.shape[1]), ptr(kw.get("atoms", sd)), ptr(kw.get("coef", cf)),
                                         lld, a, b, ne, ptr(kw.get("w_arg", w)), ptr(d_full), ptr(d_diag), ptr(cnorm))

    def host(x):
        if x is None or isinstance(x, np.ndarray):
            return x
        import torch
        torch.cuda.synchronize()
        return x.cpu().numpy().transpose(tuple(range(x.ndim))[::-1])
    return rc, host(d_full), host(d_diag), cnorm


def last_error(rec):
    buf = C.create_string_buffer(512)
    rec._L.rsrec_last_error(rec._h, buf, 512)
    return buf.value


@functools.lru_cache(maxsize=None)
def alloy_reference(hoh):
    """Case 1's inputs and its dense restatement, computed once: three plane-wave vectors at ALLOY_K, ne = 3 random complex weights."""
    dims, p, H, a, b, _, _, cr, _ = alloy_case(hoh)
    seeds, coefs = plane_wave_seeds(commensurate_k(dims, ALLOY_K), cr)
    w = random_weights(11, ALLOY_LLD, 3)
    ref = site_map(H, a, b, seeds, coefs, ALLOY_LLD, w)
    for r in ref:
        r.setflags(write=False)
    return seeds, np.ascontiguousarray(coefs), w, ref


@pytest.mark.parametrize("kernels", KERNEL_SETS)
@pytest.mark.parametrize("hoh", [False, True])
def test_alloy_plane_waves(hoh, kernels):
    """Cases 1 and 11: 4x4x8 two-type alloy, lld 5 (12 orders: six passes of 2), three plane-wave vectors (a short tile of VT = 8),
    ne = 3: d_full, d_diag and cnorm against the restatement; the launch count and the timing slots."""
    rec, dims, p, H, a, b, cr = alloy_rec(hoh, kernels)
    seeds, coefs, w, (r_full, r_diag, r_norm) = alloy_reference(hoh)
    d_full, d_diag, cnorm = rec.site_map(seeds, coefs, weights=w)
    t = rec.timing()
    rec.close()
    e_full, e_diag, e_norm = worst(d_full, r_full), worst(d_diag, r_diag), worst(cnorm, r_norm)
    print("hoh %s kernels %d: d_full %.2e d_diag %.2e cnorm %.2e" % (hoh, kernels, e_full, e_diag, e_norm))
    assert d_full.shape == (18, 18, 3, 128) and d_diag.shape == (18, 3, 128) and cnorm.shape == (128,)
    assert e_full <= RTOL and e_diag <= RTOL and e_norm <= 1e-15
    assert t["hop_launches"] == (2 if hoh else 1) * (2 * ALLOY_LLD + 1) and t["total_ms"] > 0 and t["hop_ms"] > 0
    assert t["site_accum_ms"] > 0 and t["site_out_ms"] > 0 and abs(t["rest_ms"] - t["site_accum_ms"] - t["site_out_ms"]) <= 1e-9 * t["rest_ms"]


RAGGED_KK, RAGGED_LLD, RAGGED_WINDOW = 75, 4, (-51.0, 51.0)
RAGGED_BARE = (7, 40, 63)          # 0-based atoms no vector seeds


@functools.lru_cache(maxsize=None)
def ragged_case(hoh):
    """Case 2's lattice, as test_ragged_lattice_with_per_atom_blocks builds it: 75 atoms (odd; 24 300 elements, no multiple of 256), two
    types, 9 atoms with their own operator blocks.  Five random-phase vectors; a fifth of each vector's entries, drawn per vector, and
    three atoms in every vector are set to atom 0.  ne = 16 random complex weights.  Returns (p, a, b, seeds, coefs, w, restatement)."""
    rng = np.random.default_rng(4243 + int(hoh))
    p = random_problem(rng, RAGGED_KK, 5, 2, 9, hoh, False)
    if hoh:
        p["eeo"] = np.asfortranarray(p["eeo"] * 0.1)
        p["hallo"] = np.asfortranarray(p["hallo"] * 0.1)
    seeds, coefs = random_vec_coefficients(rng.random((RAGGED_KK, 5)))
    seeds = seeds.copy()
    for v in range(5):
        seeds[v, rng.permutation(RAGGED_KK)[:RAGGED_KK // 5]] = 0
        seeds[v, list(RAGGED_BARE)] = 0
    a, b = chebyshev_scaling(*RAGGED_WINDOW)
    w = random_weights(12, RAGGED_LLD, 16)
    ref = site_map(dense_h(p), a, b, seeds, coefs, RAGGED_LLD, w)
    for r in ref:
        r.setflags(write=False)
    assert (ref[2] == 0).sum() == len(RAGGED_BARE) and 0 < ((seeds == 0).sum(axis=0) > 0).sum() < RAGGED_KK
    return p, a, b, seeds, coefs, w, ref


def ragged_rec(hoh, kernels=None):
    return make_rec(ragged_case(hoh)[0], RAGGED_LLD, *RAGGED_WINDOW, kernels)


@pytest.mark.parametrize("kernels", KERNEL_SETS)
@pytest.mark.parametrize("hoh", [False, True])
def test_ragged_lattice_with_unseeded_atoms(hoh, kernels):
    """Case 2: five vectors (a short tile of the default VT = 8; full tiles next to short ones and a short last pass: test_every_tile_shape),
    10 orders, the element tail, ne = 16 and ne = 1; an atom seeded by no vector is an exact zero block."""
    p, a, b, seeds, coefs, w, (r_full, r_diag, r_norm) = ragged_case(hoh)
    rec = ragged_rec(hoh, kernels)
    d_full, d_diag, cnorm = rec.site_map(seeds, coefs, weights=w)
    one_full, one_diag, _ = rec.site_map(seeds, coefs, weights=w[:, 5:6])
    rec.close()
    errs = worst(d_full, r_full), worst(d_diag, r_diag), worst(one_full, r_full[:, :, 5:6]), worst(one_diag, r_diag[:, 5:6])
    print("hoh %s kernels %d: ne 16 d_full %.2e d_diag %.2e, ne 1 d_full %.2e d_diag %.2e" % ((hoh, kernels) + errs))
    # cnorm: |c|^2 as re^2 + im^2 here and as hypot^2 in the restatement, a few ulp apart; five positive terms keep the relative error
    assert max(errs) <= RTOL and worst(cnorm, r_norm) <= 1e-15
    bare = list(RAGGED_BARE)
    assert np.all(d_full[..., bare] == 0) and np.all(d_diag[..., bare] == 0) and np.all(one_full[..., bare] == 0) and np.all(cnorm[bare] == 0)
    assert min(np.abs(d_full[..., j]).max() for j in range(RAGGED_KK) if j not in bare) > 0


@functools.lru_cache(maxsize=None)
def probing_case():
    """Case 3's inputs: the alloy, stride 4 (64 colours of 2 atoms at least 4 hops apart, asserted by test_site_map_restatement), random
    signs, lld 1 (degree 3), and the dense on-site blocks."""
    dims, p, H, a, b, emin, emax, _, _ = alloy_case(False)
    seeds, coefs = probing_seeds(supercell_colouring(dims, 4), np.random.default_rng(6))
    w = random_weights(13, 1, 3)
    ref = onsite_function(H, a, b, 1, w)
    ref.setflags(write=False)
    return p, emin, emax, seeds, coefs, w, ref


@pytest.mark.parametrize("vbatch", [0, 3])
def test_exact_probing(vbatch):
    """Case 3: 64 probing vectors of degree 3 below the colour distance 4: D / cnorm equals the dense on-site blocks on all 128 atoms.
    vbatch 0: eight batches of 8; vbatch 3: 22 batches, the last of one vector; the accumulators persist across them."""
    p, emin, emax, seeds, coefs, w, ref = probing_case()
    rec = make_rec(p, 1, emin, emax)
    rec.set_option("kubo_vbatch", vbatch)
    d_full, _, cnorm = rec.site_map(seeds, coefs, weights=w, diag=False)
    t = rec.timing()
    rec.close()
    err = worst(d_full / cnorm[None, None, None, :], ref)
    print("kubo_vbatch %d: exact probing %.2e" % (vbatch, err))
    assert np.array_equal(cnorm, np.ones(128)) and err <= RTOL
    assert t["hop_launches"] == 3 * (22 if vbatch else 8)


def test_gamma_plane_wave_on_the_odd_cube():
    """Case 4: 9x9x9 one-type cell (729 atoms: two staging slices, the second short), Gamma-point plane wave, lld 6: every atom's block
    equals (1/kk) sum_n w(n,e) T_{n-1}(H~(k = 0)), the chain-free oracle.  No dense matrix is formed."""
    dims, p, lld, emin, emax, cr, k, group, ref = cube_case()
    w = random_weights(14, lld, 2)
    seeds, coefs = plane_wave_seeds(k[:, :1], cr)
    rec = make_rec(p, lld, emin, emax)
    d_full, d_diag, cnorm = rec.site_map(seeds, coefs, weights=w)
    rec.close()
    want = np.einsum("ne,abn->abe", w, ref[..., 0]) / 729.0
    errs = np.abs(d_full - want[..., None]).max(axis=(0, 1, 2)) / np.abs(want).max()
    print("9x9x9 Gamma: worst of 729 blocks %.2e" % errs.max())
    assert errs.shape == (729,) and errs.max() <= RTOL
    assert np.array_equal(d_diag, np.einsum("aaej->aej", d_full)) and np.allclose(cnorm, 1.0 / 729.0, rtol=1e-14, atol=0)


def test_one_atom_seeds_against_the_pair_call():
    """Case 5: seeds on one atom each with coefficient 1 give sum_n w M_ii of rsrec_chebyshev_pairs_direct, run on the device."""
    dims, p, H, a, b, emin, emax, cr, cell = alloy_case(False)
    atoms = [5, 37, 90, 128]
    rec = make_rec(p, ALLOY_LLD, emin, emax, pairs=[[i, i] for i in atoms])
    m_pair = rec.chebyshev_recur_ij_direct(both_ends=False)
    w = random_weights(15, ALLOY_LLD, 2)
    d_full, _, cnorm = rec.site_map([[i] for i in atoms], np.ones((4, 1)), weights=w, diag=False)
    rec.close()
    for c, i in enumerate(atoms):
        ref = np.einsum("ne,abn->abe", w, m_pair[:, :, :, 0, c])
        err = worst(d_full[..., i - 1], ref)
        print("atom %d against sum_n w M_ii: %.2e" % (i, err))
        assert err <= RTOL and cnorm[i - 1] == 1
    others = np.setdiff1d(np.arange(128), np.asarray(atoms) - 1)
    assert np.all(d_full[..., others] == 0) and np.all(cnorm[others] == 0)


def test_group_sums_against_the_lattice_call():
    """Case 6: sum_{j in g} d_full against the weights applied to rsrec_chebyshev_lattice's m_g, summed over the vectors: same seeds,
    groups by type, both on the device."""
    rec, dims, p, H, a, b, cr = alloy_rec(False, None)
    seeds, coefs, w, _ = alloy_reference(False)
    group = p["iz"].astype(np.int32)
    m_g = rec.chebyshev_lattice(seeds, coefs, group=group)                  # (18,18,nmom,2,3)
    d_full, _, _ = rec.site_map(seeds, coefs, weights=w, diag=False)
    rec.close()
    for g in (1, 2):
        ref = np.einsum("ne,abnv->abe", w, m_g[:, :, :, g - 1, :])
        err = worst(d_full[..., group == g].sum(axis=3), ref)
        print("group %d: site sums against rsrec_chebyshev_lattice %.2e" % (g, err))
        assert err <= RTOL


def test_bitwise():
    """Case 7: a repeated call; after an unrelated Kubo call; column e of an ne = 16 call against an ne = 1 call with that column alone;
    d_diag against the diagonal of d_full; either output alone against both; device outputs against host outputs."""
    p, a, b, seeds, coefs, w, _ = ragged_case(False)
    rec = ragged_rec(False)
    call = lambda **kw: raw(rec, seeds, coefs, RAGGED_LLD, a, b, kw.pop("w", w), **kw)
    rc, first, first_diag, first_norm = call()
    assert rc == 0 and np.abs(first).max() > 0
    rc, again, again_diag, again_norm = call()
    assert rc == 0 and same_bits(first, again) and same_bits(first_diag, again_diag) and same_bits(first_norm, again_norm)
    rng = np.random.default_rng(19)
    v = np.asfortranarray(0.1 * (rng.standard_normal(p["ee"].shape) + 1j * rng.standard_normal(p["ee"].shape)))
    full_seeds, full_coefs = random_vec_coefficients(rng.random((RAGGED_KK, 2)))
    rec.compute_moments_stochastic(v, v, 3, seeds=full_seeds, coefs=full_coefs, diag=True)          # an unrelated Kubo call: dirty buffers
    rc, dirty, dirty_diag, _ = call()
    assert rc == 0 and same_bits(first, dirty) and same_bits(first_diag, dirty_diag)
    for e in (0, 7, 15):
        rc, one, one_diag, _ = call(w=w[:, e:e + 1])
        assert rc == 0 and same_bits(one[:, :, 0], first[:, :, e]) and same_bits(one_diag[:, 0], first_diag[:, e]), e
    assert same_bits(first_diag, np.einsum("aaej->aej", first))
    rc, only_full, none_diag, _ = call(diag=None)
    assert rc == 0 and none_diag is None and same_bits(only_full, first)
    rc, none_full, only_diag, none_norm = call(full=None, norm=False)
    assert rc == 0 and none_full is None and none_norm is None and same_bits(only_diag, first_diag)
    rc, dev_full, dev_diag, _ = call(full="device", diag="device")
    assert rc == 0 and same_bits(dev_full, first) and same_bits(dev_diag, first_diag)
    rc, dev_full, host_diag, _ = call(full="device", diag="host")
    assert rc == 0 and same_bits(dev_full, first) and same_bits(host_diag, first_diag)
    rec.close()


def test_every_tile_shape():
    """Case 8: each sitemap_orders in {1, 2, 4, 8, 16} and each sitemap_vtile in {1, 2, 4, 8} on case 2: within RTOL of the restatement
    and bitwise repeatable.  The value left at 0 follows to VT PT = 16, so the five vectors and ten orders meet tiles of 4 + 1 with
    passes of 4, 4, 2 (<4,4>), tiles of 2, 2, 1 with passes of 8, 2 (<2,8>), one pass of 10 (<1,16>), a tile of 5 (<8,1>, <8,2>).
    Bitwise equality between different values is NOT asserted: the accumulator is shared by the vectors."""
    p, a, b, seeds, coefs, w, (r_full, r_diag, _) = ragged_case(False)
    rec = ragged_rec(False)
    for key, values in (("sitemap_orders", (1, 2, 4, 8, 16)), ("sitemap_vtile", (1, 2, 4, 8))):
        for value in values:
            rec.set_option(key, value)
            rc, one, one_diag, _ = raw(rec, seeds, coefs, RAGGED_LLD, a, b, w)
            rc2, two, two_diag, _ = raw(rec, seeds, coefs, RAGGED_LLD, a, b, w)
            err = max(worst(one, r_full), worst(one_diag, r_diag))
            print("%s = %d: %.2e" % (key, value, err))
            assert rc == 0 and rc2 == 0 and err <= RTOL, (key, value)
            assert same_bits(one, two) and same_bits(one_diag, two_diag), (key, value)
        rec.set_option(key, 0)
    rec.set_option("sitemap_orders", 16)
    rec.set_option("sitemap_vtile", 8)                           # both set and 128 loads asked for: VT gives way
    rc, one, _, _ = raw(rec, seeds, coefs, RAGGED_LLD, a, b, w)
    assert rc == 0 and worst(one, r_full) <= RTOL
    rec.close()


def test_refusals_leave_the_handle_usable():
    """Case 9: every RSREC_ERR_ARG of the header with a message that names the function, each followed by a good call with the bits of
    the first; nvec = 0."""
    p, a, b, seeds, coefs, w, _ = ragged_case(False)
    rec = ragged_rec(False)
    good = lambda **kw: raw(rec, seeds, coefs, RAGGED_LLD, a, b, w, **kw)
    rc, first, first_diag, first_norm = good()
    assert rc == 0
    nan_w = w.copy(); nan_w[3, 2] = np.nan
    no_seed = seeds.copy(); no_seed[1, :] = 0
    big_atom = seeds.copy(); big_atom[2, 4] = RAGGED_KK + 1
    neg_atom = seeds.copy(); neg_atom[0, 0] = -1
    cases = dict(ne_zero=dict(ne=0), ne_large=dict(ne=17), no_w=dict(w_arg=None), nan_weight=dict(w_arg=nan_w), no_outputs=dict(full=None, diag=None),
                 vector_without_seed=dict(atoms=no_seed), atom_large=dict(atoms=big_atom), atom_negative=dict(atoms=neg_atom),
                 nseed_zero=dict(nseed=0), nseed_large=dict(nseed=RAGGED_KK + 1), no_atoms=dict(atoms=None), no_coefs=dict(coef=None),
                 nvec_negative=dict(nvec=-1))
    for name, kw in cases.items():
        assert good(**kw)[0] == _lib.ERR_ARG, name
        assert NAME in last_error(rec), name
        rc, again, again_diag, again_norm = good()
        assert rc == 0 and same_bits(again, first) and same_bits(again_diag, first_diag) and same_bits(again_norm, first_norm), name
    for kw in (dict(lld_=0), dict(a_=0.0)):
        rc = raw(rec, seeds, coefs, kw.get("lld_", RAGGED_LLD), kw.get("a_", a), b, w)[0]
        assert rc == _lib.ERR_ARG and NAME in last_error(rec), kw
    rc, untouched, untouched_diag, untouched_norm = good(nvec=0)
    assert rc == 0 and not untouched.any() and not untouched_diag.any() and not untouched_norm.any()
    assert good(nvec=0, atoms=None, coef=None)[0] == 0
    assert same_bits(good()[1], first)
    rec.close()


def test_a_window_too_narrow_diverges():
    """Case 9: a = 0.2 x the sound value at lld 20 puts the spectrum outside [-1, 1]: RSREC_ERR_DIVERGED, the outputs left alone, and
    the handle goes on working."""
    rec, dims, p, H, a, b, cr = alloy_rec(False, None)
    seeds, coefs, w, (r_full, _, _) = alloy_reference(False)
    w20 = random_weights(16, 20, 2)
    rc, d_full, d_diag, _ = raw(rec, seeds, coefs, 20, 0.2 * a, b, w20)
    assert rc == _lib.ERR_DIVERGED and b"energy_min" in last_error(rec)
    assert not d_full.any() and not d_diag.any()
    rc, d_full, _, _ = raw(rec, seeds, coefs, 20, a, b, w20)
    assert rc == 0 and np.isfinite(d_full).all()
    rc, d_full, _, _ = raw(rec, seeds, coefs, ALLOY_LLD, a, b, w)
    rec.close()
    assert rc == 0 and worst(d_full, r_full) <= RTOL


def test_site_ldos_against_the_ordinary_chain():
    """Case 10: site_ldos with a one-atom seed against the LDOS of an ordinary chebyshev_recur site through Green, at the tolerance
    tests/test_gpu_cheb_ldos.py gives that stage: 1e-10 of the largest LDOS."""
    dims, p, H, a, b, emin, emax, cr, cell = alloy_case(False)
    from helpers import objects_from
    from rslmtoasa_amd.recursion import Recursion
    rec = Recursion(*objects_from(p, [37], ALLOY_LLD, emin=emin, emax=emax), device=0)
    rec.chebyshev_recur()
    ene = np.linspace(emin + 0.3, emax - 0.3, 16)
    ref = Green(rec, ene).chebyshev_ldos()["dosial"][0]                      # (18, nen)
    ldos = rec.site_ldos([[37]], [[1.0]], ene)
    rec.close()
    scale = np.abs(ref).max()
    err = np.abs(ldos[:, :, 36] - ref).max()
    print("site_ldos of atom 37 against chebyshev_ldos: %.2e of %.3e" % (err, scale))
    assert ldos.shape == (18, 16, 128) and scale > 0 and err <= 1e-10 * scale
    assert not np.delete(ldos, 36, axis=2).any()


def test_site_occupations_trace_against_cell_moments():
    """Case 10: site_occupations with powers = (0,): the trace summed over all atoms of a random-phase run equals cell_moments
    contracted with the same column of weights, divided by the uniform cnorm, at RTOL of the scale."""
    rec, dims, p, H, a, b, cr = alloy_rec(False, None)
    numbers = np.random.default_rng(23).random((128, 3))
    seeds, coefs = random_vec_coefficients(numbers)
    fermi, kT = 0.5 * (rec.en.energy_min + rec.en.energy_max), 0.1 * a
    occ = rec.site_occupations(seeds, coefs, fermi, kT)
    m = rec.cell_moments(numbers)                                            # (18,18,nmom,1,3)
    rec.close()
    w = chebyshev_fermi_weights(fermi, kT, ALLOY_LLD, rec.en.energy_min, rec.en.energy_max, powers=(0,))
    cnorm = 3.0 * float(np.sqrt(np.float32(128))) ** -2
    moments = np.einsum("aanv->n", m[:, :, :, 0, :])
    want = (w[:, 0] * moments).sum() / cnorm
    scale = (np.abs(w[:, 0]) * np.abs(moments)).sum() / cnorm
    got = np.einsum("aaj->", occ[:, :, 0, :])
    print("sum of the occupation traces %.12g against the cell moments %.12g: %.2e of the scale" % (got.real, want.real, abs(got - want) / scale))
    assert occ.shape == (18, 18, 1, 128) and abs(got - want) <= RTOL * scale
