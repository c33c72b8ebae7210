"""rsrec_chebyshev_bloch_map (kernels_blochmap.hpp): functions of H at many k-points and a few energies from one chain per source atom,
G_i(k, e) = sum_j exp(-i k.d(j, i)) sum_n w(n, e) <j|T_{n-1}(H~)|i>, and the orbital weights a_k = -Im diag G / pi formed beside them.

References: the dense energy-first restatement (bloch_map_reference.bloch_map), the weights applied to the chain-free oracle T_n(H~(k))
(bloch_reference.bloch_hamiltonian_moments), the numpy phase sum over the blocks rsrec_chebyshev_pairs_direct returns, and the existing
device route (rsrec_chebyshev_bloch + rsrec_chebyshev_green).  Deviations are judged as bloch_reference.image_errors judges them, at
helpers.RTOL (1e-10) of the largest element of the (group, source) image: the bound of tests/test_gpu_bloch.py on the same sums."""
import ctypes as C
import functools

import numpy as np
import pytest

from bloch_map_reference import bloch_map, green_weights, weighted_moments
from bloch_reference import bloch_hamiltonian_moments, commensurate_k, fixture_case, image_errors, stencil_column, supercell_cell
from helpers import RTOL, load_golden, problem_dict, supercell_problem
from pair_direct_reference import dense_h
from rslmtoasa_amd import _lib
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.lattice import supercell_positions
from rslmtoasa_amd.recursion import chebyshev_scaling
from test_gpu_bloch import K17, KERNEL_SETS, SOURCES, make_rec, small_case

pytestmark = pytest.mark.gpu

NE_MAX, NK_MAX = 16, 1048576       # RSREC_BLOCH_MAP_NE_MAX, RSREC_BLOCH_MAP_NK_MAX (include/rsrec.h)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's (as bench.py does): test_bitwise hands over device tensors
    torch.cuda.set_device(0)


def worst(mine, ref):
    return max(max(row) for row in image_errors(mine, ref))


def diag_of(g_k):
    """(18, ne, nk, ngroup, nsrc): -Im g_k(l, l, ...) / pi, the expression the device evaluates."""
    return -np.imag(np.einsum("aa...->a...", g_k)) / np.pi


def random_weights(rng, lld, ne):
    return np.asfortranarray(rng.standard_normal((2 * lld + 2, ne)) + 1j * rng.standard_normal((2 * lld + 2, ne)))


@functools.lru_cache(maxsize=None)
def small_reference(hoh):
    """The first test's call restated once: k-points, Green weights of three energies, the dense restatement, the weighted oracle."""
    dims, _, H, a, b, lld, emin, emax, cr, cell = fixture_case(hoh)
    k = commensurate_k(dims, K17)
    ene = np.array([emin + 0.4, -0.1, emax - 0.4])
    w = green_weights(2 * lld + 2, a, b, ene)
    dense = bloch_map(H, a, b, SOURCES, lld, cr, cell, k, w)
    dense.setflags(write=False)
    oracle = {s: weighted_moments(bloch_hamiltonian_moments(H, a, b, s, lld, cr, cell, k), w) for s in set(SOURCES)}
    return k, ene, w, dense, oracle


@pytest.mark.parametrize("kernels", KERNEL_SETS)
@pytest.mark.parametrize("hoh", [False, True])
def test_small_cell_both_kernel_sets(hoh, kernels):
    """4x4x8, lld 12, sources (1, 37, 37), 17 k-points, three energies: the region grows through lists of 15 and 65 atoms (no multiples of
    4 or 16) and covers the cell from level 4 on."""
    rec, dims, H, a, b, lld, cr, cell = small_case(hoh, kernels)
    k, ene, w, dense, oracle = small_reference(hoh)
    assert lld == 12 and k.shape == (3, 17)
    g_k, a_k = rec.bloch_map(SOURCES, k, cr, energies=ene, cell=cell)
    t = rec.timing()
    by_weights = rec.bloch_map(SOURCES, k, cr, weights=w, cell=cell)[0]
    rec.close()
    assert g_k.shape == (18, 18, 3, 17, 1, 3) and a_k.shape == (18, 3, 17, 1, 3)
    e_dense = worst(g_k, dense)
    e_oracle = max(np.abs(g_k[..., 0, i] - oracle[s]).max() / np.abs(oracle[s]).max() for i, s in enumerate(SOURCES))
    e_w = worst(by_weights, dense)
    print("hoh %s kernels %d: against the dense restatement %.2e (the reference's weights %.2e), against the weighted T_n(H~(k)) %.2e"
          % (hoh, kernels, e_dense, e_w, e_oracle))
    assert e_dense <= RTOL and e_oracle <= RTOL and e_w <= RTOL
    assert np.array_equal(a_k, diag_of(g_k))                     # bit for bit the diagonal of g_k
    assert np.array_equal(g_k[..., 1], g_k[..., 2]) and np.array_equal(a_k[..., 1], a_k[..., 2])   # a duplicated source carries the same bits
    assert t["hop_launches"] == (2 if hoh else 1) * (2 * lld + 1) and t["total_ms"] > 0 and t["hop_ms"] > 0 and t["rest_ms"] > 0
    assert abs(t["map_accum_ms"] + t["map_phase_ms"] + t["map_final_ms"] - t["rest_ms"]) <= 1e-9 * t["rest_ms"] and t["map_accum_ms"] > 0


@pytest.mark.parametrize("kernels", KERNEL_SETS)
def test_chunk_boundary(kernels):
    """300 incommensurate k-points with minimum images: 600 phase rows padded to 640, past one 512-row launch; chunks of 256 + 44 by
    default, and of 100 when forced -- the same bits."""
    rec, dims, H, a, b, lld, cr, cell = small_case(False, kernels, lld=6)
    rng = np.random.default_rng(17)
    k = np.asfortranarray(rng.uniform(-4.0, 4.0, (3, 300)))
    w = green_weights(2 * lld + 2, a, b, [-0.3, 0.2])
    sources = [5, 128]
    ref = bloch_map(H, a, b, sources, lld, cr, cell, k, w)
    g_k, a_k = rec.bloch_map(sources, k, cr, weights=w, cell=cell)
    err = worst(g_k, ref)
    print("kernels %d: 300 k-points %.2e" % (kernels, err))
    assert err <= RTOL and np.array_equal(a_k, diag_of(g_k))
    for chunk in (100, 600):                                     # 600: one chunk of two 512-row launches
        rec.set_option("blochmap_kchunk", chunk)
        g_c, a_c = rec.bloch_map(sources, k, cr, weights=w, cell=cell)
        assert np.array_equal(g_c, g_k) and np.array_equal(a_c, a_k), chunk
    rec.close()


@pytest.mark.parametrize("kernels", KERNEL_SETS)
def test_groups(kernels):
    """Three groups from the cell index, a fifth of the atoms left out, the largest ne with random complex weights; relabelling the
    groups permutes the images bit for bit."""
    rec, dims, H, a, b, lld, cr, cell = small_case(False, kernels, lld=6)
    kk = H.shape[0] // 18
    group = (np.arange(kk) // dims[0] % 3 + 1).astype(np.int32)
    group[::5] = 0
    assert all((group == g).sum() > 0 for g in range(4))
    k = commensurate_k(dims, K17[:5])
    w = random_weights(np.random.default_rng(23), lld, NE_MAX)
    g_k, a_k = rec.bloch_map([1, 37], k, cr, weights=w, cell=cell, group=group)
    ref = bloch_map(H, a, b, [1, 37], lld, cr, cell, k, w, group, 3)
    assert g_k.shape == ref.shape == (18, 18, NE_MAX, 5, 3, 2)
    err = worst(g_k, ref)
    print("kernels %d: groups, ne = %d, against the dense restatement %.2e" % (kernels, NE_MAX, err))
    assert err <= RTOL and np.array_equal(a_k, diag_of(g_k))
    perm = np.array([0, 3, 1, 2], np.int32)                      # group g becomes perm[g]
    g_p, a_p = rec.bloch_map([1, 37], k, cr, weights=w, cell=cell, group=perm[group])
    rec.close()
    for g in (1, 2, 3):
        assert np.array_equal(g_p[..., perm[g] - 1, :], g_k[..., g - 1, :]) and np.array_equal(a_p[..., perm[g] - 1, :], a_k[..., g - 1, :]), g


@pytest.mark.parametrize("kernels", KERNEL_SETS)
def test_ragged_lattice(kernels):
    """fuzz_seed_1766: a ragged lattice of two atom types with hoh and a random non-Hermitian operator, random positions, k and groups.
    Its regions stay small (35, 22 and 16 atoms for these sources), so most atoms never join."""
    z = load_golden("fuzz_seed_1766")
    p = problem_dict(z)
    kk, lld, emin, emax = int(z["kk"]), 5, -4.0, 4.0
    rng = np.random.default_rng(3)
    cr = np.asfortranarray(rng.uniform(-3.0, 3.0, (3, kk)))
    k = np.asfortranarray(rng.uniform(-2.0, 2.0, (3, 6)))
    group = rng.integers(0, 3, kk).astype(np.int32)
    w = random_weights(rng, lld, 3)
    sources = [31, 16, 17]
    a, b = chebyshev_scaling(emin, emax)
    ref = bloch_map(dense_h(p), a, b, sources, lld, cr, None, k, w, group, 2)
    rec = make_rec(p, lld, emin, emax, kernels)
    g_k, a_k = rec.bloch_map(sources, k, cr, weights=w, group=group)
    rec.close()
    assert min(np.abs(ref[..., g, s]).max() for g in range(2) for s in range(3)) > 0
    err = worst(g_k, ref)
    print("kernels %d: ragged lattice %.2e" % (kernels, err))
    assert err <= RTOL and np.array_equal(a_k, diag_of(g_k))


@pytest.mark.parametrize("kernels", KERNEL_SETS)
def test_multi_class_cluster_against_the_pair_blocks(kernels):
    """B2FeCo (three types, 15 atoms with their own operator blocks): group 1 is a 40-atom star around an impurity atom; the reference
    is the numpy phase sum of the weighted blocks M_ji rsrec_chebyshev_pairs_direct returns for that star."""
    g = load_golden("B2FeCo_block")
    p = problem_dict(g)
    kk, lld, src = g["nn"].shape[0], 6, 3
    star = np.arange(1, 41)
    rng = np.random.default_rng(5)
    cr = np.asfortranarray(rng.uniform(-2.0, 2.0, (3, kk)))
    k = np.asfortranarray(rng.uniform(-2.0, 2.0, (3, 9)))
    w = random_weights(rng, lld, 2)
    group = np.zeros(kk, np.int32)
    group[star - 1] = 1
    rec = make_rec(p, lld, float(g["emin"]), float(g["emax"]), kernels, pairs=np.stack([np.full(40, src), star], axis=1))
    m_pair = rec.chebyshev_recur_ij_direct(both_ends=False)
    g_k, a_k = rec.bloch_map([src], k, cr, weights=w, group=group)
    rec.close()
    ph = np.exp(-1j * (k.T @ (cr[:, star - 1] - cr[:, src - 1:src])))         # (nk, 40)
    ref = np.einsum("qj,abnj,ne->abeq", ph, m_pair[:, :, :, 1, :], w)[..., None, None]
    err = worst(g_k, ref)
    print("kernels %d: B2FeCo star %.2e" % (kernels, err))
    assert err <= RTOL and np.array_equal(a_k, diag_of(g_k))


def test_agrees_with_the_moment_route():
    """The route a user had before: rsrec_chebyshev_bloch, its moments in rec.mu_n, green%chebyshev_green on a mesh -- against g_k at the
    same energies."""
    rec, dims, H, a, b, lld, cr, cell = small_case(False, None)
    k = commensurate_k(dims, K17)
    ene = np.linspace(rec.en.energy_min + 0.4, rec.en.energy_max - 0.4, 5)
    s_k = rec.chebyshev_bloch([1, 37], k, cr, cell=cell)
    nimg = 17 * 2
    rec.mu_n = np.asfortranarray(s_k.reshape(18, 18, 2 * lld + 2, nimg, order="F"))
    g0 = Green(rec, ene).chebyshev_green(nsites=nimg).copy()     # (18, 18, 5, image)
    g_k, _ = rec.bloch_map([1, 37], k, cr, energies=ene, cell=cell)
    rec.close()
    ref = g0.reshape(18, 18, 5, 17, 1, 2, order="F")
    err = worst(g_k, ref)
    print("against rsrec_chebyshev_bloch + rsrec_chebyshev_green: %.2e" % err)
    assert err <= RTOL


def raw_call(rec, sources, k, cr, cell, w, g_k, a_k, lld, a, b, group=None, ngroup=1):
    """The C entry point itself; g_k / a_k: numpy arrays, raw device addresses or None."""
    P = lambda x: None if x is None else (C.c_void_p(x) if isinstance(x, int) else x.ctypes.data_as(C.c_void_p))
    src = np.ascontiguousarray(sources, np.int32)
    return rec._L.rsrec_chebyshev_bloch_map(rec._h, len(src), P(src), lld, a, b, P(cr), P(cell), k.shape[1], P(k), ngroup, P(group), w.shape[1], P(w), P(g_k), P(a_k))


@pytest.mark.parametrize("kernels", KERNEL_SETS)
def test_bitwise(kernels):
    import torch
    rec, dims, H, a, b, lld, cr, cell = small_case(False, kernels, lld=6)
    k = commensurate_k(dims, K17)
    sources = [1, 37, 90]
    w = green_weights(2 * lld + 2, a, b, [-0.4, -0.1, 0.3])
    run = lambda s=sources, kp=k, ww=w, **kw: rec.bloch_map(s, kp, cr, weights=ww, cell=cell, **kw)
    g1, a1 = run()
    assert np.abs(g1).max() > 0 and np.array_equal(a1, diag_of(g1))
    same = lambda pair: np.array_equal(pair[0], g1) and np.array_equal(pair[1], a1)
    assert same(run())                                           # a repeated call
    rec.recur_b()                                                # other data in the work vectors
    assert same(run())
    rec.set_option("batch", 1)
    assert same(run())
    rec.set_option("batch", 0)
    rec.set_option("blochmap_orders", 1)                         # one order per accumulation pass: the same fmas in the same order
    assert same(run())
    rec.set_option("blochmap_orders", 2)
    g_s, a_s = run(s=[37])                                       # a source alone
    assert np.array_equal(g_s, g1[..., 1:2]) and np.array_equal(a_s, a1[..., 1:2])
    for q in (0, 9, 16):                                         # a k-point alone: nk = 1
        g_q, a_q = run(kp=k[:, q:q + 1])
        assert np.array_equal(g_q, g1[:, :, :, q:q + 1]) and np.array_equal(a_q, a1[:, :, q:q + 1]), q
    for e in range(3):                                           # an energy column alone: ne = 1
        g_e, a_e = run(ww=np.asfortranarray(w[:, e:e + 1]))
        assert np.array_equal(g_e, g1[:, :, e:e + 1]) and np.array_equal(a_e, a1[:, e:e + 1]), e
    g_only, none = run(diag=False)                               # g_k requested alone
    assert none is None and np.array_equal(g_only, g1)
    none, a_only = run(blocks=False)
    assert none is None and np.array_equal(a_only, a1)
    # outputs given as device tensors: written in place, one or both
    for dev_g, dev_a in ((True, True), (True, False), (False, True)):
        t_g, t_a = torch.zeros(g1.size, dtype=torch.complex128, device="cuda"), torch.zeros(a1.size, dtype=torch.float64, device="cuda")
        h_g, h_a = np.zeros_like(g1), np.zeros_like(a1)
        assert raw_call(rec, sources, k, cr, cell, w, t_g.data_ptr() if dev_g else h_g, t_a.data_ptr() if dev_a else h_a, lld, a, b) == 0
        torch.cuda.synchronize()
        got_g = t_g.cpu().numpy().reshape(g1.shape, order="F") if dev_g else h_g
        got_a = t_a.cpu().numpy().reshape(a1.shape, order="F") if dev_a else h_a
        assert np.array_equal(got_g, g1) and np.array_equal(got_a, a1), (dev_g, dev_a)
    rec.close()


def test_errors_leave_the_handle_usable():
    rec, dims, H, a, b, lld, cr, cell = small_case(False, None, lld=6)
    k = commensurate_k(dims, K17[:3])
    w = green_weights(2 * lld + 2, a, b, [-0.2, 0.1])
    good_g, good_a = rec.bloch_map([1, 37], k, cr, weights=w, cell=cell)
    grp = np.ones(128, np.int32)
    out_g, out_a = np.zeros_like(good_g), np.zeros_like(good_a)

    def call(sources=(1, 37), cell_=cell, kpt=k, w_=w, ne=None, nk=None, g_k=out_g, a_k=out_a, group=None, ngroup=1):
        P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        src = np.ascontiguousarray(sources, np.int32)
        return rec._L.rsrec_chebyshev_bloch_map(rec._h, len(src), P(src), lld, a, b, P(cr), P(cell_), kpt.shape[1] if nk is None else nk, P(kpt), ngroup, P(group),
                                                (w_.shape[1] if ne is None else ne), P(w_), P(g_k), P(a_k))
    assert call() == 0 and np.array_equal(out_g, good_g) and np.array_equal(out_a, good_a)
    w17 = np.asfortranarray(np.tile(w[:, :1], (1, NE_MAX + 1)))
    w_nan = w.copy(order="F"); w_nan[5, 1] = complex(0.0, np.nan)
    w_inf = w.copy(order="F"); w_inf[0, 0] = complex(np.inf, 0.0)
    bad_group = grp.copy(); bad_group[17] = 2
    big_k = np.zeros((3, NK_MAX + 1), order="F")
    singular = np.asfortranarray(np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 0.0]]))
    cases = dict(ne_zero=dict(ne=0), ne_large=dict(w_=w17, g_k=None, a_k=np.zeros(18 * 17 * 3 * 2)), nk_zero=dict(nk=0),
                 nk_large=dict(kpt=big_k, g_k=None, a_k=None), no_w=dict(w_=None, ne=2), nan_weight=dict(w_=w_nan), inf_weight=dict(w_=w_inf),
                 no_output=dict(g_k=None, a_k=None), group_value=dict(group=bad_group), group_missing=dict(ngroup=2), singular_cell=dict(cell_=singular),
                 source_zero=dict(sources=(0, 37)), source_large=dict(sources=(1, 129)))
    for name, kw in cases.items():
        assert call(**kw) == _lib.ERR_ARG, name
        buf = C.create_string_buffer(512)
        rec._L.rsrec_last_error(rec._h, buf, 512)
        assert b"rsrec_chebyshev_bloch_map" in buf.value, name
    assert call(sources=()) == 0
    out_g[:] = 0; out_a[:] = 0
    assert call() == 0 and np.array_equal(out_g, good_g) and np.array_equal(out_a, good_a)      # the handle still works
    rec.close()


def test_a_window_too_narrow_diverges():
    rec, dims, H, a, b, lld, cr, cell = small_case(False, None)
    k, ene, w, dense, _ = small_reference(False)
    good_window = rec.en.energy_min, rec.en.energy_max
    rec.en.energy_min, rec.en.energy_max = -0.3, 0.3
    with pytest.raises(_lib.RsrecError) as ei:
        rec.bloch_map([1], k[:, :3], cr, energies=[0.0], cell=cell)
    assert ei.value.code == _lib.ERR_DIVERGED
    rec.en.energy_min, rec.en.energy_max = good_window
    g_k, _ = rec.bloch_map(SOURCES, k, cr, weights=w, cell=cell)
    rec.close()
    assert worst(g_k, dense) <= RTOL                             # the handle still works


def test_depth_and_size():
    """22^3, matrix-core set, lld 50, source 4711, a 64 x 64 commensurate plane (4 096 k-points in 16 chunks), two energies: a_k against
    the weights applied to T_n(H~(k)).  The plane's integer triples repeat modulo 22, so the oracle runs on its 484 distinct points."""
    dims, lld, src, emin, emax = (22, 22, 22), 50, 4711, -3.0, 1.8
    p = supercell_problem(dims)
    cr, cell = supercell_positions(dims), supercell_cell(dims)
    i, j = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    m = np.stack([i.ravel(), j.ravel(), np.zeros(4096, int)], axis=1)
    k = commensurate_k(dims, m)
    a, b = chebyshev_scaling(emin, emax)
    ene = [-1.1, 0.4]
    w = green_weights(2 * lld + 2, a, b, ene)
    uniq, inv = np.unique(m % 22, axis=0, return_inverse=True)
    assert len(uniq) == 484
    g_u = weighted_moments(bloch_hamiltonian_moments(stencil_column(p, src), a, b, src, lld, cr, cell, commensurate_k(dims, uniq)), w)
    ref = diag_of(g_u)[:, :, np.ravel(inv)]                      # (18, 2, 4096)
    rec = make_rec(p, lld, emin, emax, 2)
    none, a_k = rec.bloch_map([src], k, cr, energies=ene, cell=cell, blocks=False)
    t = rec.timing()
    rec.close()
    assert none is None and a_k.shape == (18, 2, 4096, 1, 1)
    err = np.abs(a_k[..., 0, 0] - ref).max() / np.abs(ref).max()
    print("22^3 lld 50, 4096 k: %.2e of max|a_k| = %.3f; accumulation %.1f ms, phases %.1f ms, final sums %.1f ms of %.1f ms"
          % (err, np.abs(ref).max(), t["map_accum_ms"], t["map_phase_ms"], t["map_final_ms"], t["total_ms"]))
    assert err <= RTOL and a_k.min() >= -RTOL * np.abs(ref).max()    # (the Jackson kernel is positive: so are the orbital weights of the whole cell)
