"""The numpy restatement of the damping traces (damping_reference.py) against explicit formulas, on the CPU."""
import numpy as np

from damping_reference import damping_rows, damping_traces, gij_gji, total_damping


def rnd(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def test_trace_identity_against_the_explicit_triple_product():
    """Tr(X_k Y_l) = sum_ab X_k(a,b) Y_l(b,a) (the sum the kernel runs) is the trace of the reference's temp3, element by element."""
    rng = np.random.default_rng(3)
    gij, gji = rnd(rng, 4, 18, 18), rnd(rng, 4, 18, 18)
    ti, tj = rnd(rng, 18, 18, 3), rnd(rng, 18, 18, 3)
    re, im = damping_traces(gij, gji, ti, tj)
    for nv in range(4):
        Aij, Aji = gij[nv] - gji[nv].conj().T, gji[nv] - gij[nv].conj().T
        for k in range(3):
            for l in range(3):
                X, Y = ti[:, :, k] @ Aij, tj[:, :, l].conj().T @ Aji
                s = 0.0
                for a in range(18):
                    for b in range(18):
                        s += X[a, b] * Y[b, a]
                explicit = sum(ti[a, c, k] * Aij[c, b] * np.conj(tj[d, b, l]) * Aji[d, a]
                               for a in range(18) for b in range(18) for c in range(18) for d in range(18)) if (nv, k, l) == (0, 1, 2) else s
                m = 3 * k + l
                scale = np.abs(X).max() * np.abs(Y).max() * 18
                assert abs(re[m, nv] + 1j * im[m, nv] - s) <= 1e-13 * scale
                assert abs(s - explicit) <= 1e-12 * scale


def test_row_order_is_l_fastest():
    rng = np.random.default_rng(4)
    gij, gji = rnd(rng, 1, 18, 18), rnd(rng, 1, 18, 18)
    ti, tj = np.zeros((18, 18, 3), complex), np.zeros((18, 18, 3), complex)
    ti[:, :, 1] = rnd(rng, 18, 18)          # only k = 2 and l = 3 contribute: row m = 3 * 1 + 2
    tj[:, :, 2] = rnd(rng, 18, 18)
    re, im = damping_traces(gij, gji, ti, tj)
    live = np.abs(re[:, 0]) + np.abs(im[:, 0]) > 0
    assert list(np.nonzero(live)[0]) == [5]


def test_assembly_of_gij_and_gji_from_the_chains():
    """i == j: gij = gji = g0 of chain 1; i /= j: (g1 - g2 +- (g3 - g4) / i) / 2, on a small hand-made g0."""
    g0 = np.zeros((18, 18, 2, 4), complex)
    for c in range(4):
        for e in range(2):
            g0[:, :, e, c] = (c + 1) * np.arange(324).reshape(18, 18) * (1 + 0.5j * e) + 1j * (c == 2) - 3.0 * (c == 3)
    gij, gji = gij_gji(g0, True)
    for e in range(2):
        assert np.allclose(gij[e], g0[:, :, e, 0], rtol=0, atol=1e-12) and np.allclose(gji[e], g0[:, :, e, 0], rtol=0, atol=1e-12)
    gij, gji = gij_gji(g0, False)
    for e in range(2):
        d = g0[:, :, e, 0] - g0[:, :, e, 1]
        s = (g0[:, :, e, 2] - g0[:, :, e, 3]) / 1j
        assert np.allclose(gij[e], 0.5 * (d + s), rtol=0, atol=1e-11) and np.allclose(gji[e], 0.5 * (d - s), rtol=0, atol=1e-11)
    # chains 2..4 are not read for an i == j pair
    g1 = g0.copy()
    g1[..., 1:] = 7.0
    tm = rnd(np.random.default_rng(5), 18, 18, 3, 2)
    assert np.array_equal(damping_rows(g0, True, tm), damping_rows(g1, True, tm))


def test_same_pair_with_hermitian_g_has_no_damping():
    """A = g - g^H vanishes for a Hermitian g: every trace of an i == j pair is zero."""
    rng = np.random.default_rng(6)
    h = rnd(rng, 18, 18)
    g0 = np.zeros((18, 18, 1, 4), complex)
    g0[:, :, 0, 0] = h + h.conj().T
    assert np.abs(damping_rows(g0, True, rnd(rng, 18, 18, 3, 2))).max() < 1e-12


def test_total_is_the_ordered_sum_of_the_real_rows():
    rng = np.random.default_rng(8)
    rows = [rng.standard_normal((18, 5)) for _ in range(4)]
    t = total_damping(rows)
    assert np.array_equal(t, ((rows[0][:9] + rows[1][:9]) + rows[2][:9]) + rows[3][:9])
