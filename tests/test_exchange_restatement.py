"""CPU checks of the two identities rsrec_exchange rests on (kernels_exchange.hpp), on the numpy restatement of the reference:
(1) with d_matrix diagonal, Tr(D_i A D_j B) = sum_ab d_i(a) A_ab d_j(b) B_ba reproduces the 9x9 matmul form of every integrand;
(2) at T = 0 and Ef = ene(nv) the Fermi weights are a step, so fort.150's O(nE^2) integrals are a prefix scan."""
import numpy as np

from exchange_reference import PI, combos, d_matrix, integrands, intersite_parts, simpson_f


def rand_pair(rng, nE, same):
    g0 = rng.standard_normal((18, 18, nE, 4)) + 1j * rng.standard_normal((18, 18, nE, 4))
    dpar = np.empty((4, 3, 2))
    dpar[:2] = rng.uniform(-0.3, 0.4, (2, 3, 2))
    dpar[2:] = rng.uniform(0.04, 0.25, (2, 3, 2))
    return g0, dpar


def trace_form(g0, same, dpar, ene):
    """The library's formulation: 42 traces of diagonal-scaled products, combined into the 41 rows."""
    G = intersite_parts(g0, same)
    di = np.diagonal(d_matrix(dpar[:, :, 0], ene), axis1=1, axis2=2)
    dj = np.diagonal(d_matrix(dpar[:, :, 1], ene), axis1=1, axis2=2)

    def T(a, b):
        return np.einsum("ea,eab,eb,eba->e", di, G[a], dj, G[b])

    x = "xyz"
    r = np.zeros((41, len(ene)))
    r[0] = (T("Ginmag", "Gjnmag") - sum(T("Gi" + c, "Gj" + c) for c in x)).imag
    for k, c in enumerate(x):
        r[1 + k] = (T("Ginmag", "Gj" + c) - T("Gi" + c, "Gjnmag")).real
        for l, cl in enumerate(x):
            r[4 + k + 3 * l] = 0.5 * (T("Gi" + c, "Gj" + cl) + T("Gi" + cl, "Gj" + c)).imag
            r[23 + k + 3 * l] = T("G%s0ij" % c, "G%s0ji" % cl).imag
            r[32 + k + 3 * l] = T("G%s1ij" % c, "G%s1ji" % cl).imag
        r[20 + k] = T("G00ij", "G%s1ji" % c).real
        r[17 + k] = T("G01ij", "G%s0ji" % c).real
    r[13] = T("G00ij", "G00ji").imag
    r[15] = T("G01ij", "G01ji").imag
    r[14] = r[23] + r[27] + r[31]
    r[16] = r[32] + r[36] + r[40]
    return r


def test_trace_identity_reproduces_the_matmul_form():
    rng = np.random.default_rng(3)
    ene = np.linspace(-0.6, 0.4, 23)
    for same in (False, True):
        g0, dpar = rand_pair(rng, len(ene), same)
        ref = integrands(g0, same, dpar, ene)
        mine = trace_form(g0, same, dpar, ene)
        assert np.abs(mine - ref).max() <= 1e-12 * np.abs(ref).max()


def prefix_jcum(y, ene, nv1):
    """k_exchange_integrate's cumulative J: triples below Ef summed once, the (at most two) touching Ef added per point."""
    nE = len(y)
    yy = lambda k: y[k] if k < nE else 0.0
    ntrip = (nv1 + 9) // 2
    out, Afull, tfull = np.zeros(nE), 0.0, 0
    for n in range(nE):
        while tfull < ntrip and 2 * (tfull + 1) < n:
            k = 2 * (tfull + 1) - 1
            Afull = Afull + yy(k - 1) + 4.0 * yy(k) + yy(k + 1)
            tfull += 1
        A = Afull
        tt = tfull + 1
        while tt <= ntrip and 2 * tt - 2 <= n:
            k = 2 * tt - 1
            w = lambda i: 1.0 if i < n else (0.5 if i == n else 0.0)
            A = A + yy(k - 1) * w(k - 1) + 4.0 * yy(k) * w(k) + yy(k + 1) * w(k + 1)
            tt += 1
        out[n] = (ene[1] - ene[0]) * A / 3.0
    return out


def test_cumulative_j_is_a_prefix_scan():
    rng = np.random.default_rng(5)
    for channels in (40, 41):
        nv1 = channels + 1 if channels % 2 == 0 else channels
        nE = (nv1 - 1) + 10
        ene = -0.6 + 0.01 * np.arange(nE)
        rows = rng.standard_normal((41, nE))
        y, _ = combos(rows)
        direct = np.array([simpson_f(y[13:14], ene, ef, nv1)[0] for ef in ene])
        scan = prefix_jcum(y[13], ene, nv1)
        assert np.array_equal(direct, scan)
        assert np.isfinite(direct).all() and np.abs(direct).max() > 0
        assert PI == np.float64(3.14159265358979323846)
