"""The weight tables of the single-shot Kubo call (rslmtoasa_amd.recursion.kubo_bastin_weights, kubo_greenwood_weights) on the CPU:
contracted in numpy with the compiled reference's own moments they give the reference's integrand, and the Greenwood columns are a
normalised delta function with the Jackson kernel's known first-moment shift.  No GPU."""
import numpy as np
import pytest

import cond_reference as R
from helpers import load_golden
from rslmtoasa_amd.recursion import chebyshev_scaling, kubo_bastin_weights, kubo_greenwood_weights

DIAG = np.arange(18)


def window(z):
    """energy_min / energy_max whose Chebyshev scaling is the fixture's a, b (chebyshev_scaling inverted)."""
    a, b = float(z["acheb"]), float(z["bcheb"])
    half = a * float(np.float32(2) - np.float32(0.3)) / 2
    return b - half, b + half


def edge_energies(emin, emax, n=8):
    """n energies inside the window, the first and the last within 2 % of its edges"""
    de = emax - emin
    return np.concatenate([[emin + 0.015 * de], np.linspace(emin + 0.13 * de, emax - 0.21 * de, n - 2), [emax - 0.012 * de]])


@pytest.mark.parametrize("name", ["fccPt_kubo", "fccPt_kubo_hoh", "fccPt_kubo_random"])
def test_bastin_columns_reproduce_the_reference_integrand(name):
    z = load_golden(name)
    emin, emax = window(z)
    ene = edge_energies(emin, emax)
    assert (ene[0] - emin) < 0.02 * (emax - emin) and (emax - ene[-1]) < 0.02 * (emax - emin)
    mu = np.asarray(z["mu_nm"])
    d = mu[DIAG, DIAG]                                              # (18, n, m, v)
    L = d.shape[1]
    wl, wr = kubo_bastin_weights(ene, L, emin, emax)
    assert wl.shape == wr.shape == (L, 16) and wl.flags.f_contiguous and wr.flags.f_contiguous
    s = np.einsum("me,ne,lnmv->lev", wl, wr, d)                     # s(l, e, v) = sum_{n,m} wl(m, e) wr(n, e) mu(l, l, n, m, v)
    got = s[:, 0::2] + s[:, 1::2]
    ref = R.integrand_factorised(mu, ene, emin, emax)
    mag = np.einsum("me,ne,lnmv->lev", np.abs(wl), np.abs(wr), np.abs(d))
    mag = mag[:, 0::2] + mag[:, 1::2]
    ratio = np.abs(got - ref) / mag
    print(name, "worst |dev| / magnitude sum: %.2e" % ratio.max())
    assert np.all(np.abs(got - ref) <= 1e-12 * mag), (name, float(ratio.max()))


def jackson(n_terms):
    n = np.arange(n_terms, dtype=np.float64)
    th = np.pi * n / (n_terms + 1.0)
    return ((n_terms - n + 1.0) * np.cos(th) + np.sin(th) / np.tan(np.pi / (n_terms + 1.0))) / (n_terms + 1.0)


@pytest.mark.parametrize("cond_ll", [1, 2, 9])
def test_greenwood_columns_are_a_normalised_delta(cond_ll):
    """delta_K(E, E') = sum_n d(n, E) T_{n-1}(x') as a function of the energy E the column belongs to.  With dE = a dx and
    d = F(x) / (a sqrt(1 - x^2)), the integral over E is  int F(x) / sqrt(1 - x^2) dx  with F a polynomial of degree < cond_ll, which
    Gauss-Chebyshev quadrature with K = 4 cond_ll nodes x_k = cos(pi (k + 1/2) / K) integrates exactly:  (pi / K) sum_k F(x_k).
    Orthogonality (int T_n T_m / (pi sqrt(1 - x^2)) dx = delta_nm (1 + delta_n0) / 2) leaves
      int T_k(x) delta_K dE = g_k T_k(x')  for every k < cond_ll  (and 0 for cond_ll <= k < 3 cond_ll, which the quadrature still takes),
    g the Jackson factors of cond_ll terms, which holds every row of the table.  In particular
      int delta_K dE = g_0 T_0(x') = 1        and        int E delta_K dE = b + a g_1 x' = E' - a (1 - g_1) x':
    the kernel pulls the first moment towards the band centre by a (1 - g_1) x' (all of it at cond_ll = 1, where the expansion is the
    constant term alone)."""
    emin, emax = -0.9, 0.7
    a, b = chebyshev_scaling(emin, emax)
    K = 4 * cond_ll
    xk = np.cos(np.pi * (np.arange(K) + 0.5) / K)                   # (beyond the window |x| < 0.85, inside the axis |x| < 1)
    g = jackson(cond_ll)
    assert abs(g[0] - 1.0) <= 1e-15 and np.all(np.diff(g) < 0) and g[-1] > 0      # the Jackson factors fall from 1 and stay positive
    g1 = g[1] if cond_ll > 1 else 0.0
    cols = []
    for i0 in range(0, K, 16):
        wl, wr = kubo_greenwood_weights(b + a * xk[i0:i0 + 16], cond_ll, emin, emax)
        assert np.array_equal(wl, wr) and wl is not wr and np.all(wl.imag == 0)
        cols.append(wl.real)
    d = np.concatenate(cols, axis=1)                                # (cond_ll, K)
    quad = (np.pi / K) * a * np.sqrt(1.0 - xk ** 2)                 # dE weights of the nodes
    for xp in (-0.8, -0.31, 0.0, 0.47, 0.84):
        t = np.cos(np.arange(cond_ll) * np.arccos(xp))
        delta = t @ d                                               # delta_K(E_k, E')
        assert abs(np.sum(quad * delta) - 1.0) <= 1e-12
        first = np.sum(quad * delta * (a * xk + b))
        assert abs(first - (b + a * g1 * xp)) <= 1e-12 * max(1.0, abs(b) + a)
        assert abs((first - (a * xp + b)) + a * (1.0 - g1) * xp) <= 1e-12 * max(1.0, abs(b) + a)
        for k in range(3 * cond_ll):                                # degree k + cond_ll - 1 < 2 K: exact
            got = np.sum(quad * delta * np.cos(k * np.arccos(xk)))
            want = g[k] * np.cos(k * np.arccos(xp)) if k < cond_ll else 0.0
            assert abs(got - want) <= 1e-12, (k, got, want)


def test_value_errors():
    emin, emax = -0.8, 0.6
    inside = np.linspace(-0.5, 0.4, 17)
    for fn, nmax in ((kubo_bastin_weights, 8), (kubo_greenwood_weights, 16)):
        wl, wr = fn(inside[:nmax], 5, emin, emax)
        assert wl.shape[0] == 5 and wl.shape == wr.shape
        with pytest.raises(ValueError):
            fn(inside[:nmax + 1], 5, emin, emax)
    for bad in (emin, emax, emin - 0.1, emax + 0.3):                # Bastin: the reference's window, open
        with pytest.raises(ValueError):
            kubo_bastin_weights([0.0, bad], 5, emin, emax)
    a, b = chebyshev_scaling(emin, emax)
    for bad in (b - a, b + a, b + 1.01 * a):                        # Greenwood: the Chebyshev axis |x| < 1, where the delta function is finite
        with pytest.raises(ValueError):
            kubo_greenwood_weights([0.0, bad], 5, emin, emax)
