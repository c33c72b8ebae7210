"""numpy restatement of the optical conductivity rsrec_kubo_optical computes from the orbital-diagonal Kubo moments (include/rsrec.h,
rslmtoasa_amd/csrc/kernels_optical.hpp).  With x_i = (ene_i - b)/a on a uniform mesh of step Delta (a, b: cond_reference.scaling),
w_n = g_n weights_n (cond_reference.kernel_weights) and T from the three-term recurrence:

    D(i,n)       = 2 w_n T_{n-1}(x_i) / (pi sqrt(1 - x_i^2)),  n = 1..L;  a row with |x_i| >= 1 is zero
    J_{l,s}(i,j) = sum_{n,m} D(i,n) mu(l,n,m,s) D(j,m)
    opt(l,k,f,s) = (pi / a^2) (1/k) sum_{i=0}^{nen-1-k} [F_f(x_i) - F_f(x_{i+k})] J_{l,s}(i, i+k),     k = 1..nw  (omega_k = k Delta)
    F_f(x)       = 1 / (exp((x - x_F,f)/kT) + 1),  x_F,f = (fermi_f - b)/a,  kT = 0.633362019e-5 T + 1e-15 on the scaled axis

``optical_dense`` follows these lines literally; ``optical_factorised`` computes the same numbers the way the kernels do: stage 1
P = D mu per orbital, stage 2 in tiles of 64 x 32 energies of which only those with a pair i < j <= i + nw and a non-zero weight
are formed, the tile's diagonals summed per Fermi level, and the tiles of a diagonal added in ascending tile order.
``temperature`` is in K on the unscaled axis, as Conductivity.optical takes it: the weights are formed with T / a."""
import numpy as np

import cond_reference as R

TILE_I, TILE_J = 64, 32


def scaled_axis(ene, energy_min, energy_max):
    a, b = R.scaling(energy_min, energy_max)
    return (np.asarray(ene, np.float64) - b) / a, a, b


def basis_table(ene, energy_min, energy_max, L):
    """D(i, n), n = 0-based order: real (nen, L)."""
    x, _, _ = scaled_axis(ene, energy_min, energy_max)
    g, wt = R.kernel_weights(L)
    w = g * wt
    inside = np.abs(x) < 1.0
    xs = np.where(inside, x, 0.0)
    T = np.empty((x.size, L))
    T[:, 0] = 1.0
    if L > 1:
        T[:, 1] = xs
    for n in range(2, L):
        T[:, n] = 2.0 * xs * T[:, n - 1] - T[:, n - 2]
    pre = 2.0 / (np.pi * np.sqrt(1.0 - xs ** 2))
    return np.where(inside[:, None], pre[:, None] * w[None, :] * T, 0.0)


def fermi_table(ene, energy_min, energy_max, fermi, temperature=0.0):
    """F_f(x_i): real (nfermi, nen)."""
    x, a, b = scaled_axis(ene, energy_min, energy_max)
    xf = (np.atleast_1d(np.asarray(fermi, np.float64)) - b) / a
    kt = 0.633362019e-5 * (temperature / a) + 1.0e-15
    with np.errstate(over="ignore"):
        return 1.0 / (np.exp((x[None, :] - xf[:, None]) / kt) + 1.0)


def density(D, M):
    """J(i, j) = sum_{n,m} D(i,n) M(n,m) D(j,m) for M (..., L, L): complex (..., nen, nen)."""
    return np.matmul(np.matmul(D.astype(np.complex128), M), D.T.astype(np.complex128))


def frequency_sum(J, F, nw, a):
    """opt(k, f) of one density J (nen, nen) and the Fermi table F (nfermi, nen): complex (nw, nfermi).  Terms of weight zero are left out."""
    nen = J.shape[0]
    out = np.zeros((nw, F.shape[0]), np.complex128)
    for k in range(1, nw + 1):
        diag = np.diagonal(J, offset=k)                              # J(i, i + k), i = 0 .. nen - 1 - k
        for f in range(F.shape[0]):
            wgt = F[f, :nen - k] - F[f, k:]
            on = wgt != 0.0
            out[k - 1, f] = np.pi / a ** 2 / k * np.sum(wgt[on] * diag[on])
    return out


def optical_dense(d, ene, energy_min, energy_max, fermi, nw=None, temperature=0.0):
    """The formula as it stands, on the orbital diagonals d(l, n, m, s): complex (18, nw, nfermi, nset)."""
    d = np.asarray(d, np.complex128)
    ene = np.asarray(ene, np.float64)
    nw = ene.size - 1 if nw is None else nw
    L, nset = d.shape[1], d.shape[3]
    _, a, _ = scaled_axis(ene, energy_min, energy_max)
    D = basis_table(ene, energy_min, energy_max, L)
    F = fermi_table(ene, energy_min, energy_max, fermi, temperature)
    out = np.empty((18, nw, F.shape[0], nset), np.complex128)
    for s in range(nset):
        for l in range(18):
            out[l, :, :, s] = frequency_sum(density(D, d[l, :, :, s]), F, nw, a)
    return out


def tile_is_live(i0, j0, nen, nw, F):
    """A tile of rows i0 .. i0 + 63 and columns j0 .. j0 + 31 is formed when it holds a pair 1 <= j - i <= nw with j < nen and, for some
    Fermi level, its rows' and columns' weights are not all one value."""
    jmax = min(j0 + TILE_J, nen) - 1
    if jmax <= i0 or j0 - min(i0 + TILE_I - 1, nen - 1) > nw:
        return False
    v = np.concatenate([F[:, i0:min(i0 + TILE_I, nen)], F[:, j0:jmax + 1]], axis=1)
    return bool((v != v[:, :1]).any())


def optical_factorised(d, ene, energy_min, energy_max, fermi, nw=None, temperature=0.0):
    """The same numbers the way the kernels form them (the module docstring): complex (18, nw, nfermi, nset)."""
    d = np.asarray(d, np.complex128)
    ene = np.asarray(ene, np.float64)
    nen = ene.size
    nw = nen - 1 if nw is None else nw
    L, nset = d.shape[1], d.shape[3]
    _, a, _ = scaled_axis(ene, energy_min, energy_max)
    D = basis_table(ene, energy_min, energy_max, L)
    F = fermi_table(ene, energy_min, energy_max, fermi, temperature)
    nf = F.shape[0]
    ii, jj = np.arange(TILE_I)[:, None], np.arange(TILE_J)[None, :]
    out = np.zeros((18, nw, nf, nset), np.complex128)
    for s in range(nset):
        P = np.matmul(D[None].astype(np.complex128), d[:, :, :, s])           # stage 1: P(l, i, m) = sum_n D(i,n) mu(l,n,m)
        for i0 in range(0, nen, TILE_I):
            for j0 in range(0, nen, TILE_J):
                if not tile_is_live(i0, j0, nen, nw, F):
                    continue
                ni, nj = min(TILE_I, nen - i0), min(TILE_J, nen - j0)
                Jt = np.matmul(P[:, i0:i0 + ni, :], D[j0:j0 + nj, :].T)          # stage 2: (18, ni, nj)
                k = (j0 + jj[:, :nj]) - (i0 + ii[:ni])                           # the diagonal of every element
                ok = (k >= 1) & (k <= nw)
                for f in range(nf):
                    wgt = np.where(ok, F[f, i0:i0 + ni, None] - F[f, None, j0:j0 + nj], 0.0)
                    WJ = wgt[None] * Jt
                    for off in range(1 - ni, nj):                                # the tile's diagonals: column - row = off
                        kk = j0 - i0 + off
                        if 1 <= kk <= nw:
                            out[:, kk - 1, f, s] += np.diagonal(WJ, offset=off, axis1=1, axis2=2).sum(axis=1)
    return out * (np.pi / a ** 2 / np.arange(1, nw + 1))[None, :, None, None]


# (L, nset, nen, nw, nfermi): the smallest shapes that cross the 4-wide k-step, the 16- and 64-wide tiles, a 256-energy block,
# nw < nen - 1 and a long K loop -- shared by tests/test_optical_restatement.py and tests/test_gpu_optical.py
CASES = [(1, 1, 2, 1, 1), (2, 1, 3, 2, 1), (17, 3, 37, 36, 2), (24, 1, 61, 60, 1), (50, 2, 130, 129, 3), (131, 1, 257, 100, 2),
         (500, 1, 300, 299, 1)]
WINDOW = (-0.8, 0.6)


def random_diagonals(L, nset, seed):
    """Random moments with the decay of test_gpu_conductivity.random_diagonals: complex (18, L, L, nset)."""
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    decay = 1.0 / (1.0 + 0.05 * (n[:, None] + n[None, :]))
    return (rng.standard_normal((18, L, L, nset)) + 1j * rng.standard_normal((18, L, L, nset))) * decay[None, :, :, None]


def inner_mesh(nen, energy_min, energy_max):
    """nen uniform energies strictly inside the window (test_gpu_conductivity.mesh for small nen)."""
    return np.linspace(energy_min, energy_max, nen + 2)[1:-1]


def case_fermi(ene, nfermi):
    """Fermi levels of a case: between two mesh points near the middle, then exactly on a mesh point, then near the lower end."""
    nen = ene.size
    levels = [0.5 * (ene[nen // 2 - 1] + ene[nen // 2]) if nen > 2 else 0.5 * (ene[0] + ene[1]), ene[nen // 3], 0.3 * ene[0] + 0.7 * ene[min(2, nen - 1)]]
    return np.array(levels[:nfermi])


def orbital_err(x, ref):
    """Per orbital, relative to the orbital's largest magnitude (test_gpu_conductivity.orbital_err)."""
    return max(np.abs(x[l] - ref[l]).max() / np.abs(ref[l]).max() for l in range(18))
