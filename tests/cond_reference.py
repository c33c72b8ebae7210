"""numpy restatement of the reference's conductivity integrand (conductivity.f90:158-268): calculate_gamma_nm as it is written
(the (nE, L, L) array Gamma), the contraction with the orbital diagonals of mu_nm_stochastic, and the factorised form the GPU
kernel computes (rslmtoasa_amd/csrc/kernels_cond.hpp), which needs no array of size nE L^2.

The reference's single-precision quirks are kept: lorentz_kernel forms (real(ll) - 1)/real(bign) and 1 - that in REAL(4)
(math.f90:1664-1676); `2 - 0.3` is a default-real expression (conductivity.f90:179, :254); weights(1) = 0.5 (:194); T_n comes
from the three-term recurrence (:203-207) and c_n from the complex exponential of (n - 1) theta (:197-200)."""
import numpy as np

LAMBDA = 6.0


def scaling(energy_min, energy_max):
    a = (energy_max - energy_min) / float(np.float32(2) - np.float32(0.3))
    b = (energy_max + energy_min) / 2
    return a, b


def factor(energy_min, energy_max):
    de = energy_max - energy_min
    return 16 / (np.pi * de ** 2)


def kernel_weights(L):
    """g_kernel(n) * weights(n), n = 1..L."""
    ll = np.arange(1, L + 1, dtype=np.float32)
    t = np.float32(1) - (ll - np.float32(1)) / np.float32(L)          # REAL(4) throughout
    g = np.sinh(LAMBDA * t.astype(np.float64)) / np.sinh(LAMBDA)
    w = np.ones(L)
    w[0] = 0.5
    return g, w


def energy_mesh(energy_min, energy_max, channels_ldos):
    """energy%ene (energy.f90:201-207): channels_ldos + 10 points from energy_min in steps of edel."""
    edel = (energy_max - energy_min) / channels_ldos
    return energy_min + edel * np.arange(channels_ldos + 10)


def basis(ene, energy_min, energy_max, L):
    a, b = scaling(energy_min, energy_max)
    x = (ene - b) / a
    acos_x, s = np.arccos(x), np.sqrt(1.0 - x ** 2)
    n = np.arange(L, dtype=np.float64)
    cn = (x[:, None] - 1j * n[None, :] * s[:, None]) * np.exp(1j * n[None, :] * acos_x[:, None])
    cm = (x[:, None] + 1j * n[None, :] * s[:, None]) * np.exp(-1j * n[None, :] * acos_x[:, None])
    T = np.empty((x.size, L))
    T[:, 0] = 1.0
    if L > 1:
        T[:, 1] = x
    for k in range(2, L):
        T[:, k] = 2.0 * x * T[:, k - 1] - T[:, k - 2]
    return x, cn, cm, T


def gamma_nm(ene, energy_min, energy_max, L):
    """calculate_gamma_nm (:158-225) as written: complex (nE, L, L), Gamma(i, n, m)."""
    x, cn, cm, T = basis(ene, energy_min, energy_max, L)
    g, w = kernel_weights(L)
    G = cn[:, :, None] * T[:, None, :] + cm[:, None, :] * T[:, :, None]
    G = G / ((1.0 - x ** 2) ** 2)[:, None, None]
    G = G * g[None, :, None] * g[None, None, :] * w[None, :, None] * w[None, None, :]
    return G


def diagonals(mu_nm):
    """mu(l, l, n, m, v) -> (18, L, L, nvec)."""
    l = np.arange(18)
    return mu_nm[l, l]


def integrand_direct(G, mu_nm, energy_min, energy_max):
    """integrand_at(l, l, i, v) of calculate_conductivity_tensor (:259-281), factor applied: complex (18, nE, nvec)."""
    d = diagonals(mu_nm)
    return factor(energy_min, energy_max) * np.einsum("inm,lnmv->liv", G, d)


def integrand_factorised(mu_nm, ene, energy_min, energy_max):
    """The same sum without Gamma (kernels_cond.hpp): with A = w c_n, B = w T_n, M = mu(l, l, :, :, v), S = M + M^T, D = M - M^T,
    integrand = factor / (1 - x^2)^2 sum_n [Re A (B S^T) + i Im A (B D^T)]."""
    return integrand_from_diagonals(diagonals(mu_nm), ene, energy_min, energy_max)


def integrand_from_diagonals(d, ene, energy_min, energy_max):
    """integrand_factorised on the orbital diagonals d(l, n, m, v) alone: complex (18, nE, nvec)."""
    L, nvec = d.shape[1], d.shape[3]
    x, cn, cm, T = basis(np.asarray(ene, np.float64), energy_min, energy_max, L)
    g, w = kernel_weights(L)
    A, B = cn * (g * w), T * (g * w)
    out = np.empty((18, x.size, nvec), np.complex128)
    for v in range(nvec):
        M = d[:, :, :, v]                                          # (l, n, m)
        S, D = M + M.transpose(0, 2, 1), M - M.transpose(0, 2, 1)
        BS = np.matmul(B.astype(np.complex128), S.transpose(0, 2, 1))   # (l, i, n) = sum_m B(i, m) S(n, m)
        BD = np.matmul(B.astype(np.complex128), D.transpose(0, 2, 1))
        out[:, :, v] = (A.real[None] * BS).sum(axis=2) + 1j * (A.imag[None] * BD).sum(axis=2)
    return out * (factor(energy_min, energy_max) / (1.0 - x ** 2) ** 2)[None, :, None]


def fort123(integrand, ene, energy_min, energy_max, fermi):
    """The columns of fort.123 (:301): energy - fermi, Re and Im of the integrand summed over orbitals and vectors."""
    a, b = scaling(energy_min, energy_max)
    x = (ene - b) / a
    tot = integrand.sum(axis=(0, 2))
    return np.stack([(a * x + b) - fermi, tot.real, tot.imag], axis=1)
