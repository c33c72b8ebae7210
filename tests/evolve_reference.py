"""Dense numpy restatement of the wave-packet propagation (rsrec_chebyshev_evolve).  Not a test module.

``dense_operator`` builds a (type, slot) operator as ``pair_direct_reference.dense_h`` builds H, the way the Kubo calls apply v_b / vo_b:
rows of bulk atoms only, and with hoh  V psi = v psi - sum_{slot >= 2} vo_slot (h_bulk psi)_nbr  (velo_hoh_vec_matmul).  ``step`` is one
time step of the recurrence
    psi' = sum_n w_n p_n,  p_n = T_n(H~) psi;    chi' = sum_n w_n g_n,  g_0 = chi,  g_1 = H~ g_0 + D p_0 / a,
    g_{n+1} = 2 H~ g_n - g_{n-1} + 2 D p_n / a,
``evolve`` the whole call on vectors (18 kk, 18) whose block j is rows 18 j .. 18 j + 17, with the magnitude sums the GPU tests judge
rounding by: the same recurrences on |H~|, |D|, |w| and the magnitudes of the state with plus signs, propagated through the steps.  ``exact_step`` gives
U = exp(-i H tau) and the Frechet derivative of exp(-i H tau) in direction D from an eigen-decomposition (Hermitian H only)."""
import numpy as np

from helpers import random_problem
from lattice_seed_reference import placed_coefficients
from pair_direct_reference import _stencil

KK_ODD = 75


def dense_operator(p, v, vo=None):
    """(18 kk, 18 kk): the operator with per-type blocks v(:, :, slot, type) (and vo with hoh) of problem dict ``p``, as the Kubo calls apply
    it.  Rows on the first ``nmax`` atoms are zero."""
    nn, iz, nmax = np.asarray(p["nn"]), np.asarray(p["iz"]), int(p.get("nmax", 0))
    bulk = np.ones(18 * nn.shape[0])
    bulk[:18 * nmax] = 0.0
    V = _stencil(nn, iz, 0, np.asarray(v), None) * bulk[:, None]
    if p.get("hoh"):
        vo = np.array(vo, np.complex128)
        vo[:, :, 0] = 0.0                                                  # (the on-site vo term is commented out in the reference)
        hb = _stencil(nn, iz, 0, p["ee"], None) * bulk[:, None]
        V = V - (_stencil(nn, iz, 0, vo, None) * bulk[:, None]) @ hb
    return V


def ragged_problem(hoh):
    """the operator kubo_cases.ragged_case builds and its v_a, v_b (vo_a, vo_b): the first draws of its generator"""
    rng = np.random.default_rng(4242 + int(hoh))
    p = random_problem(rng, KK_ODD, 5, 2, 0, hoh, False)
    if hoh:
        p["eeo"] = np.asfortranarray(p["eeo"] * 0.1)

    def vel():
        return np.asfortranarray((rng.standard_normal((18, 18, 5, 2)) + 1j * rng.standard_normal((18, 18, 5, 2))) * 0.2)
    v_a, v_b = vel(), vel()
    vo_a, vo_b = (vel(), vel()) if hoh else (None, None)
    coefs = np.exp(2j * np.pi * rng.random((3, KK_ODD))) / np.sqrt(KK_ODD)
    seeds = np.tile(np.arange(1, KK_ODD + 1, dtype=np.int32), (3, 1))
    return p, (v_a, v_b, vo_a, vo_b), seeds, coefs


def seed_vector(kk, seeds, coefs):
    """(18 kk, 18): block j = c_j 1 of one vector's placed coefficients"""
    return np.kron(placed_coefficients(kk, seeds, coefs)[:, None], np.eye(18))


def step(Ht, Ds, w, psi, chi, sign=-1.0):
    """one step with H~ = ``Ht`` and D / a = ``Ds``: (psi', chi').  sign = +1 with |H~|, |D / a|, |w| and the magnitudes of the state:
    every product and sum of the step with absolute values and plus signs, the magnitude sums rounding is judged by."""
    p0, g0 = psi, chi
    p1, g1 = Ht @ p0, Ht @ g0 + Ds @ p0
    ps, cs = w[0] * p0 + w[1] * p1, w[0] * g0 + w[1] * g1
    for n in range(2, len(w)):
        p2, g2 = 2.0 * (Ht @ p1) + sign * p0, 2.0 * (Ht @ g1) + sign * g0 + 2.0 * (Ds @ p1)
        ps, cs = ps + w[n] * p2, cs + w[n] * g2
        p0, p1, g0, g1 = p1, p2, g1, g2
    return ps, cs


def _chain_grams(Ht, x, mom, sign):
    """x_v^H T_n(H~) x_v for n = 0 .. mom - 1 and every vector v (18 columns each) of x (sign = -1), or the same sums of magnitudes
    (sign = +1: T_{n+1} = 2 |H~| T_n + T_{n-1}): (18, 18, mom, nvec)"""
    nvec = x.shape[1] // 18
    out = np.zeros((18, 18, mom, nvec), np.complex128)
    q0 = x
    for n in range(mom):
        if n == 1:
            q1 = Ht @ q0
        elif n >= 2:
            q0, q1 = q1, 2.0 * (Ht @ q1) + sign * q0
        q = q0 if n == 0 else q1
        for v in range(nvec):
            out[:, :, n, v] = x[:, 18 * v:18 * v + 18].conj().T @ q[:, 18 * v:18 * v + 18]
    return out


def evolve(H, Dm, a, b, seeds, coefs, w, nt, stride, mom):
    """The call restated: a dict with ``ret`` (18,18,nt,nvec), ``m0_full`` (18,18,mom,nvec), ``m_full`` (18,18,mom,nt,nvec), and under
    ``ret_mag``, ``m0_mag``, ``m_mag`` the magnitude sums of every element.  The vectors advance side by side, 18 columns each."""
    kk = H.shape[0] // 18
    seeds, coefs = np.asarray(seeds).reshape(len(seeds), -1), np.asarray(coefs).reshape(len(seeds), -1)
    nvec = len(seeds)
    w = np.asarray(w, np.complex128).ravel()
    Ht, Ds = (H - b * np.eye(H.shape[0])) / a, Dm / a
    Ha, Da, wa = np.abs(Ht), np.abs(Ds), np.abs(w)
    out = {k: np.zeros((18, 18, nt, nvec), np.complex128, order="F") for k in ("ret", "ret_mag")}
    out.update({k: np.zeros((18, 18, mom, nvec), np.complex128, order="F") for k in ("m0_full", "m0_mag")})
    out.update({k: np.zeros((18, 18, mom, nt, nvec), np.complex128, order="F") for k in ("m_full", "m_mag")})
    c = [placed_coefficients(kk, seeds[v], coefs[v]) for v in range(nvec)]
    psi = np.hstack([seed_vector(kk, seeds[v], coefs[v]) for v in range(nvec)])
    chi = np.zeros_like(psi)
    pm, cm = np.abs(psi), np.abs(chi)
    if mom:
        out["m0_full"][...] = _chain_grams(Ht, psi, mom, -1.0)
        out["m0_mag"][...] = _chain_grams(Ha, pm, mom, 1.0)
    for s in range(nt):
        for _ in range(stride):
            psi, chi = step(Ht, Ds, w, psi, chi)
            pm, cm = step(Ha, Da, wa, pm, cm, 1.0)
        for v in range(nvec):
            out["ret"][:, :, s, v] = np.einsum("j,jab->ab", np.conj(c[v]), psi[:, 18 * v:18 * v + 18].reshape(kk, 18, 18))
            out["ret_mag"][:, :, s, v] = np.einsum("j,jab->ab", np.abs(c[v]), pm[:, 18 * v:18 * v + 18].reshape(kk, 18, 18))
        if mom:
            out["m_full"][:, :, :, s] = _chain_grams(Ht, chi, mom, -1.0)
            out["m_mag"][:, :, :, s] = _chain_grams(Ha, cm, mom, 1.0)
    return out


def exact_step(H, Dm, tau):
    """(U, L): U = exp(-i H tau) and L = the Frechet derivative of exp(-i H tau) in direction Dm, by divided differences in the
    eigenbasis of the Hermitian H:  L = V [(V^H Dm V) o Phi] V^H,  Phi_ij = (f_i - f_j) / (e_i - e_j),  Phi_ii = -i tau f_i."""
    e, V = np.linalg.eigh(H)
    f = np.exp(-1j * e * tau)
    de = e[:, None] - e[None, :]
    close = np.abs(de) < 1e-9 * max(1.0, np.abs(e).max())
    phi = np.where(close, -1j * tau * 0.5 * (f[:, None] + f[None, :]), (f[:, None] - f[None, :]) / np.where(close, 1.0, de))
    return (V * f[None, :]) @ V.conj().T, V @ ((V.conj().T @ Dm @ V) * phi) @ V.conj().T
