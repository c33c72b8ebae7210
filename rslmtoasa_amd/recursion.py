"""Host-side mirror of the reference's ``recursion_mod`` (source/recursion.f90) on top of the C ABI.

Same names, argument meaning and error behaviour as the Fortran type the rest of RS-LMTO-ASA drives
(recursion.f90:41-116): a ``Recursion`` object borrows ``hamiltonian``/``lattice``/``control``/``energy``
objects, exposes ``recur()``, ``recur_b()``, ``chebyshev_recur()``, ``recur_b_ij()``, ``zsqr()`` and fills
``a, b2, a_b, b2_b, mu_n`` with the reference's shapes and index order (arrays are Fortran-ordered numpy
arrays, so ``a_b[l, m, ll, site]`` reads like ``a_b(l+1, m+1, ll+1, site+1)``).

All arithmetic happens in librsrec (HIP kernels); this module only marshals arrays.  The production host
for the reference is the Fortran shim under ``fortran/`` -- this Python mirror exists so the parity tests
and the benchmark read like the reference's own call sites (self.f90:799-806, :829).
"""
import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib


@dataclass
class Control:
    """control%lld, %llsp, %nsp, %recur (control.f90:36-164)."""
    lld: int = 21
    llsp: int = 0
    nsp: int = 2
    recur: str = "block"


@dataclass
class Energy:
    """energy%energy_min / %energy_max (energy.f90:175-207)."""
    energy_min: float = -1.0
    energy_max: float = 1.0


@dataclass
class Lattice:
    """The tables of lattice.f90:138-239 the recursion reads."""
    nn: np.ndarray            # (kk, nncols) int32, 1-based, 0 = absent, column 0 = count
    iz: np.ndarray            # (kk,) int32 1-based type
    irec: np.ndarray          # (nrec,) int32 1-based recursion sites
    nmax: int = 0
    ntype: int = 1
    ijpair: np.ndarray = None  # (njij, 2) atom pairs for recur_b_ij (lattice%ijpair)
    cr: np.ndarray = None      # (3, kk) positions, lattice%cr -- optional locality hint for the engine

    @property
    def kk(self):
        return self.nn.shape[0]

    @property
    def nrec(self):
        return len(self.irec)


@dataclass
class Hamiltonian:
    """hamiltonian%ee, %lsham, %eeo, %enim, %hall, %hallo, %hoh (hamiltonian.f90:51-70)."""
    ee: np.ndarray
    lsham: np.ndarray
    eeo: np.ndarray = None
    enim: np.ndarray = None
    hall: np.ndarray = None
    hallo: np.ndarray = None
    hoh: bool = False
    local_axis: bool = False


def site_partition(rank, nprocs, nsites):
    """get_mpi_variables (mpi.f90:32-58): 1-based inclusive (start_atom, end_atom)."""
    s, e = C.c_int(), C.c_int()
    _lib.lib().rsrec_site_partition(rank, nprocs, nsites, C.byref(s), C.byref(e))
    return s.value, e.value


def chebyshev_scaling(energy_min, energy_max):
    """a, b of chebyshev_recur (recursion.f90:3078-3079).  The literal 0.3 there is default REAL(4)."""
    a = (energy_max - energy_min) / float(np.float32(2) - np.float32(0.3))
    b = (energy_max + energy_min) / 2
    return a, b


def chebyshev_green_weights(energies, lld, energy_min, energy_max):
    """The coefficients ``green%chebyshev_green`` applies to the moments, as the weights ``Recursion.bloch_map`` takes: complex (2 lld + 2, ne),
    w(n, e) = jackson(n) (2 for n > 1) (-i exp(-i (n-1) acos x_e)) / sqrt(a^2 - (E_e - b)^2), x_e = (E_e - b) / a, with the Jackson kernel of
    math.f90:1641-1655 and a, b of ``chebyshev_scaling``.  Raises ValueError for an energy outside the open window (energy_min, energy_max)."""
    ene = np.atleast_1d(np.asarray(energies, np.float64)).ravel()
    if not np.all((ene > energy_min) & (ene < energy_max)):
        raise ValueError("energies must lie inside the open window (%g, %g)" % (energy_min, energy_max))
    a, b = chebyshev_scaling(energy_min, energy_max)
    nm = 2 * lld + 2
    n = np.arange(nm, dtype=np.float64)
    th = np.pi * n / (nm + 1.0)
    kern = ((nm - n + 1.0) * np.cos(th) + np.sin(th) / np.tan(np.pi / (nm + 1.0))) / (nm + 1.0)
    kern[1:] *= 2.0
    phase = -1j * np.exp(-1j * n[:, None] * np.arccos((ene - b) / a)[None, :])
    return np.asfortranarray(kern[:, None] * phase / np.sqrt(a * a - (ene - b) ** 2)[None, :])


def chebyshev_fermi_weights(fermi, kT, lld, energy_min, energy_max, powers=(0, 1, 2), jackson=False):
    """The weights with which ``Recursion.site_map`` gives the occupation matrix and the band moments of every atom: real values as
    complex (2 lld + 2, len(powers)) in Fortran order, column q the Chebyshev coefficients of E^q / (1 + exp((E - fermi) / kT)) in
    x = (E - b) / a, a and b of ``chebyshev_scaling``, so that sum_n w(n, q) T_{n-1}(H~) = H^q f(H) to the accuracy of a degree-(2 lld + 1)
    expansion.  Chebyshev-Gauss quadrature on the N = 2 lld + 2 points x_k = cos(pi (k + 1/2) / N):
    c_n = (2 - delta_n0) / N sum_k F(a x_k + b) cos(n pi (k + 1/2) / N) -- the interpolant through those points.  ``jackson=True`` multiplies
    row n by the Jackson damping g_n of N terms (math.f90:1641-1655), which trades the Gibbs ripples of a cold Fermi function for a
    broadening of about pi a / N."""
    nm = 2 * int(lld) + 2
    a, b = chebyshev_scaling(energy_min, energy_max)
    powers = [int(q) for q in powers]
    k = np.arange(nm, dtype=np.float64)
    theta = np.pi * (k + 0.5) / nm
    ene = a * np.cos(theta) + b
    with np.errstate(over="ignore"):
        fermi_fn = 1.0 / (1.0 + np.exp((ene - fermi) / kT))
    n = np.arange(nm, dtype=np.float64)
    cosines = np.cos(n[:, None] * theta[None, :])                                       # (n, k)
    w = np.empty((nm, len(powers)), np.complex128, order="F")
    for col, q in enumerate(powers):
        c = 2.0 / nm * (cosines @ (ene ** q * fermi_fn))
        c[0] *= 0.5
        w[:, col] = c
    if jackson:
        th = np.pi * n / (nm + 1.0)
        g = ((nm - n + 1.0) * np.cos(th) + np.sin(th) / np.tan(np.pi / (nm + 1.0))) / (nm + 1.0)
        w *= g[:, None]
    return w


def probing_seeds(colour, rng=None):
    """Probing vectors for ``Recursion.site_map`` from a colouring of the atoms: ``colour`` int (kk) with values 0 .. nc - 1.  Returns
    ``(seeds (nc, kk) int32, coefs (nc, kk) complex)``: vector c has coefficient 1 on the atoms of colour c -- or +-1 drawn from ``rng``
    (a numpy Generator) -- and entry 0 (unused) elsewhere.  When same-coloured atoms are further apart than the degree of the polynomial,
    D / cnorm of ``site_map`` is exact (``lattice.supercell_colouring``)."""
    colour = np.asarray(colour)
    if colour.ndim != 1 or colour.size == 0 or colour.min() < 0:
        raise ValueError("colour must be (kk) with values 0 .. nc - 1")
    kk, nc = colour.size, int(colour.max()) + 1
    atoms = np.arange(1, kk + 1, dtype=np.int32)
    sign = np.ones(kk) if rng is None else rng.choice([-1.0, 1.0], kk)
    seeds = np.zeros((nc, kk), np.int32)
    coefs = np.zeros((nc, kk), np.complex128)
    for c in range(nc):
        on = colour == c
        seeds[c, on] = atoms[on]
        coefs[c, on] = sign[on]
    return seeds, coefs


def _scaled_energies(energies, energy_min, energy_max, nmax, who, window=True):
    """(x_e, a) of a weight table: the energies on the Chebyshev axis.  ValueError for more than nmax energies and for one outside the
    open window (energy_min, energy_max), or with window=False outside the open axis |x_e| < 1 (which holds the window)."""
    ene = np.atleast_1d(np.asarray(energies, np.float64)).ravel()
    if ene.size > nmax:
        raise ValueError("%s: at most %d energies per call, got %d" % (who, nmax, ene.size))
    a, b = chebyshev_scaling(energy_min, energy_max)
    x = (ene - b) / a
    if window and not np.all((ene > energy_min) & (ene < energy_max)):
        raise ValueError("%s: energies must lie inside the open window (%g, %g)" % (who, energy_min, energy_max))
    if not np.all(np.abs(x) < 1.0):
        raise ValueError("%s: energies must lie inside (b - a, b + a) = (%g, %g)" % (who, b - abs(a), b + abs(a)))
    return x, a


def _chebyshev_t(x, cond_ll):
    """T_n(x_e), n = 0 .. cond_ll - 1, by the three-term recurrence (conductivity.f90:203-207): real (cond_ll, ne)."""
    t = np.empty((cond_ll, x.size))
    t[0] = 1.0
    if cond_ll > 1:
        t[1] = x
    for k in range(2, cond_ll):
        t[k] = 2.0 * x * t[k - 1] - t[k - 2]
    return t


def kubo_bastin_weights(energies, cond_ll, energy_min, energy_max):
    """The weights with which ``Recursion.kubo_single_shot`` gives the reference's Kubo-Bastin integrand at chosen energies: ``(wl, wr)``,
    complex (cond_ll, 2 nE) in Fortran order.  gamma_nm of calculate_gamma_nm (conductivity.f90:216-218) is a sum of two products,
    gw_n gw_m [c_n T_m + conj(c)_m T_n] / (1 - x^2)^2, so two columns per energy reproduce it -- column 2 i: wr = F gw c_n / (1 - x^2)^2,
    wl = gw T_m; column 2 i + 1: wr = F gw T_n / (1 - x^2)^2, wl = gw conj(c)_m -- and the sum of the two columns of ``s_diag`` is
    integrand_at(l, l, i, v) with the reference's factor F = 16 / (pi (energy_max - energy_min)^2) inside wr.  The reference's quirks are
    kept: the Lorentz kernel gw (lambda = 6) forms (n - 1) / cond_ll and 1 - that in REAL(4) (math.f90:1664-1676), weights(1) = 0.5
    (:194), `2 - 0.3` of the scaling is default real (:179), T_n comes from the recurrence and c_n = (x - i n sqrt(1 - x^2)) exp(i n acos x)
    (:197-200).  Raises ValueError for an energy outside the open window (energy_min, energy_max) and for more than 8 energies (16 columns
    per call)."""
    cond_ll = int(cond_ll)
    x, _ = _scaled_energies(energies, energy_min, energy_max, _lib.KUBO_SHOT_NE_MAX // 2, "kubo_bastin_weights")
    n = np.arange(cond_ll, dtype=np.float64)[:, None]
    acos_x, s = np.arccos(x)[None, :], np.sqrt(1.0 - x ** 2)[None, :]
    cn = (x[None, :] - 1j * n * s) * np.exp(1j * n * acos_x)
    cm = (x[None, :] + 1j * n * s) * np.exp(-1j * n * acos_x)
    t = _chebyshev_t(x, cond_ll)
    step = np.arange(1, cond_ll + 1, dtype=np.float32)
    lor = np.float32(1) - (step - np.float32(1)) / np.float32(cond_ll)                # REAL(4) throughout
    gw = np.sinh(6.0 * lor.astype(np.float64)) / np.sinh(6.0)
    gw[0] *= 0.5
    gw = gw[:, None]
    f = 16.0 / (np.pi * (energy_max - energy_min) ** 2) / ((1.0 - x ** 2) ** 2)[None, :]
    wl = np.empty((cond_ll, 2 * x.size), np.complex128, order="F")
    wr = np.empty((cond_ll, 2 * x.size), np.complex128, order="F")
    wl[:, 0::2], wr[:, 0::2] = gw * t, f * gw * cn
    wl[:, 1::2], wr[:, 1::2] = gw * cm, f * gw * t
    return wl, wr


def kubo_greenwood_weights(energies, cond_ll, energy_min, energy_max):
    """The weights with which ``Recursion.kubo_single_shot`` gives the Kubo-Greenwood trace Tr[v_out delta(E - H) v_b delta(E - H)]:
    ``(wl, wr)`` with wl = wr = d, real values as complex (cond_ll, nE) in Fortran order,
    d(n, e) = jackson_n (2 - delta_{n,1}) T_{n-1}(x_e) / (pi a sqrt(1 - x_e^2)), x_e = (E_e - b) / a, so that
    sum_n d(n, e) T_{n-1}(H~) = delta(E_e - H) broadened by the Jackson kernel of cond_ll terms (math.f90:1641-1655), a and b of
    ``chebyshev_scaling``.  The delta function is finite on the whole Chebyshev axis, so energies beyond the window are taken as long
    as |x_e| < 1.  Raises ValueError for an energy outside (b - a, b + a) and for more than 16 energies."""
    cond_ll = int(cond_ll)
    x, a = _scaled_energies(energies, energy_min, energy_max, _lib.KUBO_SHOT_NE_MAX, "kubo_greenwood_weights", window=False)
    n = np.arange(cond_ll, dtype=np.float64)
    th = np.pi * n / (cond_ll + 1.0)
    kern = ((cond_ll - n + 1.0) * np.cos(th) + np.sin(th) / np.tan(np.pi / (cond_ll + 1.0))) / (cond_ll + 1.0)
    kern[1:] *= 2.0
    d = kern[:, None] * _chebyshev_t(x, cond_ll) / (np.pi * a * np.sqrt(1.0 - x ** 2))[None, :]
    d = np.asfortranarray(d, dtype=np.complex128)
    return d, d.copy(order="F")


def evolution_weights(tau, korder, a, b):
    """The weights of one time step of ``Recursion.evolve``: complex (korder), w_n = the Chebyshev coefficient of order n of
    exp(-i a tau x) times exp(-i b tau), so that sum_n w_n T_n(H~) = exp(-i H tau) with H~ = (H - b) / a, up to the neglected orders
    (``evolution_order``).  A cosine transform at N >= 4 korder Chebyshev nodes x_k = cos(pi (k + 1/2) / N):
    c_n = (2 - delta_n0) / N sum_k exp(-i a tau x_k) cos(n pi (k + 1/2) / N), which equals (2 - delta_n0) (-i)^n J_n(a tau) up to
    the aliased orders 2 N - n and beyond (N also exceeds 2 |a tau| + 64, so those are far below rounding).  The angle
    n (2 k + 1) pi / (2 N) is reduced in integers before the cosine is taken.  numpy only."""
    korder = int(korder)
    if korder < 1:
        raise ValueError("evolution_weights: korder must be at least 1")
    z = float(a) * float(tau)
    if not np.isfinite(z) or not np.isfinite(float(b) * float(tau)):
        raise ValueError("evolution_weights: a tau and b tau must be finite")
    nn = max(4 * korder, 2 * int(np.ceil(abs(z))) + 64)
    k = np.arange(nn, dtype=np.int64)
    # the samples: the phase a tau x_k is tens of radians, so it is formed in numpy's widest real type before it is rounded
    wide = np.longdouble
    phase = wide(a) * wide(tau) * np.cos((2 * k.astype(wide) + 1) * _pi_wide() / (2 * wide(nn)))
    f = np.cos(phase).astype(np.float64) - 1j * np.sin(phase).astype(np.float64)
    c = np.empty(korder, np.complex128)
    for n0 in range(0, korder, 256):                                      # (rows in chunks: the cosine table of 4096 orders is half a GB)
        n = np.arange(n0, min(korder, n0 + 256), dtype=np.int64)
        cosines = np.cos(np.pi * ((n[:, None] * (2 * k + 1)[None, :]) % (4 * nn)) / (2.0 * nn))
        c[n0:n0 + n.size] = (2.0 / nn) * (cosines @ f)
    c[0] *= 0.5
    return c * np.exp(-1j * float(b) * float(tau))


def _pi_wide():
    """pi in numpy's widest real type (4 atan 1 there; the double where there is none wider)"""
    return 4 * np.arctan(np.longdouble(1))


def evolution_order(tau, a, tol=1e-14):
    """The smallest korder for ``evolution_weights(tau, korder, a, b)`` whose first neglected coefficient, and every one behind it,
    is below ``tol`` in magnitude: the coefficients 2 |J_n(a tau)| fall faster than geometrically once n exceeds |a tau|, about
    |a tau| + 40 at 1e-14 for |a tau| of a few tens."""
    z = abs(float(a) * float(tau))
    length = int(np.ceil(z)) + 32
    while True:
        mag = np.abs(evolution_weights(tau, length, a, 0.0))
        over = np.nonzero(mag >= tol)[0]
        if over.size == 0:
            return 2
        if over[-1] + 1 < length:
            return max(2, int(over[-1]) + 1)
        length *= 2


def position_commutator(ee, slot_vec, direction, alat=1.0, eeo_factor=None):
    """The operator D = [X, H] of ``Recursion.evolve`` for the position along ``direction`` (3; normalised here), in the (type, slot)
    form of the velocity operators: d_op(:, :, m, t) = ((r_i - r_j) . dir) alat ee(:, :, m, t) for neighbour slot m of an atom i of
    type t, zero in the on-site slot -- i times the reference's v_a (build_realspace_velocity_operators, hamiltonian.f90:1343-1348).
    ``ee`` (18, 18, nslots, ntype); ``slot_vec`` (nslots, 3) or (nslots, 3, ntype), fewer rows for a stencil with unused slots: r_j - r_i of slot m in units of
    alat (row 0, the atom itself, is ignored), as ``lattice.bcc_supercell`` takes it.  Only differences of positions enter, so a
    periodic cell needs no position operator.  Returns ``d_op``, or with ``eeo_factor`` ``(d_op, do_op)`` for hoh: do_op(:, :, m, t) =
    d_op(:, :, m, t) @ eeo_factor(:, :, m, t), the reference's product with obarm of the neighbour's type (:1356-1358);
    ``eeo_factor`` is (18, 18, nslots, ntype), or one (18, 18) matrix for every slot and type."""
    ee = np.asarray(ee, np.complex128)
    if ee.ndim != 4 or ee.shape[:2] != (18, 18):
        raise ValueError("ee must be (18, 18, nslots, ntype), got %s" % (ee.shape,))
    nslots, ntype = ee.shape[2:]
    sv = np.asarray(slot_vec, np.float64)
    if sv.ndim == 2:
        sv = np.repeat(sv[:, :, None], ntype, axis=2)
    if sv.ndim == 3 and sv.shape[0] < nslots:                             # (slots the stencil does not use: zero blocks)
        sv = np.concatenate([sv, np.zeros((nslots - sv.shape[0],) + sv.shape[1:])], axis=0)
    if sv.shape != (nslots, 3, ntype):
        raise ValueError("slot_vec must be (%d, 3) or (%d, 3, %d), got %s" % (nslots, nslots, ntype, np.shape(slot_vec)))
    d = np.asarray(direction, np.float64).ravel()
    if d.size != 3 or not np.linalg.norm(d) > 0:
        raise ValueError("direction must be a non-zero 3-vector")
    d = d / np.linalg.norm(d)
    dot = -np.einsum("x,mxt->mt", d, sv) * float(alat)                    # (r_i - r_j) . dir
    dot[0] = 0.0
    d_op = np.asfortranarray(ee * dot[None, None])
    if eeo_factor is None:
        return d_op
    ob = np.asarray(eeo_factor, np.complex128)
    if ob.shape == (18, 18):
        ob = np.broadcast_to(ob[:, :, None, None], ee.shape)
    if ob.shape != ee.shape:
        raise ValueError("eeo_factor must be (18, 18) or %s, got %s" % (ee.shape, np.shape(eeo_factor)))
    return d_op, np.asfortranarray(np.einsum("abmt,bcmt->acmt", d_op, ob))


def _fc(a, dtype):
    return np.asfortranarray(np.asarray(a, dtype=dtype))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Recursion:
    """Drop-in counterpart of ``type(recursion)`` (recursion.f90:41-116)."""

    def __init__(self, hamiltonian, lattice, control, energy=None, device=0, rank=0, nprocs=1):
        self.hamiltonian, self.lattice, self.control, self.en = hamiltonian, lattice, control, energy or Energy()
        self.rank, self.nprocs = rank, nprocs
        self._L = _lib.lib()
        self._h = C.c_void_p()
        rc = self._L.rsrec_create(C.byref(self._h), device)
        if rc != 0:
            raise _lib.RsrecError(rc, "rsrec_create failed (no usable gfx950 device? there is no CPU fallback)")
        self.restore_to_default()
        self.update_lattice()
        self.update_hamiltonian()

    # -- lifetime --------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.rsrec_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            buf = C.create_string_buffer(512)
            self._L.rsrec_last_error(self._h, buf, 512)
            # the reference calls g_logger%fatal here (recursion.f90:1942, :2595)
            raise _lib.RsrecError(rc, buf.value.decode(errors="replace"))

    def set_option(self, key, value):
        self._check(self._L.rsrec_set_option(self._h, key.encode(), int(value)))


    def timing(self):
        out = (C.c_double * 25)()
        self._L.rsrec_get_timing(self._h, out, 25)
        keys = ("total_ms", "hop_ms", "hop_launches", "atom_steps", "block_multiplies", "rest_ms", "host_ms", "hop_fuses_a", "hop_mfma_flop", "hop_required_flop",
                "operator_arrays_from_device", "octet_launches", "rotate_ms", "gram_folded_launches", "map_accum_ms", "map_phase_ms", "map_final_ms",
                "shot_accum_ms", "shot_final_ms", "kubo_left_chunks", "kubo_lchunk_planned", "site_accum_ms", "site_out_ms",
                "evolve_pass_ms", "evolve_record_ms")
        return dict(zip(keys, list(out)))

    # -- state (restore_to_default, recursion.f90:3713-3825) --------------------------------------------
    def restore_to_default(self):
        lat, ctl = self.lattice, self.control
        llmax = max(ctl.llsp, ctl.lld)
        nrec = lat.nrec
        njij = 0 if lat.ijpair is None else len(lat.ijpair)
        nsites = nrec if njij == 0 else 4 * njij
        self.a = np.zeros((llmax, 18, nrec, 3), np.float64, order="F")
        self.b2 = np.zeros((llmax, 18, nrec, 3), np.float64, order="F")
        self.a_b = np.zeros((18, 18, ctl.lld, nsites), np.complex128, order="F")
        self.b2_b = np.zeros((18, 18, ctl.lld, nsites), np.complex128, order="F")
        self.mu_n = np.zeros((18, 18, 2 * ctl.lld + 2, nsites), np.complex128, order="F")
        self.mu_ng = np.zeros_like(self.mu_n)

    def update_lattice(self):
        lat = self.lattice
        self._nn = _fc(lat.nn, np.int32)
        self._iz = _fc(lat.iz, np.int32)
        self._check(self._L.rsrec_set_lattice(self._h, lat.kk, self._nn.shape[1], _ptr(self._nn), _ptr(self._iz), int(lat.nmax), int(lat.ntype)))
        if lat.cr is not None:
            cr = _fc(lat.cr, np.float64)
            assert cr.shape == (3, lat.kk)
            self._check(self._L.rsrec_set_positions(self._h, _ptr(cr)))

    def update_hamiltonian(self):
        """Must be called whenever the caller rebuilt the blocks (self.f90:777-797 does before every recur*)."""
        ham = self.hamiltonian
        keep = {}
        for k in ("ee", "lsham", "eeo", "enim", "hall", "hallo"):
            v = getattr(ham, k)
            keep[k] = None if v is None else _fc(v, np.complex128)
        self._ham_keep = keep
        self._check(self._L.rsrec_set_hamiltonian(self._h, keep["ee"].shape[2], int(bool(ham.hoh)), int(self.control.nsp),
                                                  _ptr(keep["ee"]), _ptr(keep["lsham"]), _ptr(keep["eeo"]), _ptr(keep["enim"]),
                                                  _ptr(keep["hall"]), _ptr(keep["hallo"])))

    def _assemble(self, part, hmag, nbr_type, obarm):
        hoh = bool(self.hamiltonian.hoh)
        hm = _fc(hmag, np.complex128)
        assert hm.ndim == 5 and hm.shape[:2] == (9, 9) and hm.shape[3] == 4, "hmag is (9,9,nslots,4,ncls)"
        nslots, ncls = hm.shape[2], hm.shape[4]
        ty = ob = None
        ntype = 0
        if hoh:
            ty, ob = _fc(nbr_type, np.int32), _fc(obarm, np.complex128)
            assert ty.shape == (nslots, ncls) and ob.shape[:2] == (18, 18)
            ntype = ob.shape[2]
        blocks = np.zeros((18, 18, nslots, ncls), np.complex128, order="F")
        blocks_o = np.zeros_like(blocks) if hoh else None
        self._check(self._L.rsrec_assemble_blocks(self._h, part, ncls, nslots, int(hoh), _ptr(hm), _ptr(ty), _ptr(ob), ntype, _ptr(blocks), _ptr(blocks_o)))
        return blocks, blocks_o

    def build_bulkham(self, hmag, nbr_type=None, obarm=None):
        """hamiltonian%build_bulkham after chbar_nc (hamiltonian.f90:1553-1616), on the device: ee (and eeo = ee.obar with hoh) of every atom
        type from the (Hx, Hy, Hz, H0) parts ``hmag`` (9,9,nslots,4,ntype); fills ``self.hamiltonian.ee / .eeo``.  A following
        update_hamiltonian() finds the blocks on the device."""
        self.hamiltonian.ee, eeo = self._assemble(0, hmag, nbr_type, obarm)
        if eeo is not None:
            self.hamiltonian.eeo = eeo

    def build_locham(self, hmag, nbr_type=None, obarm=None):
        """hamiltonian%build_locham (hamiltonian.f90:1618-1667): hall / hallo of the first nmax atoms, as build_bulkham."""
        self.hamiltonian.hall, hallo = self._assemble(1, hmag, nbr_type, obarm)
        if hallo is not None:
            self.hamiltonian.hallo = hallo

    def _my_sites(self):
        start, end = site_partition(self.rank, self.nprocs, self.lattice.nrec)   # recursion.f90:1816
        return start, end, np.ascontiguousarray(self.lattice.irec[start - 1:end], dtype=np.int32)

    # -- drivers ---------------------------------------------------------------------------------------
    def recur_b(self):
        """Block Lanczos for the sites this rank owns (recursion.f90:1807-1866)."""
        lld = self.control.lld
        start, end, seeds = self._my_sites()
        n = len(seeds)
        a_b = np.zeros((18, 18, lld, n), np.complex128, order="F")
        b2_b = np.zeros_like(a_b)
        self._check(self._L.rsrec_block_lanczos(self._h, n, _ptr(seeds), lld, _ptr(a_b), _ptr(b2_b)))
        self.a_b[:, :, :, :n] = a_b                                   # index i - start_atom + 1 (:1847-1848)
        self.b2_b[:, :, :, :n] = b2_b
        d = np.arange(18)
        self.a[:lld, :, :n, 0] = a_b[d, d].real.transpose(1, 0, 2)    # :1850-1851
        self.b2[:lld, :, :n, 0] = b2_b[d, d].real.transpose(1, 0, 2)

    def recur_b_local_axis(self, rot):
        """recur_b with hamiltonian%local_axis = T (recursion.f90:1830-1832): the Hamiltonian object holds the GLOBAL-frame blocks
        (ee_glob, ...), ``rot`` (18,18,nrec) the spin-frame rotation of every site; all sites go in one batched call.  The coefficients
        are conjugated with the rotations on the device and the chains stay resident there in each site's local frame, the same bits as
        ``a_b`` / ``b2_b``: ``Green.block_ldos()``, ``Green.block_spectra()``, ``Green.contour_occupation(resident=True)`` and
        ``pack_diag()`` follow as after ``recur_b``."""
        lld = self.control.lld
        start, end, seeds = self._my_sites()
        n = len(seeds)
        r = _fc(np.asarray(rot)[:, :, start - 1:end], np.complex128)
        a_b = np.zeros((18, 18, lld, n), np.complex128, order="F")
        b2_b = np.zeros_like(a_b)
        self._check(self._L.rsrec_block_lanczos_local_axis(self._h, n, _ptr(seeds), _ptr(r), lld, _ptr(a_b), _ptr(b2_b)))
        self.a_b[:, :, :, :n] = a_b
        self.b2_b[:, :, :, :n] = b2_b
        d = np.arange(18)
        self.a[:lld, :, :n, 0] = a_b[d, d].real.transpose(1, 0, 2)
        self.b2[:lld, :, :n, 0] = b2_b[d, d].real.transpose(1, 0, 2)

    def pack_diag(self, site_offset, nsites_total, a_img, b2_img):
        """This rank's part of the zero-padded (lld, 18, nsites_total) images of a / b2 that the ranks all-reduce
        (bands.f90:271-274), written from the coefficients resident on the device.  a_img / b2_img: numpy arrays or raw
        (device) addresses, e.g. ``tensor.data_ptr()`` of the CUDA tensor handed to the collective."""
        pa = a_img if isinstance(a_img, int) else a_img.ctypes.data
        pb = b2_img if isinstance(b2_img, int) else b2_img.ctypes.data
        self._check(self._L.rsrec_pack_diag(self._h, int(site_offset), int(nsites_total), C.c_void_p(pa), C.c_void_p(pb)))

    def pack_moments(self, site_offset, nsites_total, mu_img):
        """The Chebyshev counterpart: mu_n(18,18,2 lld + 2,site) of this rank's sites inside a zero image over all sites, written from
        the moments resident on the device.  mu_img: numpy array or raw (device) address."""
        pm = mu_img if isinstance(mu_img, int) else mu_img.ctypes.data
        self._check(self._L.rsrec_pack_moments(self._h, int(site_offset), int(nsites_total), C.c_void_p(pm)))

    # -- library-level communicator (RCCL bound by librsrec itself: no MPI, no torch) -----------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        if _lib.lib().rsrec_comm_unique_id(buf) != 0:
            raise _lib.RsrecError(2, "rsrec_comm_unique_id failed (RCCL not available?)")
        return buf.raw

    def comm_init(self, rank, nranks, ident=None, path=None, timeout_s=60.0):
        """Collective: every rank passes the same 128-byte id (from comm_unique_id on one rank), or a `path` through which rank 0
        publishes it."""
        if path is not None:
            self._check(self._L.rsrec_comm_init_file(self._h, int(rank), int(nranks), os.fsencode(path), float(timeout_s)))
        else:
            self._check(self._L.rsrec_comm_init(self._h, int(rank), int(nranks), ident))

    def comm_size(self):
        r, n = C.c_int(), C.c_int()
        self._check(self._L.rsrec_comm_size(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def allreduce_sum(self, buf, n=None):
        """In-place sum over the ranks (bands.f90:271-274): numpy float64 array, or a raw device address with `n` doubles."""
        if isinstance(buf, int):
            self._check(self._L.rsrec_allreduce_sum(self._h, C.c_void_p(buf), int(n)))
        else:
            # the images this mirror reduces are float64 (diagonals, LDOS) or complex128 (a_b, mu_n): a complex array counts as 2 doubles per element
            if buf.dtype not in (np.float64, np.complex128):
                raise TypeError("allreduce_sum: float64 or complex128 arrays only, got %s" % buf.dtype)
            if not (buf.flags["C_CONTIGUOUS"] or buf.flags["F_CONTIGUOUS"]):
                raise ValueError("allreduce_sum: the array must be contiguous (it is reduced in place)")
            self._check(self._L.rsrec_allreduce_sum(self._h, C.c_void_p(buf.ctypes.data), buf.nbytes // 8))

    def recur_b_ij(self):
        """Four chains per atom pair, seeds (psi_i +- psi_j)/sqrt2 and (psi_i +- i psi_j)/sqrt2 (recursion.f90:1655-1800)."""
        lld = self.control.lld
        pairs = np.asarray(self.lattice.ijpair, dtype=np.int32)
        njij = len(pairs)
        start, end = site_partition(self.rank, self.nprocs, njij)
        slots, sa, sc = self._pair_seeds(pairs[start - 1:end], skip_diagonal_repeats=True)
        nch = len(slots)
        a_b = np.zeros((18, 18, lld, nch), np.complex128, order="F")
        b2_b = np.zeros_like(a_b)
        self._check(self._L.rsrec_block_lanczos_seeded(self._h, nch, 2, _ptr(sa), _ptr(sc), lld, _ptr(a_b), _ptr(b2_b)))
        self.a_b[:, :, :, slots] = a_b
        self.b2_b[:, :, :, slots] = b2_b

    @staticmethod
    def _pair_seeds(pairs, skip_diagonal_repeats):
        """(asign, bsign) of the four chains of every pair (recursion.f90:1679-1707 / :2403-2448); slot = ij_loc*4 - 4 + reci."""
        s2 = 1.0 / np.sqrt(2.0)          # one_over_sqrt_two (math.f90)
        slots, seeds, coefs = [], [], []
        for ij_loc, (i, j) in enumerate(pairs):
            for reci in range(4):
                a, b = s2, (s2, -s2, 1j * s2, -1j * s2)[reci]
                if i == j and skip_diagonal_repeats:
                    if reci > 0:
                        continue                                      # recur_b_ij :1705-1706 `cycle`: slots 2..4 stay zero
                    a = b = 1.0                                       # :1702-1704
                seeds.append((i, j)); coefs.append((a, b))            # assigned in order: for i == j the second value stays
                slots.append(ij_loc * 4 + reci)
        return slots, np.ascontiguousarray(seeds, dtype=np.int32), np.ascontiguousarray(coefs, dtype=np.complex128)

    def chebyshev_recur_ij(self):
        """Chebyshev moments of the four chains per pair (recursion.f90:2376-2487); no i == j special case there."""
        lld = self.control.lld
        a, b = chebyshev_scaling(self.en.energy_min, self.en.energy_max)
        pairs = np.asarray(self.lattice.ijpair, dtype=np.int32)
        start, end = site_partition(self.rank, self.nprocs, len(pairs))
        slots, sa, sc = self._pair_seeds(pairs[start - 1:end], skip_diagonal_repeats=False)
        nch = len(slots)
        mu = np.zeros((18, 18, 2 * lld + 2, nch), np.complex128, order="F")
        self._check(self._L.rsrec_chebyshev_seeded(self._h, nch, 2, _ptr(sa), _ptr(sc), lld, a, b, _ptr(mu)))
        self.mu_n[:, :, :, slots] = mu

    def chebyshev_recur_ij_direct(self, both_ends=False):
        """The moments ``chebyshev_recur_ij`` delivers, from one chain per atom instead of four per pair
        (``rsrec_chebyshev_pairs_direct``): the block at atom j of the Chebyshev vector started at atom i is M_ji(n) = <j|T_n|i>.
        ``both_ends=False``: one chain per distinct first atom, M_ij := M_ji^H (the caller asserts a Hermitian H), and the slots written to
        ``self.mu_n`` lack the (M_ii + M_jj)/2 that every consumer cancels.  ``both_ends=True``: chains from both atoms of every pair,
        the reference's own slot values.  Same rank partition of ``ijpair`` and the same slots ij_loc*4 - 4 + reci as
        ``chebyshev_recur_ij``; the image stays resident for ``Exchange.compute(resident=True)`` and its siblings.  Returns ``m_pair``
        (18, 18, 2 lld + 2, 2, npairs): M_ij and M_ji of this rank's pairs."""
        lld = self.control.lld
        a, b = chebyshev_scaling(self.en.energy_min, self.en.energy_max)
        pairs = np.asarray(self.lattice.ijpair, dtype=np.int32).reshape(-1, 2)
        start, end = site_partition(self.rank, self.nprocs, len(pairs))
        mine = np.ascontiguousarray(pairs[start - 1:end])            # (npairs, 2) in C order = (2, npairs) column-major
        n = len(mine)
        mu = np.zeros((18, 18, 2 * lld + 2, 4 * n), np.complex128, order="F")
        m_pair = np.zeros((18, 18, 2 * lld + 2, 2, n), np.complex128, order="F")
        self._check(self._L.rsrec_chebyshev_pairs_direct(self._h, n, _ptr(mine), lld, a, b, int(bool(both_ends)), _ptr(mu), _ptr(m_pair)))
        self.mu_n[:, :, :, :4 * n] = mu
        return m_pair

    def chebyshev_bloch(self, sources, kpts, cr, cell=None, group=None, download=True):
        """k-resolved Chebyshev moments from one chain per source atom (``rsrec_chebyshev_bloch``): the lattice Fourier sum
        S_i(k, n) = sum_j exp(-i k.(r_j - r_i)) <j|T_n(H~)|i> of the Chebyshev vector started at atom i -- T_n(H~(k)) itself on a periodic
        one-atom cell.  ``sources``: 1-based atoms; ``kpts`` (3, nk) Cartesian with 2 pi; ``cr`` (3, kk) positions; ``cell`` (3, 3) with the
        supercell vectors as columns (displacements are then reduced to their minimum image) or None; ``group`` (kk) with values 0..ngroup
        (0: left out) or None (every atom in group 1).  Returns (18, 18, 2 lld + 2, nk, ngroup, nsrc), or None with ``download=False``;
        either way the image stays resident as ``chebyshev_recur`` of nk * ngroup * nsrc sites leaves it (image q + nk (g + ngroup s))."""
        lld = self.control.lld
        a, b = chebyshev_scaling(self.en.energy_min, self.en.energy_max)
        src = np.ascontiguousarray(sources, dtype=np.int32).ravel()
        k = _fc(kpts, np.float64).reshape(3, -1, order="F")
        cr = _fc(cr, np.float64)
        if cr.shape != (3, self.lattice.kk):
            raise ValueError("cr must be (3, kk), got %r" % (cr.shape,))
        cell = None if cell is None else _fc(cell, np.float64).reshape(3, 3, order="F")
        ngroup = 1
        if group is not None:
            group = np.ascontiguousarray(group, dtype=np.int32).ravel()
            if group.shape != (self.lattice.kk,):
                raise ValueError("group must be (kk,), got %r" % (group.shape,))
            ngroup = max(int(group.max()), 1)
        nk = k.shape[1]
        s_k = np.zeros((18, 18, 2 * lld + 2, nk, ngroup, len(src)), np.complex128, order="F") if download else None
        self._check(self._L.rsrec_chebyshev_bloch(self._h, len(src), _ptr(src), lld, a, b, _ptr(cr), _ptr(cell), nk, _ptr(k), ngroup, _ptr(group), _ptr(s_k)))
        return s_k

    def bloch_spectral(self, green, sources, kpts, cr, cell=None, group=None):
        """Orbital-resolved Bloch spectral weights on ``green``'s energy mesh: ``chebyshev_bloch`` without a download, then the LDOS stage
        on the resident image (``green.chebyshev_ldos``).  Returns ``dosial`` as (nk, ngroup, nsrc, 18, nen); summed over the orbitals it
        is A(k,E) = -Im Tr G(k,E) / pi of the source's group sum."""
        self.chebyshev_bloch(sources, kpts, cr, cell=cell, group=group, download=False)
        nk = np.asarray(kpts).reshape(3, -1, order="F").shape[1]
        ngroup = 1 if group is None else max(int(np.max(group)), 1)
        nsrc = np.asarray(sources).size
        nimg = nk * ngroup * nsrc
        img = green.chebyshev_ldos(nsites_total=nimg)
        return img["dosial"].reshape((nk, ngroup, nsrc, 18, -1), order="F")

    def chebyshev_green_weights(self, energies):
        """``chebyshev_green_weights`` of this module at the object's depth and window: complex (2 lld + 2, ne)."""
        return chebyshev_green_weights(energies, self.control.lld, self.en.energy_min, self.en.energy_max)

    def bloch_map(self, sources, kpts, cr, energies=None, weights=None, cell=None, group=None, blocks=True, diag=True):
        """A function of H at many k-points and a few energies from one chain per source atom (``rsrec_chebyshev_bloch_map``): the sums of
        ``chebyshev_bloch`` in the other order, g_k(:, :, e, q, g, s) = sum_n w(n, e) S_s(k_q, n) restricted to group g, without ever forming
        the moments -- ne accumulated vectors per chain and one Bloch sum per energy.  ``sources``, ``kpts`` (3, nk), ``cr``, ``cell`` and
        ``group`` as ``chebyshev_bloch`` takes them (kk atoms); give either ``energies`` -- the Green weights of ``chebyshev_green_weights``,
        so that g_k = G(k, E) -- or ``weights`` complex (2 lld + 2, ne), row n for order n - 1, any function of H.  Returns ``(g_k, a_k)``:
        g_k complex (18, 18, ne, nk, ngroup, nsrc) or None with ``blocks=False``; a_k real (18, ne, nk, ngroup, nsrc) = -Im diag g_k / pi,
        bit for bit, or None with ``diag=False``.  Nothing is normalised, nothing stays resident, and only the sum over the groups has a
        non-negative spectral weight."""
        if (energies is None) == (weights is None):
            raise ValueError("give either energies or weights")
        lld = self.control.lld
        a, b = chebyshev_scaling(self.en.energy_min, self.en.energy_max)
        w = self.chebyshev_green_weights(energies) if weights is None else _fc(weights, np.complex128)
        if w.ndim != 2 or w.shape[0] != 2 * lld + 2:
            raise ValueError("weights must be (2 lld + 2, ne) = (%d, ne), got %r" % (2 * lld + 2, w.shape))
        if not (blocks or diag):
            raise ValueError("nothing asked for: blocks and diag are both False")
        src = np.ascontiguousarray(sources, dtype=np.int32).ravel()
        k = _fc(kpts, np.float64).reshape(3, -1, order="F")
        cr = _fc(cr, np.float64)
        if cr.shape != (3, self.lattice.kk):
            raise ValueError("cr must be (3, kk), got %r" % (cr.shape,))
        cell = None if cell is None else _fc(cell, np.float64).reshape(3, 3, order="F")
        group, ngroup = self._group(group)
        ne, nk = w.shape[1], k.shape[1]
        g_k = np.zeros((18, 18, ne, nk, ngroup, len(src)), np.complex128, order="F") if blocks else None
        a_k = np.zeros((18, ne, nk, ngroup, len(src)), np.float64, order="F") if diag else None
        self._check(self._L.rsrec_chebyshev_bloch_map(self._h, len(src), _ptr(src), lld, a, b, _ptr(cr), _ptr(cell), nk, _ptr(k), ngroup, _ptr(group),
                                                      ne, _ptr(w), _ptr(g_k), _ptr(a_k)))
        return g_k, a_k

    def constant_energy_map(self, sources, origin, u, v, n1, n2, cr, energy, cell=None, group=None):
        """A(k, E) at one energy on the grid k = origin + (i / n1) u + (j / n2) v, i < n1, j < n2 (Cartesian, 2 pi included) -- a Fermi-surface
        or constant-energy cut: ``bloch_map`` with the Green weights of ``energy``, diagonal only, summed over the 18 orbitals.  Returns
        (n1, n2, ngroup, nsrc).  Nothing is normalised (kk atoms, one source: the trace of the source's own spectral function), and only
        the sum over the groups has a non-negative spectral weight."""
        origin, u, v = (np.asarray(x, np.float64).reshape(3) for x in (origin, u, v))
        i, j = np.meshgrid(np.arange(n1) / float(n1), np.arange(n2) / float(n2), indexing="ij")
        k = origin[:, None] + u[:, None] * i.ravel(order="F")[None, :] + v[:, None] * j.ravel(order="F")[None, :]
        a_k = self.bloch_map(sources, k, cr, energies=[energy], cell=cell, group=group, blocks=False)[1]
        return a_k.sum(axis=0)[0].reshape((n1, n2) + a_k.shape[3:], order="F")

    def _group(self, group):
        """(group as int32 (kk) or None, ngroup) of the calls that take atom groups 0..ngroup."""
        if group is None:
            return None, 1
        group = np.ascontiguousarray(group, dtype=np.int32).ravel()
        if group.shape != (self.lattice.kk,):
            raise ValueError("group must be (kk,), got %r" % (group.shape,))
        return group, max(int(group.max()), 1)

    def chebyshev_lattice(self, seeds, coefs, group=None, download=True):
        """Chebyshev moments from whole-lattice seeds (``rsrec_chebyshev_lattice``): chain c starts from |x> = sum_j c_j |j> (x) 1_18 with
        ``seeds`` (nchains, nseed) 1-based atoms (0: unused entry) and ``coefs`` (nchains, nseed) complex, placed as
        ``compute_moments_stochastic`` places its vectors, and M_g(n) = sum_{j in g} conj(c_j) [T_{n-1}(H~) x]_j = <x|P_g T_{n-1}(H~)|x>.
        ``group`` (kk) with values 0..ngroup (0: left out) or None (every atom in group 1).  Returns (18, 18, 2 lld + 2, ngroup, nchains),
        or None with ``download=False``; either way the image stays resident as ``chebyshev_recur`` of ngroup * nchains sites leaves it
        (image g + ngroup c).  Nothing is normalised here: with |c_j|^2 = 1/kk, tr M_g(1) = 18 N_g / kk, and the caller divides.  Only the
        sum over the groups is Hermitian; the LDOS stage reads the real part of an image's diagonal, the symmetrised group weight."""
        lld = self.control.lld
        a, b = chebyshev_scaling(self.en.energy_min, self.en.energy_max)
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        coefs = np.ascontiguousarray(coefs, dtype=np.complex128)
        if seeds.ndim != 2 or coefs.shape != seeds.shape:
            raise ValueError("seeds and coefs must both be (nchains, nseed), got %r and %r" % (seeds.shape, coefs.shape))
        group, ngroup = self._group(group)
        nchains, nseed = seeds.shape
        m_g = np.zeros((18, 18, 2 * lld + 2, ngroup, nchains), np.complex128, order="F") if download else None
        self._check(self._L.rsrec_chebyshev_lattice(self._h, nchains, nseed, _ptr(seeds), _ptr(coefs), lld, a, b, ngroup, _ptr(group), _ptr(m_g)))
        return m_g

    def site_map(self, seeds, coefs, weights=None, energies=None, blocks=True, diag=True, norm=True):
        """The 18 x 18 block of ne functions of H on EVERY atom from a few whole-lattice vectors (``rsrec_chebyshev_site_map``):
        D(:, :, e, j) = sum_v conj(c^v_j) [sum_n w(n, e) T_{n-1}(H~) x^v]_j = cnorm_j f_e(H~)_jj + cross terms, with ``seeds`` and ``coefs``
        (nvec, nseed) as ``chebyshev_lattice`` takes them.  The cross terms average out over random-phase vectors and vanish for probing
        vectors whose atoms are further apart than the degree 2 lld + 1 (``probing_seeds``).  Give either ``weights`` complex
        (2 lld + 2, ne), row n for order n - 1, ne <= 16 -- any function of H, e.g. ``chebyshev_fermi_weights`` -- or ``energies``, shorthand
        for ``chebyshev_green_weights``.  Returns ``(d_full, d_diag, cnorm)``: complex (18, 18, ne, kk), complex (18, ne, kk) -- bit for bit
        the diagonal of d_full -- and real (kk) = sum_v |c^v_j|^2 of the coefficients placed; each None when ``blocks``, ``diag`` or
        ``norm`` is False.  Nothing is normalised (divide by cnorm) and nothing stays resident.  The bits depend on the order of the
        vectors and on the options sitemap_vtile, sitemap_orders and kubo_vbatch: the accumulators are shared by all vectors."""
        if (energies is None) == (weights is None):
            raise ValueError("give either energies or weights")
        lld = self.control.lld
        a, b = chebyshev_scaling(self.en.energy_min, self.en.energy_max)
        w = self.chebyshev_green_weights(energies) if weights is None else _fc(weights, np.complex128)
        if w.ndim != 2 or w.shape[0] != 2 * lld + 2:
            raise ValueError("weights must be (2 lld + 2, ne) = (%d, ne), got %r" % (2 * lld + 2, w.shape))
        if not (blocks or diag):
            raise ValueError("nothing asked for: blocks and diag are both False")
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        coefs = np.ascontiguousarray(coefs, dtype=np.complex128)
        if seeds.ndim != 2 or coefs.shape != seeds.shape:
            raise ValueError("seeds and coefs must both be (nvec, nseed), got %r and %r" % (seeds.shape, coefs.shape))
        nvec, nseed = seeds.shape
        ne, kk = w.shape[1], self.lattice.kk
        d_full = np.zeros((18, 18, ne, kk), np.complex128, order="F") if blocks else None
        d_diag = np.zeros((18, ne, kk), np.complex128, order="F") if diag else None
        cnorm = np.zeros(kk, np.float64) if norm else None
        self._check(self._L.rsrec_chebyshev_site_map(self._h, nvec, nseed, _ptr(seeds), _ptr(coefs), lld, a, b, ne, _ptr(w), _ptr(d_full), _ptr(d_diag),
                                                     _ptr(cnorm)))
        return d_full, d_diag, cnorm

    @staticmethod
    def _site_norm(cnorm):
        """What the front ends divide by: cnorm, and 1 on an atom no vector seeds (its block is an exact zero and stays one)."""
        return np.where(cnorm > 0, cnorm, 1.0)

    def site_ldos(self, seeds, coefs, energies):
        """The orbital-resolved LDOS of every atom at a few energies from the vectors of ``site_map``: -Im d_diag / pi / cnorm with the
        Green weights of ``energies``, real (18, ne, kk) -- the map an STM-like image of an impurity cell or a slab surface is cut from.
        Exact for one-atom and for far-apart probing seeds, a stochastic estimate for random-phase ones.  An atom seeded by no vector
        gives zeros."""
        _, d_diag, cnorm = self.site_map(seeds, coefs, energies=energies, blocks=False)
        return -d_diag.imag / np.pi / self._site_norm(cnorm)[None, None, :]

    def site_occupations(self, seeds, coefs, fermi, kT, powers=(0,)):
        """The occupation matrix of every atom, and with further ``powers`` its energy moments: d_full / cnorm of ``site_map`` on the columns
        of ``chebyshev_fermi_weights(fermi, kT, lld, energy_min, energy_max, powers)``, complex (18, 18, len(powers), kk); column q
        estimates [H^q f(H)]_jj.  The trace of column 0 is the atom's charge, the spin blocks give its moment.  An atom seeded by no
        vector gives zeros."""
        w = chebyshev_fermi_weights(fermi, kT, self.control.lld, self.en.energy_min, self.en.energy_max, powers)
        d_full, _, cnorm = self.site_map(seeds, coefs, weights=w, diag=False)
        return d_full / self._site_norm(cnorm)[None, None, None, :]

    def bloch_average(self, kpts, cr, group=None, download=True):
        """The source average of ``chebyshev_bloch``, one chain per k-point instead of kk: plane-wave seeds c_j = exp(+i k.r_j) / sqrt(kk) on
        every atom, built here in float64 from ``kpts`` (3, nk) Cartesian with 2 pi and ``cr`` (3, kk).  The sum over the groups of the
        result is (1/kk) sum_i S_i(k, n), the moments of the effective (unfolded) band structure of a disordered supercell; ``group``
        resolves it by atom type or layer, tr M_g(1) = 18 N_g / kk.  Returns (18, 18, 2 lld + 2, ngroup, nk), see ``chebyshev_lattice``."""
        kk = self.lattice.kk
        k = np.asarray(kpts, np.float64).reshape(3, -1, order="F")
        cr = np.asarray(cr, np.float64)
        if cr.shape != (3, kk):
            raise ValueError("cr must be (3, kk), got %r" % (cr.shape,))
        coefs = np.exp(1j * (k.T @ cr)) / np.sqrt(float(kk))                      # (nk, kk)
        seeds = np.tile(np.arange(1, kk + 1, dtype=np.int32), (k.shape[1], 1))
        return self.chebyshev_lattice(seeds, coefs, group=group, download=download)

    def bloch_average_spectral(self, green, kpts, cr, group=None):
        """Orbital-resolved weights of the source-averaged Bloch spectral function on ``green``'s energy mesh: ``bloch_average`` without a
        download, then the LDOS stage on the resident image.  Returns ``dosial`` as (ngroup, nk, 18, nen); summed over the orbitals and the
        groups it is the effective A(k,E) of the cell, each group carrying its weight N_g / kk."""
        self.bloch_average(kpts, cr, group=group, download=False)
        nk = np.asarray(kpts).reshape(3, -1, order="F").shape[1]
        ngroup = self._group(group)[1]
        img = green.chebyshev_ldos(nsites_total=ngroup * nk)
        return img["dosial"].reshape((ngroup, nk, 18, -1), order="F")

    def cell_moments(self, rng, group=None, download=True):
        """Stochastic-trace moments of the whole cell by atom group, on the vectors ``cond_calctype = 'random_vec'`` builds from its random
        numbers ``rng`` (kk, nvec) (recursion.f90:1130-1138): c_j = exp(2 pi i rng_j) / sqrt(real(kk)), the single-precision square root
        widened, as there.  M_g(n) estimates (1/kk) sum_{j in g} <j|T_{n-1}(H~)|j>: tr M_g(1) = 18 N_g / kk up to that rounding of the norm,
        and the caller divides.  Returns (18, 18, 2 lld + 2, ngroup, nvec), see ``chebyshev_lattice``."""
        rng = np.asarray(rng, np.float64)
        if rng.ndim != 2 or rng.shape[0] != self.lattice.kk:
            raise ValueError("rng must be (kk, nvec), got %r" % (rng.shape,))
        kk, nvec = rng.shape
        coefs = np.ascontiguousarray((np.exp(2.0 * np.pi * 1j * rng) / float(np.sqrt(np.float32(kk)))).T)
        seeds = np.tile(np.arange(1, kk + 1, dtype=np.int32), (nvec, 1))
        return self.chebyshev_lattice(seeds, coefs, group=group, download=download)

    def zsqr(self):
        """b2_b <- sqrt(b2_b) in place (recursion.f90:1980-2023)."""
        self._check(self._L.rsrec_zsqr(self._h, self.b2_b.shape[2] * self.b2_b.shape[3], _ptr(self.b2_b)))

    def chebyshev_recur(self):
        """Chebyshev moments for the sites this rank owns (recursion.f90:3057-3130)."""
        lld = self.control.lld
        a, b = chebyshev_scaling(self.en.energy_min, self.en.energy_max)
        start, end, seeds = self._my_sites()
        n = len(seeds)
        mu = np.zeros((18, 18, 2 * lld + 2, n), np.complex128, order="F")
        self._check(self._L.rsrec_chebyshev(self._h, n, _ptr(seeds), lld, a, b, _ptr(mu)))
        self.mu_n[:, :, :, :n] = mu

    def compute_moments_stochastic(self, v_a, v_b, cond_ll, vo_a=None, vo_b=None, seeds=None, coefs=None, atlist=None, diag=False,
                                   resident_only=False):
        """Kubo-Bastin double moments mu_nm_stochastic(18,18,cond_ll,cond_ll,nvec) (recursion.f90:979-1234).
        ``cond_calctype='per_type'``: pass ``atlist`` (lattice%atlist, one seed atom per type).  Random vectors: pass ``seeds``
        (nvec, nseed) atoms and ``coefs`` (nvec, nseed) complex (the caller owns the random numbers).

        ``diag=True``: only the orbital-diagonal moments mu_nm(l,l,n,m,v), the ones conductivity.f90:289, :292 read
        (``rsrec_kubo_moments_diag``): complex128 (18, cond_ll, cond_ll, nvec) in Fortran order.  They also stay on the device for
        ``Conductivity.integrand(None, ene)``; with ``resident_only=True`` nothing is downloaded and None is returned."""
        keep = [None if v is None else _fc(v, np.complex128) for v in (v_a, vo_a, v_b, vo_b)]
        if diag:
            return self._kubo_moments(self._L.rsrec_kubo_moments_diag, (), keep, cond_ll, seeds, coefs, atlist, (), resident_only)
        return self._kubo_moments(self._L.rsrec_kubo_moments, (), keep, cond_ll, seeds, coefs, atlist, None, False)

    def _kubo_moments(self, entry, counts, ops, cond_ll, seeds, coefs, atlist, sets, resident_only):
        """What the compute_moments_stochastic* methods share: the vectors normalised, the result allocated, the call of ``entry`` and
        the bookkeeping.  ``counts``: the set counts the entry point takes before nvec; ``ops``: its four operators (v_out, vo_out,
        v_in, vo_in), Fortran-contiguous or None; ``sets``: the trailing extents of the diagonal result, None for the full moments."""
        a, b = chebyshev_scaling(self.en.energy_min, self.en.energy_max)
        if seeds is None:
            seeds = np.asarray(atlist, dtype=np.int32).reshape(-1, 1)
            coefs = np.ones(seeds.shape, np.complex128)
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        coefs = np.ascontiguousarray(coefs, dtype=np.complex128)
        nvec, nseed = seeds.shape
        shape = (18, 18, cond_ll, cond_ll, nvec) if sets is None else (18, cond_ll, cond_ll, nvec) + sets
        mu = None if resident_only else np.zeros(shape, np.complex128, order="F")
        self._check(entry(self._h, *counts, nvec, nseed, _ptr(seeds), _ptr(coefs), int(cond_ll), a, b, *[_ptr(k) for k in ops], _ptr(mu)))
        if sets is None:
            self.mu_nm_stochastic = mu
        else:
            self.mu_diag_resident = (int(cond_ll), nvec * int(np.prod(sets)))   # what Conductivity.integrand(None, ...) asks the library for
        return mu

    def compute_moments_stochastic_multi(self, v_out, v_b, cond_ll, vo_out=None, vo_b=None, seeds=None, coefs=None, atlist=None,
                                         resident_only=False):
        """The orbital-diagonal Kubo moments of several responses to one applied field (``rsrec_kubo_moments_diag_multi``):
        ``v_out`` (18, 18, nslots, ntype, nout) holds one output operator per response (``vo_out`` likewise, hoh only), ``v_b`` the
        input operator; vectors as in ``compute_moments_stochastic``.  Set j of the result, complex128 (18, cond_ll, cond_ll, nvec,
        nout) in Fortran order, is ``compute_moments_stochastic(v_out[..., j], v_b, diag=True)`` bit for bit, at (2 + nout) instead of
        3 nout whole-lattice products per moment order.  The moments stay on the device as nvec * nout vectors, set outermost:
        ``Conductivity.integrand(None, ene)`` returns (18, nen, nvec * nout), and ``Conductivity.tensor`` takes a set's slice
        ``[:, :, j * nvec:(j + 1) * nvec]``.  ``resident_only=True``: nothing is downloaded and None is returned."""
        keep = [None if v is None else _fc(v, np.complex128) for v in (v_out, vo_out, v_b, vo_b)]
        if keep[0].ndim != 5 or (keep[1] is not None and keep[1].shape != keep[0].shape):
            raise ValueError("v_out (and vo_out) must be (18, 18, nslots, ntype, nout), got %s" % (keep[0].shape,))
        nout = keep[0].shape[4]
        return self._kubo_moments(self._L.rsrec_kubo_moments_diag_multi, (nout,), keep, cond_ll, seeds, coefs, atlist, (nout,),
                                  resident_only)

    def compute_moments_stochastic_tensor(self, v_out, v_in, cond_ll, vo_out=None, vo_in=None, seeds=None, coefs=None, atlist=None,
                                          resident_only=False):
        """The orbital-diagonal Kubo moments of several responses to several applied fields (``rsrec_kubo_moments_diag_tensor``):
        ``v_out`` (18, 18, nslots, ntype, nout) holds one output operator per response and ``v_in`` (18, 18, nslots, ntype, nin) one
        input operator per field (``vo_out``, ``vo_in`` likewise, hoh only); a single (18, 18, nslots, ntype) operator counts as one
        output or one input.  Vectors as in ``compute_moments_stochastic``.  Set (j, i) of the result, complex128 (18, cond_ll, cond_ll,
        nvec, nout, nin) in Fortran order, is ``compute_moments_stochastic(v_out[..., j], v_in[..., i], diag=True)`` bit for bit, and
        slice ``[..., i]`` is ``compute_moments_stochastic_multi(v_out, v_in[..., i])``.  The moments stay on the device as
        nvec * nout * nin vectors, input outermost: ``Conductivity.integrand(None, ene)`` returns (18, nen, nvec * nout * nin), and
        ``Conductivity.tensor`` takes a set's slice ``[:, :, s * nvec:(s + 1) * nvec]`` with s = i * nout + j.
        ``resident_only=True``: nothing is downloaded and None is returned."""
        def five(v):                        # one operator (18, 18, nslots, ntype) -> a stack of one
            if v is None:
                return None
            v = np.asarray(v)
            return _fc(v[..., None] if v.ndim == 4 else v, np.complex128)
        keep = [five(v) for v in (v_out, vo_out, v_in, vo_in)]
        for name, k, ko in (("v_out", keep[0], keep[1]), ("v_in", keep[2], keep[3])):
            if k is None or k.ndim != 5 or (ko is not None and ko.shape != k.shape):
                raise ValueError("%s (and its vo) must be (18, 18, nslots, ntype[, n]), got %s" % (name, None if k is None else k.shape))
        nout, nin = keep[0].shape[4], keep[2].shape[4]
        return self._kubo_moments(self._L.rsrec_kubo_moments_diag_tensor, (nin, nout), keep, cond_ll, seeds, coefs, atlist, (nout, nin),
                                  resident_only)

    def kubo_single_shot(self, v_out, v_b, wl, wr, vo_out=None, vo_b=None, seeds=None, coefs=None, atlist=None, blocks=False):
        """The double sum over the Kubo moments at a few weight columns without the moments (``rsrec_kubo_single_shot``):
        s(:, :, e, v, j) = sum_{n,m} wl(m, e) wr(n, e) mu_j(:, :, n, m, v), mu_j what ``compute_moments_stochastic`` returns for
        (v_a, v_b) = (v_out[..., j], v_b), from L_e = sum_m conj(wl(m, e)) T_{m-1}(H~) r and R_e = sum_n wr(n, e) T_{n-1}(H~) v_b r --
        no left matrix, no cond_ll x cond_ll contraction, 2 (cond_ll - 1) chain steps per vector whatever the cell size.
        ``v_out`` (18, 18, nslots, ntype[, nout]) (``vo_out`` likewise, hoh only), ``v_b`` one input operator; ``wl``, ``wr`` complex
        (cond_ll, ne), ne <= 16, row n for order n - 1 (``kubo_greenwood_weights``, ``kubo_bastin_weights``, or any table: the library does
        not interpret them, and conjugates ``wl`` itself on the bra side).  Vectors as ``compute_moments_stochastic_multi`` takes them:
        ``atlist``, or ``seeds`` and ``coefs`` (nvec, nseed).  Returns ``s_diag`` complex (18, ne, nvec, nout) in Fortran order, or
        ``(s_diag, s_full)`` with ``blocks=True``, s_full complex (18, 18, ne, nvec, nout) whose diagonal s_diag is bit for bit.
        Nothing is normalised and nothing stays resident (resident diagonal moments of an earlier call are dropped).  A Fermi-sea
        integral over a whole mesh (sigma_xy) still needs the moments: ``compute_moments_stochastic(diag=True)`` and
        ``Conductivity.tensor``."""
        def five(v):
            if v is None:
                return None
            v = np.asarray(v)
            return _fc(v[..., None] if v.ndim == 4 else v, np.complex128)
        keep = [five(v_out), five(vo_out), None if v_b is None else _fc(v_b, np.complex128), None if vo_b is None else _fc(vo_b, np.complex128)]
        if keep[0] is None or keep[0].ndim != 5 or (keep[1] is not None and keep[1].shape != keep[0].shape):
            raise ValueError("v_out (and vo_out) must be (18, 18, nslots, ntype[, nout]), got %s" % (None if keep[0] is None else keep[0].shape,))
        wl, wr = _fc(wl, np.complex128), _fc(wr, np.complex128)
        if wl.ndim != 2 or wr.shape != wl.shape:
            raise ValueError("wl and wr must both be (cond_ll, ne), got %r and %r" % (wl.shape, wr.shape))
        cond_ll, ne = wl.shape
        nout = keep[0].shape[4]
        a, b = chebyshev_scaling(self.en.energy_min, self.en.energy_max)
        if seeds is None:
            seeds = np.asarray(atlist, dtype=np.int32).reshape(-1, 1)
            coefs = np.ones(seeds.shape, np.complex128)
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        coefs = np.ascontiguousarray(coefs, dtype=np.complex128)
        nvec, nseed = seeds.shape
        s_diag = np.zeros((18, ne, nvec, nout), np.complex128, order="F")
        s_full = np.zeros((18, 18, ne, nvec, nout), np.complex128, order="F") if blocks else None
        self._check(self._L.rsrec_kubo_single_shot(self._h, nout, nvec, nseed, _ptr(seeds), _ptr(coefs), int(cond_ll), a, b, *[_ptr(k) for k in keep],
                                                   int(ne), _ptr(wl), _ptr(wr), _ptr(s_full), _ptr(s_diag)))
        if nvec > 0:                                   # (a call without vectors returns before the handle drops anything)
            self.mu_diag_resident = None
        return (s_diag, s_full) if blocks else s_diag

    def evolve(self, d_op, w, nt, stride=1, mom=0, do_op=None, seeds=None, coefs=None, atlist=None, blocks=False):
        """Wave-packet propagation (``rsrec_chebyshev_evolve``): psi(t) = U(t) r and chi(t) = [X, U(t)] r from psi(0) = r, chi(0) = 0 in
        nt * stride steps of the Chebyshev table ``w`` (``evolution_weights(tau, korder, a, b)`` with a, b of ``chebyshev_scaling``; complex
        (korder), not interpreted), with D = ``d_op`` (``do_op`` too with hoh; ``position_commutator``).  A record after every ``stride``
        steps, s = 1 .. nt.  Vectors as ``compute_moments_stochastic`` takes them: ``atlist``, or ``seeds`` and ``coefs`` (nvec, nseed).
        Returns a dict, Fortran order: ``ret`` complex (18, 18, nt, nvec) = r^H psi(t_s); with ``mom`` > 0 also ``m_diag`` (18, mom, nt,
        nvec), the orbital diagonals of chi(t_s)^H T_{n-1}(H~) chi(t_s), and ``m0_diag`` (18, mom, nvec), the same of r (the DOS moments);
        with ``blocks=True`` also ``m_full`` (18, 18, mom, nt, nvec) and ``m0_full``, whose diagonals the diag forms are bit for bit.
        Nothing is normalised and nothing stays resident (resident diagonal moments of an earlier call are dropped).
        ``Conductivity.spreading`` turns the dict into DX^2(E, t), D(E, t) and the DOS."""
        d_op = _fc(d_op, np.complex128)
        do_op = None if do_op is None else _fc(do_op, np.complex128)
        w = np.ascontiguousarray(w, dtype=np.complex128).ravel()
        a, b = chebyshev_scaling(self.en.energy_min, self.en.energy_max)
        if seeds is None:
            seeds = np.asarray(atlist, dtype=np.int32).reshape(-1, 1)
            coefs = np.ones(seeds.shape, np.complex128)
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        coefs = np.ascontiguousarray(coefs, dtype=np.complex128)
        nvec, nseed = seeds.shape
        nt, stride, mom = int(nt), int(stride), int(mom)

        def out(*shape):
            return np.zeros(shape, np.complex128, order="F")
        res = {"ret": out(18, 18, max(nt, 0), nvec)}
        if mom > 0:
            res["m0_diag"], res["m_diag"] = out(18, mom, nvec), out(18, mom, max(nt, 0), nvec)
            if blocks:
                res["m0_full"], res["m_full"] = out(18, 18, mom, nvec), out(18, 18, mom, max(nt, 0), nvec)
        self._check(self._L.rsrec_chebyshev_evolve(self._h, nvec, nseed, _ptr(seeds), _ptr(coefs), a, b, _ptr(d_op), _ptr(do_op), int(w.size), _ptr(w), nt, stride, mom,
                                                   _ptr(res["ret"]), _ptr(res.get("m0_full")), _ptr(res.get("m0_diag")), _ptr(res.get("m_full")), _ptr(res.get("m_diag"))))
        if nvec > 0:                                   # (a call without vectors returns before the handle drops anything)
            self.mu_diag_resident = None
        return res

    def ham_vec_matmul(self, psi_in, a, b):
        """psi_out = (H psi_in - b psi_in)/a on a whole vector psi(18,18,kk) with the PLAIN operator ee + l.s, whatever hoh says
        (recursion.f90:913-977)."""
        x = _fc(psi_in, np.complex128)
        out = np.zeros_like(x)
        self._check(self._L.rsrec_apply_operator(self._h, 2, None, None, _ptr(x), _ptr(out), float(a), float(b)))
        return out

    def ham_hoh_vec_matmul(self, psi_in, a, b):
        """The same with H = h - h o h + e_nu + l.s (recursion.f90:785-911); needs hamiltonian%hoh."""
        x = _fc(psi_in, np.complex128)
        out = np.zeros_like(x)
        self._check(self._L.rsrec_apply_operator(self._h, 0, None, None, _ptr(x), _ptr(out), float(a), float(b)))
        return out

    def chebyshev_orbital_mod(self, cr, alat, seeds=None, per_seed=False):
        """The moments of chebyshev_orbital_mod (recursion.f90:2834-3049): mu_n_orb(18,18,lld) = (1/kk) sum over all atoms as seeds
        (`seeds` = a subset: the plain sum over it, not divided), device-resident.  per_seed: also every seed's contribution."""
        lld = self.control.lld
        a, b = chebyshev_scaling(self.en.energy_min, self.en.energy_max)
        kk = self.lattice.kk
        sd = np.arange(1, kk + 1, dtype=np.int32) if seeds is None else np.ascontiguousarray(seeds, dtype=np.int32)
        crf = _fc(cr, np.float64)
        assert crf.shape == (3, kk)
        mu = np.zeros((18, 18, lld), np.complex128, order="F")
        ms = np.zeros((18, 18, lld, len(sd)), np.complex128, order="F") if per_seed else None
        self._check(self._L.rsrec_orbital_moments(self._h, len(sd), _ptr(sd), lld, a, b, _ptr(crf), float(alat), _ptr(mu), _ptr(ms)))
        if seeds is None:
            mu = mu / float(kk)                                   # :3006
        return (mu, ms) if per_seed else mu

    def velo_vec_matmul(self, v_op, psi_in, vo_op=None):
        """psi_out = V psi_in (recursion.f90:587; :656 with hoh)."""
        x = _fc(psi_in, np.complex128)
        out = np.zeros_like(x)
        v = _fc(v_op, np.complex128)
        vo = None if vo_op is None else _fc(vo_op, np.complex128)
        self._check(self._L.rsrec_apply_operator(self._h, 1, _ptr(v), _ptr(vo), _ptr(x), _ptr(out), 1.0, 0.0))
        return out

    def recur(self):
        """Scalar Haydock recursion, 18 orbital chains per site (recursion.f90:3485-3532)."""
        lld = self.control.lld
        llmax = self.a.shape[0]
        start, end, seeds = self._my_sites()
        n = len(seeds)
        a = np.zeros((llmax, 18, n), np.float64, order="F")
        b2 = np.zeros_like(a)
        self._check(self._L.rsrec_scalar_lanczos(self._h, n, _ptr(seeds), lld, llmax, _ptr(a), _ptr(b2)))
        self.a[:, :, :n, 0] = a
        self.b2[:, :, :n, 0] = b2
