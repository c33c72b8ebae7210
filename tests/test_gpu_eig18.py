"""The 18x18 eigen-solver of the library (jacobi18 + matfun18, csrc/eig18.hpp) as a SOLVER: rsrec_zsqr on a handle with no lattice and
no Hamiltonian, on the inputs with known roots of tests/eig18_cases.py -- exact integer roots, degenerate / clustered / graded spectra
with roots from a 50-digit fixture, inputs Hermitian only to rounding --, every class in ONE call (one workgroup per matrix).

  * forward error to the exact root <= max(1e-13, 16 x the CPU oracle's own error on that input), relative Frobenius;
  * backward error ||B B - S|| <= 1e-13 ||S||, ||B - B^H|| <= 1e-13 ||B||, eig(B) >= -1e-13 ||B||;
  * diagonal inputs leave before the first sweep: sqrt of the diagonal bit for bit, in any order; zero gives zero; 49 I gives 7 I;
  * sqrt(S 2^k) = sqrt(S) 2^(k/2) BIT FOR BIT for k from -600 to +600 (the matrix is brought to max|S| in [1, 2) by a power of two before
    the first sweep; before that the squared-norm tests stopped the loop early below 2^-500 and returned NaN above 2^+500);
  * the bits of a matrix do not depend on the number of matrices in the call, on its place, or on a NaN matrix beside it; a NaN or Inf
    input comes back NaN with return code 0; bad arguments are RSREC_ERR_ARG and leave the handle usable.

Measured on an MI355X (the test prints every figure), worst device error / oracle error per class: exact integer roots 7.6 (the
spin-diagonal case, cond(B) = 5 400: device 9.5e-14, oracle 1.2e-14, bar 2.0e-13; every other case <= 1.8), prescribed spectra 1.8,
perturbed lower triangles 1.5.  The oracle is itself a cyclic Jacobi (row-cyclic order), so ratios near 1 are what to expect.  Device
forward errors: 2.8e-16 .. 7.4e-15 on the well-conditioned classes, 9.1e-13 on the real integer case (cond 7e5), 1.1e-13 / 5.7e-12 on the
spectra graded over 1e-8 / 1e-12; backward error <= 1.6e-14, asymmetry <= 8e-17.  Before the prescaling the device gave roots 3.6e-9 ..
6.8e-4 off at 2^-520, sqrt(diag S) (27 % .. 99 % off) at 2^-600, both with return code 0, and NaN at 2^+500 and 2^+600."""
import ctypes as C

import numpy as np
import pytest

import eig18_cases as EC
from rslmtoasa_amd import _lib

pytestmark = pytest.mark.gpu
FAMILIES = {"exact": EC.exact_cases, "diagonal": EC.diagonal_cases, "spectrum": EC.spectrum_cases_with_roots, "perturbed": EC.perturbed_cases}


class BareHandle:
    """A library handle that never sees a lattice or a Hamiltonian."""

    def __init__(self):
        self._L, self._h = _lib.lib(), C.c_void_p()
        assert self._L.rsrec_create(C.byref(self._h), 0) == 0

    def zsqr(self, mats):
        """sqrt of every matrix of (18, 18, n), all in one call; the input is left alone."""
        out = np.array(mats, dtype=np.complex128, order="F", copy=True)
        assert out.ndim == 3 and out.shape[:2] == (18, 18)
        assert self._L.rsrec_zsqr(self._h, out.shape[2], out.ctypes.data_as(C.c_void_p)) == 0
        return out

    def close(self):
        if self._h.value:
            self._L.rsrec_destroy(self._h)
            self._h = C.c_void_p()


@pytest.fixture(scope="module")
def handle():
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's (as bench.py does)
    torch.cuda.set_device(0)
    h = BareHandle()
    yield h
    h.close()


def stack(mats):
    return np.asfortranarray(np.stack(mats, axis=2))


@pytest.fixture(scope="module")
def solved(handle, oracle_lib):
    """{family: [(name, S, exact root, device root, oracle root)]}: one device call and one oracle call per family, left unchanged."""
    out = {}
    for fam, make in FAMILIES.items():
        cases = make()
        S = stack([c[1] for c in cases])
        dev, orc = handle.zsqr(S), oracle_lib.zsqr(S)
        rows = []
        for i, (name, s, b) in enumerate(cases):
            row = (name, s, b, dev[:, :, i].copy(), orc[:, :, i].copy())
            for a in row[1:]:
                a.setflags(write=False)
            rows.append(row)
        out[fam] = rows
    return out


@pytest.mark.parametrize("fam", ["exact", "spectrum", "perturbed"])
def test_forward_error_to_the_exact_root(fam, solved):
    worst, bad = 0.0, []
    for name, S, B, dev, orc in solved[fam]:
        e_dev, e_orc = EC.forward_error(dev, B), EC.forward_error(orc, B)
        bar = EC.forward_bar(e_orc)
        ratio = e_dev / e_orc if e_orc > 0 else (0.0 if e_dev == 0 else np.inf)
        print("forward %-10s %-20s device %.2e oracle %.2e ratio %6.2f bar %.2e" % (fam, name, e_dev, e_orc, ratio, bar))
        assert np.isfinite(e_orc)
        if e_orc > 0:
            worst = max(worst, ratio)
        if not e_dev <= bar:
            bad.append((name, e_dev, bar))
    print("forward %-10s worst device / oracle ratio %.2f" % (fam, worst))
    assert not bad, bad


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_backward_error_and_structure(fam, solved):
    bad = []
    for name, S, B, dev, orc in solved[fam]:
        if name == "zero":
            continue
        assert np.isfinite(dev).all(), name
        back, asym, neg = EC.structure_errors(dev, S)
        print("structure %-10s %-24s backward %.2e asymmetry %.2e -min eig %.2e" % (fam, name, back, asym, neg))
        if not (back <= EC.BACKWARD and asym <= EC.BACKWARD and neg <= EC.BACKWARD):
            bad.append((name, back, asym, neg))
    assert not bad, bad


def test_exits_before_the_first_sweep_are_exact(solved):
    for name, S, B, dev, orc in solved["diagonal"]:
        assert EC.same_bits(dev, B), name
    by = {r[0]: r for r in solved["diagonal"]}
    assert not by["zero"][3].any()
    assert np.array_equal(by["seven_squared_identity"][3], 7.0 * np.eye(18))
    # the same diagonal in another order: the same numbers, moved
    asc, desc = np.diagonal(by["diag_ascending"][3]), np.diagonal(by["diag_descending"][3])
    assert EC.same_bits(asc[::-1], desc)
    seven = [r for r in solved["exact"] if r[0] == "seven_identity"][0]
    assert EC.same_bits(seven[3], seven[2])


@pytest.fixture(scope="module")
def bases(handle):
    """(name, S, exact root, device root) of the three matrices the scale tests use; the roots from one call at k = 0."""
    cases = EC.scale_bases()
    dev = handle.zsqr(stack([c[1] for c in cases]))
    return [(n, S, B, dev[:, :, i].copy()) for i, (n, S, B) in enumerate(cases)]


def test_power_of_two_covariance_bit_for_bit(handle, bases):
    """|k| <= 480: the range in which the solver's sums of squares never left the normal numbers; these bits were the same before the
    prescaling and pin that it changed nothing there."""
    mats = [EC.scaled(S, k) for _, S, _, _ in bases for k in EC.SCALE_IN]
    out = handle.zsqr(stack(mats))
    bad = []
    for i, (name, S, B, r0) in enumerate(bases):
        assert np.isfinite(r0).all() and EC.forward_error(r0, B) < 1e-11
        for j, k in enumerate(EC.SCALE_IN):
            if not EC.same_bits(out[:, :, i * len(EC.SCALE_IN) + j], EC.scaled(r0, k // 2)):
                bad.append((name, k))
    assert not bad, bad


@pytest.mark.parametrize("k", EC.SCALE_OUT)
def test_power_of_two_beyond_the_range_of_the_squares(k, handle, bases, oracle_lib):
    """2^-600, 2^-520: nrm and off as plain sums of squares underflowed (the loop stopped after 0 / a few sweeps and a wrong root came back
    with return code 0); 2^+500, 2^+600: nrm overflowed and a finite matrix came back NaN.  Asked for: the covariant bits, or at least a
    root inside the forward bar; never NaN, never quietly wrong."""
    mats = stack([EC.scaled(S, k) for _, S, _, _ in bases])
    out, orc = handle.zsqr(mats), oracle_lib.zsqr(mats)
    bad = []
    for i, (name, S, B, r0) in enumerate(bases):
        r, want = out[:, :, i], EC.scaled(B, k // 2)
        assert np.isfinite(r).all(), (name, k)
        covariant = EC.same_bits(r, EC.scaled(r0, k // 2))
        e_dev, e_orc = EC.forward_error(r, want), EC.forward_error(orc[:, :, i], want)
        print("scale 2^%d %-10s covariant bits %s device %.2e oracle %.2e" % (k, name, covariant, e_dev, e_orc))
        assert np.isfinite(e_orc)
        if not (covariant or e_dev <= EC.forward_bar(e_orc)):
            bad.append((name, k, e_dev, EC.forward_bar(e_orc)))
    assert not bad, bad


def test_bits_do_not_depend_on_the_batch(handle, solved):
    rows = solved["spectrum"]
    S = stack([r[1] for r in rows])
    ref = stack([r[3] for r in rows])
    n = S.shape[2]
    assert EC.same_bits(handle.zsqr(S), ref)                                    # a second call
    assert EC.same_bits(handle.zsqr(S[:, :, ::-1])[:, :, ::-1], ref)            # reversed
    for i in (0, 7, n - 1):                                                     # alone
        assert EC.same_bits(handle.zsqr(S[:, :, i:i + 1])[:, :, 0], ref[:, :, i])
    # NaN and Inf matrices in between: they come back NaN (return code 0, as k_zsqr documents), their neighbours untouched
    mixed = np.asfortranarray(np.repeat(S, 2, axis=2))
    mixed[:, :, 1::2] = S
    poison = list(range(1, 2 * n, 2))
    for j, i in enumerate(poison):
        mixed[(3 * j) % 18, (5 * j + 1) % 18, i] = np.nan if j % 2 == 0 else np.inf
    mixed[:, :, poison[2]] = np.nan
    out = handle.zsqr(mixed)
    assert EC.same_bits(out[:, :, 0::2], ref)
    assert np.isnan(out[:, :, 1::2].real).all() and np.isnan(out[:, :, 1::2].imag).all()
    assert EC.same_bits(handle.zsqr(S), ref)                                    # and the handle is none the worse for it


def test_bad_arguments_give_errors(handle, solved):
    L, h = handle._L, handle._h
    name, S, B, dev, orc = solved["exact"][0]
    buf = np.array(S, dtype=np.complex128, order="F", copy=True)
    p = buf.ctypes.data_as(C.c_void_p)
    err = C.create_string_buffer(512)
    for args in ((h, -1, p), (h, 1, None), (h, 3, None)):
        assert L.rsrec_zsqr(*args) == _lib.ERR_ARG, args
        L.rsrec_last_error(h, err, 512)
        assert b"rsrec_zsqr" in err.value
        assert np.array_equal(buf, S)                                           # nothing was written
        assert EC.same_bits(handle.zsqr(S[:, :, None])[:, :, 0], dev)           # the handle is still usable
    assert L.rsrec_zsqr(None, 1, p) == _lib.ERR_ARG
    assert L.rsrec_zsqr(h, 0, None) == 0 and L.rsrec_zsqr(h, 0, p) == 0
    assert np.array_equal(buf, S)
