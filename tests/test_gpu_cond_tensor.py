"""The conductivity tail on the GPU (rsrec_kubo_conductivity, Conductivity.tensor: k_cond_series + k_cond_tensor) against its numpy
restatement (tests/cond_tensor_reference.py, itself pinned to the compiled reference's simpson_f by
tests/test_cond_tensor_restatement.py), on a handle with no lattice and no Hamiltonian.

  * T = 0: series and sigma equal the restatement bit for bit -- the weights are exactly 1, 0.5 and 0 and the order of the sums is the
    reference's;
  * T > 0 (kBT about three mesh steps, the fixture's value): |dev - ref| <= 16 2^-52 (H / 3) sum |c_k y_k f_k| per element -- the two
    exp implementations differ by a few ulp and the weight inherits that relatively; everything else is the same sequence of operations;
  * the same bits from a host array and a GPU tensor, into host arrays and GPU tensors, from two calls, and for a set computed alone
    and inside a per_vector call;
  * resident diagonal moments survive the call; every refusal is RSREC_ERR_ARG and leaves the handle usable.

Shapes (nen, nv1): the four of the fixture (nv1 odd and even; nen = nv1 + 9, where the term past the mesh is zero, and nen = nv1 + 12,
where it is the mesh's own), one mesh of the reference's size (2510 limits, five weight tiles), one call of 1178 columns (two column
blocks per limit)."""
import ctypes as C

import numpy as np
import pytest

import cond_tensor_reference as CT
from cond_reference import scaling
from helpers import load_golden
from rslmtoasa_amd import _lib
from rslmtoasa_amd.conductivity import Conductivity
from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion

pytestmark = pytest.mark.gpu
EMIN, EMAX = -0.8, 0.6
EPS = 2.0 ** -52
SHAPES = [(12, 3), (31, 22), (32, 23), (35, 23)]
CASES = [(nen, nv1, nvec, pv) for nen, nv1 in SHAPES for nvec in (1, 3) for pv in (0, 1)] + [(2510, 2501, 3, 1), (32, 23, 30, 1)]


class BareHandle:
    """What Conductivity needs of a recursion object, on a handle that never sees a lattice or a Hamiltonian."""
    _check, timing = Recursion._check, Recursion.timing

    def __init__(self, en):
        self.en, self._L, self._h = en, _lib.lib(), C.c_void_p()
        rc = self._L.rsrec_create(C.byref(self._h), 0)
        assert rc == 0

    def close(self):
        if self._h.value:
            self._L.rsrec_destroy(self._h)
            self._h = C.c_void_p()


@pytest.fixture(scope="module")
def cond():
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's (as bench.py does)
    torch.cuda.set_device(0)
    rec = BareHandle(Energy(EMIN, EMAX))
    yield Conductivity(rec)
    rec.close()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.ravel(a, order="K").view(np.float64), np.ravel(b, order="K").view(np.float64))


def mesh(nen, nv1):
    """(ene, T): ene whose scaled axis is the fixture's x of that shape (to rounding) and the fixture's T; for the large mesh a uniform
    axis inside (-1, 1) and the T whose kBT is three of its steps."""
    a, b = scaling(EMIN, EMAX)
    g = load_golden("cond_tensor_simpson")
    s = "%d_%d" % (nen, nv1)
    if "x_" + s in g:
        return b + a * g["x_" + s], float(g["T_" + s])
    h = 1.9 / nen
    return b + a * (-0.95 + h * np.arange(nen)), 3.0 * h / CT.KB


def integrand(nen, nvec, seed):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((18, nen, nvec)) + 1j * rng.standard_normal((18, nen, nvec))) * 10.0 ** rng.uniform(-3, 3, (18, nen, nvec))
    return np.asfortranarray(z)


def to_device(z):
    """The Fortran array (18, nen, nvec) as a C-order GPU tensor (nvec, nen, 18)."""
    import torch
    t = torch.from_numpy(np.array(z.transpose(2, 1, 0), order="C")).cuda()          # (a writable copy)
    torch.cuda.synchronize()
    return t


def scaled_T(T):
    """What Conductivity.tensor hands the library for the physical temperature T a: (T a) / a, formed the same way."""
    a, _ = scaling(EMIN, EMAX)
    return float(T * a) / a


@pytest.fixture(scope="module")
def reference():
    """Inputs and restatement of a case, computed once and left unchanged."""
    cache = {}

    def get(nen, nv1, nvec, pv):
        key = (nen, nv1, nvec, pv)
        if key not in cache:
            ene, T = mesh(nen, nv1)
            z = integrand(nen, nvec, 1000 * nen + 10 * nvec + pv)
            x = CT.scaled_axis(ene, EMIN, EMAX)
            S = CT.series(z, bool(pv))
            Ts = scaled_T(T)
            out = dict(ene=ene, T=T, z=z, S=S, sigma0=CT.tensor(S, x, nv1, 0.0), sigmaT=CT.tensor(S, x, nv1, Ts), absT=CT.tensor_abs(S, x, nv1, Ts))
            for v in out.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            cache[key] = out
        return cache[key]
    return get


@pytest.mark.parametrize("nen,nv1,nvec,pv", CASES)
def test_tensor_matches_restatement(nen, nv1, nvec, pv, cond, reference):
    r = reference(nen, nv1, nvec, pv)
    a, _ = scaling(EMIN, EMAX)
    sigma, ser = cond.tensor(r["z"], r["ene"], nv1=nv1, per_vector=bool(pv), series=True)
    nsets = 1 + (nvec if pv else 0)
    assert sigma.shape == (38, nen, nsets) and ser.shape == sigma.shape and sigma.flags.f_contiguous
    assert np.isfinite(r["sigma0"]).all() and np.abs(r["sigma0"]).max() > 0
    assert same_bits(ser, r["S"])
    assert same_bits(sigma, r["sigma0"])
    hot = cond.tensor(r["z"], r["ene"], nv1=nv1, per_vector=bool(pv), temperature=r["T"] * a)
    bound = 16 * EPS * r["absT"]
    err = np.abs(hot - r["sigmaT"])
    print("tensor T>0", (nen, nv1, nvec, pv), "max err / bound", (err / np.maximum(bound, 1e-300)).max(), "max |sigma|", np.abs(r["sigmaT"]).max())
    assert np.abs(r["sigmaT"] - r["sigma0"]).max() > 0                  # (the temperature reached the kernel)
    assert (err <= bound).all()
    total, kernels = cond.timing()
    assert total > 0 and 0 < kernels <= total


def test_default_nv1_is_the_reference_mesh(cond, reference):
    r = reference(31, 22, 3, 1)
    assert same_bits(cond.tensor(r["z"], r["ene"], per_vector=True), r["sigma0"])             # nv1 = len(ene) - 9
    assert same_bits(cond.tensor(r["z"][:, :, 0], r["ene"]), cond.tensor(r["z"][:, :, :1], r["ene"]))   # (18, nen): one vector


@pytest.mark.parametrize("nen,nv1,nvec", [(35, 23, 3), (2510, 2501, 3)])
def test_host_and_device_memory_same_bits(nen, nv1, nvec, cond, reference):
    import torch
    r = reference(nen, nv1, nvec, 1)
    a, _ = scaling(EMIN, EMAX)
    zd = to_device(r["z"])
    for T in (0.0, r["T"] * a):
        host = cond.tensor(r["z"], r["ene"], nv1=nv1, per_vector=True, temperature=T, series=True)
        dev = cond.tensor(zd, r["ene"], nv1=nv1, per_vector=True, temperature=T, series=True)
        again = cond.tensor(zd, r["ene"], nv1=nv1, per_vector=True, temperature=T, series=True)
        assert same_bits(host[0], dev[0]) and same_bits(host[1], dev[1])
        assert same_bits(dev[0], again[0]) and same_bits(dev[1], again[1])
    # outputs in GPU memory: the C ABI takes them where they lie
    rec = cond.recursion
    sig = torch.zeros((1 + nvec, nen, 38), dtype=torch.float64, device="cuda")
    ser = torch.zeros_like(sig)
    torch.cuda.synchronize()
    ene = np.ascontiguousarray(r["ene"])
    rec._check(rec._L.rsrec_kubo_conductivity(rec._h, nvec, 1, nen, nv1, ene.ctypes.data_as(C.c_void_p), EMIN, EMAX, 0.0, C.c_void_p(zd.data_ptr()),
                                              C.c_void_p(sig.data_ptr()), C.c_void_p(ser.data_ptr())))
    torch.cuda.synchronize()
    assert same_bits(np.asfortranarray(sig.cpu().numpy().transpose(2, 1, 0)), r["sigma0"])
    assert same_bits(np.asfortranarray(ser.cpu().numpy().transpose(2, 1, 0)), r["S"])


def test_a_set_does_not_depend_on_the_other_vectors(cond, reference):
    r = reference(35, 23, 3, 1)
    a, _ = scaling(EMIN, EMAX)
    for T in (0.0, r["T"] * a):
        joint, jser = cond.tensor(r["z"], r["ene"], nv1=23, per_vector=True, temperature=T, series=True)
        for v in range(3):
            alone, aser = cond.tensor(r["z"][:, :, v:v + 1], r["ene"], nv1=23, per_vector=True, temperature=T, series=True)
            assert same_bits(alone[:, :, 1], joint[:, :, 1 + v]) and same_bits(aser[:, :, 1], jser[:, :, 1 + v])
            assert np.array_equal(alone[:, :, 0], joint[:, :, 1 + v])         # the sum over one vector is that vector


def test_resident_moments_survive_the_call(reference):
    """rsrec_kubo_moments_diag leaves the diagonal moments of a small cell on the handle; a tensor call in between must not take them."""
    import rslmtoasa_amd.recursion as Rm
    z = load_golden("fccPt_kubo")
    a, b = float(z["acheb"]), float(z["bcheb"])
    half = a * float(np.float32(2) - np.float32(0.3)) / 2
    ham = Hamiltonian(ee=z["ee"], lsham=z["lsham"], hoh=False)
    lat = Lattice(nn=z["nn"], iz=z["iz"], irec=np.asarray(z["atlist"], np.int32), nmax=0, ntype=z["ee"].shape[3])
    rec = Recursion(ham, lat, Control(lld=int(z["cond_ll"]), nsp=int(z["nsp"])), Energy(b - half, b + half), device=0)
    orig = Rm.chebyshev_scaling
    Rm.chebyshev_scaling = lambda e0, e1: (a, b)
    try:
        L = int(z["cond_ll"])
        assert rec.compute_moments_stochastic(z["v_a"], z["v_b"], L, atlist=z["atlist"], diag=True, resident_only=True) is None
        cond = Conductivity(rec)
        ene = b - half + (2 * half / 300) * np.arange(310)                  # channels_ldos = 300: nen = 310, nv1 = 301, |x| < 1 throughout
        before = cond.integrand(None, ene)
        assert np.isfinite(before).all() and np.abs(before).max() > 0
        sigma, ser = cond.tensor(before, ene, per_vector=True, series=True)
        S = CT.series(before, True)
        assert same_bits(ser, S)
        assert same_bits(sigma, CT.tensor(S, CT.scaled_axis(ene, b - half, b + half), 301))
        after = cond.integrand(None, ene)
        assert same_bits(before, after)
    finally:
        Rm.chebyshev_scaling = orig
        rec.close()


def test_bad_arguments_give_errors(cond, reference):
    rec = cond.recursion
    L = _lib.lib()
    r = reference(12, 3, 1, 0)
    ene, z = np.ascontiguousarray(r["ene"]), r["z"]
    sigma = np.zeros((38, 12, 1), order="F")
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    good = (rec._h, 1, 0, 12, 3, p(ene), EMIN, EMAX, 0.0, p(z), p(sigma), None)

    def with_(**kw):
        names = ("h", "nvec", "per_vector", "nen", "nv1", "ene", "emin", "emax", "T", "integrand", "sigma", "series")
        return tuple(kw.get(n, g) for n, g in zip(names, good))

    bad = [with_(nvec=0), with_(nvec=-1), with_(nen=2, nv1=1), with_(nv1=0), with_(nv1=4), with_(nen=11), with_(emin=EMAX), with_(emin=0.7, emax=-0.8),
           with_(emin=float("nan")), with_(emax=float("inf")), with_(T=-1.0), with_(T=float("nan")), with_(T=float("inf")), with_(ene=None),
           with_(integrand=None), with_(sigma=None)]
    buf = C.create_string_buffer(512)
    for args in bad:
        assert L.rsrec_kubo_conductivity(*args) == _lib.ERR_ARG, args
        L.rsrec_last_error(rec._h, buf, 512)
        assert b"rsrec_kubo_conductivity" in buf.value
        assert L.rsrec_kubo_conductivity(*good) == 0                       # the handle is still usable
        assert same_bits(sigma, r["sigma0"])
    assert L.rsrec_kubo_conductivity(*with_(h=None)) == _lib.ERR_ARG
    with pytest.raises(_lib.RsrecError):
        cond.tensor(z, ene, nv1=4)
    with pytest.raises(_lib.RsrecError):
        cond.tensor(z, ene, nv1=3, temperature=-300.0)
    with pytest.raises(ValueError):
        cond.tensor(z[:, :11], ene)
    assert same_bits(cond.tensor(z, ene, nv1=3), r["sigma0"])
