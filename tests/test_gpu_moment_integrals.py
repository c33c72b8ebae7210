"""The integrals behind the SCF spectra on the device (rsrec_spectra_integrals, Green.spectra_integrals; kernels_moments.hpp) against
the numpy restatement tests/moment_reference.py, which tests/test_moment_restatement.py ties to the compiled reference.

cum: bit for bit against the restatement evaluated LIMIT BY LIMIT (the whole rule with the Fermi weights of every limit) -- the kernels
form a prefix and finish it per limit.
mom: bit for bit as well, for nexp = 0, 1, 2 and with and without the end term: kernel and restatement run the same sequence of IEEE
operations -- the products y E^p and (4 y) E^p with E^0 = 1, E^1 = E, E^2 = E E, the sum ((A + t0) + t1) + t2 triple by triple, H A / 3,
then A + (EF - EA) ((t + t) + t) / 6 -- without contraction.  Bit equality implies the recursive-sum bound of the restatement test.

Widths named here: MI_WIDTH = 256 (series, energy) pairs per workgroup of k_moment_cum and threads per workgroup everywhere;
MI_CHUNK = 16 triples a serial thread stages at a time (k_moment_prefix, k_moment_fermi)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import moment_reference as MR
from helpers import load_golden, objects_from, problem_dict
from rslmtoasa_amd import _lib, bands
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.recursion import Recursion
from test_gpu_green import load_green

pytestmark = pytest.mark.gpu

MI_WIDTH = 256
MI_CHUNK = 16


class BareHandle(Recursion):
    """A library handle with neither lattice nor Hamiltonian: all the call needs when the image is passed in."""

    def __init__(self, device=0):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        rc = self._L.rsrec_create(C.byref(self._h), device)
        if rc != 0:
            raise _lib.RsrecError(rc, "rsrec_create failed")


@pytest.fixture(scope="module")
def bare():
    h = BareHandle()
    yield h
    h.close()


def mesh(nen, lo=-0.93, width=1.7):
    return lo + (width / nen) * np.arange(nen)


def image(rng, nop, nen, ntot):
    spec = rng.standard_normal((nop, nen, ntot)) * 10.0 ** rng.uniform(-3, 3, (nop, nen, ntot))
    return np.asfortranarray(spec)


def fermi_args(ene, npts, above):
    """edel, e1, fermi of a Fermi level `above` mesh steps over point npts (1-based); above = 0: e1 == fermi, no end term"""
    edel = float(ene[1] - ene[0])
    e1 = float(ene[npts - 1])
    return edel, e1, e1 + above * edel


def run(h, ene, nv1, npts, above, spec, comb=None, nsites=None, site_offset=0, **kw):
    edel, e1, fermi = fermi_args(ene, npts, above)
    return Green(h, ene).spectra_integrals(nv1, npts, edel, e1, fermi, spec=spec, comb=comb, nsites=nsites, site_offset=site_offset, **kw)


def expect(ene, nv1, npts, above, spec, comb=None):
    edel, e1, fermi = fermi_args(ene, npts, above)
    return MR.integrals(spec, comb, ene, nv1, npts, edel, e1, fermi)


# (nen, nv1): both parities of the stray element (nen = nv1 + 9); a mesh that extends past the rule (nen = nv1 + 12); one pair below, at
# and above MI_WIDTH with nser = 1; ntrip = (nv1 + 9) // 2 one below, at and above MI_CHUNK
CUM_MESHES = [(10, 1), (11, 2), (14, 2), (35, 23), (MI_WIDTH - 1, MI_WIDTH - 10), (MI_WIDTH, MI_WIDTH - 9), (MI_WIDTH + 1, MI_WIDTH - 8),
              (30, 21), (32, 23), (34, 25)]


@pytest.mark.parametrize("nen,nv1", CUM_MESHES)
def test_cumulative_integrals_carry_the_bits_of_the_rule_limit_by_limit(nen, nv1, bare):
    rng = np.random.default_rng(nen * 1000 + nv1)
    ene = mesh(nen)
    spec = image(rng, 1, nen, 1)
    mom, cum = run(bare, ene, nv1, 3, 0.37, spec)
    rmom, rcum = expect(ene, nv1, 3, 0.37, spec)
    assert cum.shape == (1, nen, 1) and np.isfinite(cum).all() and np.abs(cum).max() > 0
    assert np.array_equal(cum, rcum), np.abs(cum - rcum).max()
    assert np.array_equal(mom, rmom)
    assert bare.timing()["total_ms"] > 0


def test_leading_zeros_and_a_sign_change_at_the_limit(bare):
    """A series that is zero up to a point (the running sum stays +0), one whose sign changes between two limits, one of alternating
    sign, and one that is -0.0 throughout; 21 series over 3 sites cross MI_WIDTH many times."""
    nen, nv1 = 41, 29
    rng = np.random.default_rng(2)
    ene = mesh(nen)
    spec = image(rng, 21, nen, 3)
    k = np.arange(nen)
    spec[0, :17, :] = 0.0
    spec[1] = np.abs(spec[1]) * np.where(k < 20, 1.0, -1.0)[:, None]
    spec[2] = np.abs(spec[2]) * np.where(k % 2 == 0, 1.0, -1.0)[:, None]
    spec[3] = -0.0
    for npts in (19, 20, 21):
        mom, cum = run(bare, ene, nv1, npts, 0.5, spec)
        rmom, rcum = expect(ene, nv1, npts, 0.5, spec)
        assert np.array_equal(cum, rcum) and np.array_equal(mom, rmom)
    assert not cum[0, :17].any() and cum[0, 18:].all() and not cum[3].any()
    assert (cum[1, 1:20] > 0).all() and (np.diff(cum[1, 21:nv1 + 9, 0]) < 0).all()      # (limits past the rule's last point add nothing)


@pytest.mark.parametrize("above", [0.0, 0.37])
def test_fermi_level_integrals(above, bare):
    """nv1_fermi = 1, 2 (empty main loop), 3 (one pass), MI_CHUNK-sized loops and nen - 2; e1 == fermi (no end term) and e1 /= fermi;
    every nexp.  Bit for bit (module docstring)."""
    nen, nv1 = 80, 71
    rng = np.random.default_rng(7)
    ene = mesh(nen, lo=-1.1, width=1.9)                       # crosses zero: E^1 changes sign
    spec = image(rng, 5, nen, 2)
    for npts in (1, 2, 3, 2 * MI_CHUNK - 1, 2 * MI_CHUNK + 1, 2 * MI_CHUNK + 3, nen - 2):
        mom, _ = run(bare, ene, nv1, npts, above, spec, want=("mom",))
        rmom, _ = expect(ene, nv1, npts, above, spec)
        assert mom.shape == (3, 5, 2) and np.isfinite(mom).all()
        if npts < 3 and above == 0.0:
            assert not mom.any()
        else:
            assert mom.all()
        assert np.array_equal(mom, rmom), (npts, np.abs(mom - rmom).max())
        edel, e1, fermi = fermi_args(ene, npts, above)
        for p in range(3):
            for s in range(2):
                bound = MR.n_terms_m(npts) * 2.0 ** -52 * MR.simpson_m_abs(edel, fermi, npts, spec[:, :, s], e1, p, ene)
                assert (np.abs(mom[p, :, s] - rmom[p, :, s]) <= bound).all()


@pytest.mark.parametrize("nop,nser", [(1, 1), (32, 21), (32, 1), (1, 21), (15, 64)])
def test_series_shapes(nop, nser, bare):
    """nser 1 and 21 (and the largest, whose 64 x 5 serial threads cross MI_WIDTH), nop 1 and 32, a dense comb per site."""
    nen, nv1, ns = 23, 12, 5 if nser == 64 else 2
    rng = np.random.default_rng(nop * 100 + nser)
    ene = mesh(nen)
    spec = image(rng, nop, nen, ns)
    comb = np.asfortranarray(rng.standard_normal((nop, nser, ns)))
    mom, cum = run(bare, ene, nv1, 9, 0.2, spec, comb)
    rmom, rcum = expect(ene, nv1, 9, 0.2, spec, comb)
    assert mom.shape == (3, nser, ns) and cum.shape == (nser, nen, ns)
    assert np.array_equal(cum, rcum) and np.array_equal(mom, rmom)


def test_no_comb_is_the_identity_table(bare):
    nen, nv1, nop = 29, 20, 6
    rng = np.random.default_rng(3)
    ene = mesh(nen)
    spec = image(rng, nop, nen, 2)
    eye = np.asfortranarray(np.repeat(np.eye(nop)[:, :, None], 2, axis=2))
    a = run(bare, ene, nv1, 11, 0.4, spec)
    b = run(bare, ene, nv1, 11, 0.4, spec, eye)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.abs(a[1]).max() > 0


@pytest.mark.parametrize("ns", [1, 3])
def test_images_are_zero_padded(ns, bare):
    """nsites 1 and 3 at site_offset = 2 of nsites_total = 6: the sites' columns carry the bits of the offset-0 call on their slab, every
    other column is exactly zero; the columns of the image outside the slab are not read (they hold NaN)."""
    nen, nv1, off, ntot = 19, 10, 2, 6
    rng = np.random.default_rng(ns)
    ene = mesh(nen)
    slab = image(rng, 4, nen, ns)
    comb = np.asfortranarray(rng.standard_normal((4, 3, ns)))
    spec = np.full((4, nen, ntot), np.nan, order="F")
    spec[:, :, off:off + ns] = slab
    mom, cum = run(bare, ene, nv1, 7, 0.1, spec, comb, nsites=ns, site_offset=off)
    lmom, lcum = run(bare, ene, nv1, 7, 0.1, slab, comb)
    assert mom.shape == (3, 3, ntot) and cum.shape == (3, nen, ntot)
    assert np.array_equal(mom[:, :, off:off + ns], lmom) and np.array_equal(cum[:, :, off:off + ns], lcum) and lcum.all()
    mask = np.ones(ntot, bool); mask[off:off + ns] = False
    assert np.all(mom[:, :, mask] == 0) and np.all(cum[:, :, mask] == 0)
    only_cum = run(bare, ene, nv1, 7, 0.1, spec, comb, nsites=ns, site_offset=off, want=("cum",))
    assert only_cum[0] is None and np.array_equal(only_cum[1], cum)


def make_rec(name):
    g = load_golden(name)
    return Recursion(*objects_from(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"], emin=g["emin"], emax=g["emax"]), device=0), load_green(name)


@pytest.mark.parametrize("name,recur,call", [("fccCu001_block_hoh", "recur_b", "block_spectra"), ("fccCu001_cheb", "chebyshev_recur", "chebyshev_spectra")])
def test_resident_image(name, recur, call):
    """spec = NULL after a spectra call gives the bits of passing that call's output; twice the same; an LDOS stage in between leaks
    nothing; an image of another shape is refused and the next call succeeds."""
    rec, z = make_rec(name)
    getattr(rec, recur)()
    ene = np.ascontiguousarray(z["ene"])
    nen, n, off, ntot = len(ene), 2, 1, 4
    nv1, npts = nen - 9, nen // 2
    gr = Green(rec, ene)
    ops = bands.stack(bands.SCF_OPERATORS)
    mom_dir = np.array([[0.0, 0.6], [0.0, 0.0], [1.0, 0.8]])
    comb, names = bands.series_table(mom_dir)
    edel, e1, fermi = fermi_args(ene, npts, 0.3)
    args = (nv1, npts, edel, e1, fermi)
    with pytest.raises(_lib.RsrecError, match="no spectra image resident"):
        gr.spectra_integrals(*args, comb=comb, nop=15, site_offset=off, nsites_total=ntot)
    spec = getattr(gr, call)(ops, site_offset=off, nsites_total=ntot)
    res = gr.spectra_integrals(*args, comb=comb, nop=15, site_offset=off, nsites_total=ntot)
    t = rec.timing()
    again = gr.spectra_integrals(*args, comb=comb, nop=15, site_offset=off, nsites_total=ntot)
    (gr.block_ldos if recur == "recur_b" else gr.chebyshev_ldos)(site_offset=off, nsites_total=ntot)
    after = gr.spectra_integrals(*args, comb=comb, nop=15, site_offset=off, nsites_total=ntot)
    given = gr.spectra_integrals(*args, spec=spec, comb=comb, nsites=n, site_offset=off)
    for kw in (dict(nop=14, site_offset=off, nsites_total=ntot), dict(nop=15, site_offset=0, nsites_total=ntot), dict(nop=15, site_offset=off, nsites_total=ntot + 1)):
        with pytest.raises(_lib.RsrecError, match="resident image"):
            gr.spectra_integrals(*args, comb=None if kw["nop"] == 14 else comb, **kw)
    with pytest.raises(_lib.RsrecError, match="resident image"):
        Green(rec, ene[:-1]).spectra_integrals(nv1 - 1, npts, edel, e1, fermi, comb=comb, nop=15, site_offset=off, nsites_total=ntot)
    last = gr.spectra_integrals(*args, comb=comb, nop=15, site_offset=off, nsites_total=ntot)
    getattr(rec, recur)()                                        # a new recursion drops the image with the chains
    with pytest.raises(_lib.RsrecError, match="no spectra image resident"):
        gr.spectra_integrals(*args, comb=comb, nop=15, site_offset=off, nsites_total=ntot)
    rec.close()
    assert t["total_ms"] > 0 and res[0].shape == (3, 12, ntot) and res[1].shape == (12, nen, ntot) and np.abs(res[1][:, :, off:off + n]).max() > 0
    ref = MR.integrals(spec[:, :, off:off + n], comb, ene, nv1, npts, edel, e1, fermi)
    for r in (res, again, after, given, last):
        assert np.array_equal(r[0][:, :, off:off + n], ref[0]) and np.array_equal(r[1][:, :, off:off + n], ref[1])
        assert not r[0][:, :, 0].any() and not r[1][:, :, 0].any() and not r[1][:, :, 3].any()


def raw_call(h, nop, nser, nen, nv1, npts, edel, e1, fermi, nsites=1, off=0, ntot=1, spec=True, comb=False, mom=True, cum=True, ene=None):
    ene = mesh(max(nen, 2)) if ene is None else ene
    s = np.ones((max(nop, 1), max(nen, 1), ntot), order="F")
    c = np.ones((max(nop, 1), max(nser, 1), nsites), order="F")
    m, q = np.zeros((3, max(nser, 1), ntot), order="F"), np.zeros((max(nser, 1), max(nen, 1), ntot), order="F")
    p = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None
    rc = h._L.rsrec_spectra_integrals(h._h, nop, p(s, spec), nser, p(c, comb), nen, p(ene, True), nv1, npts, edel, e1, fermi, nsites, off, ntot, p(m, mom), p(q, cum))
    buf = C.create_string_buffer(512)
    h._L.rsrec_last_error(h._h, buf, 512)
    return rc, buf.value.decode(), m, q


def test_argument_errors_leave_the_handle_usable(bare):
    ok = dict(nop=3, nser=3, nen=20, nv1=11, npts=9, edel=0.1, e1=-0.2, fermi=-0.15)
    rc, _, m0, q0 = raw_call(bare, **ok)
    assert rc == 0 and q0.all()
    bad_mesh = mesh(20).copy(); bad_mesh[7] = bad_mesh[6]
    cases = [("nothing resident", dict(spec=False), "no spectra image resident"),
             ("nen < nv1 + 9", dict(nv1=12), "nv1 \\+ 9"),
             ("nv1_fermi + 2 > nen", dict(npts=19), "nv1_fermi"),
             ("nv1_fermi < 1", dict(npts=0), "nv1_fermi"),
             ("edel", dict(edel=float("nan")), "finite"), ("e1", dict(e1=float("inf")), "finite"), ("fermi", dict(fermi=float("-inf")), "finite"),
             ("nop = 0", dict(nop=0), "nop"), ("nop = 33", dict(nop=33), "nop"),
             ("nser = 0", dict(nser=0, comb=True), "nser"), ("nser = 65", dict(nser=65, comb=True), "nser"),
             ("nser /= nop without comb", dict(nser=2), "comb"),
             ("no output", dict(mom=False, cum=False), "bad argument"),
             ("sites outside the image", dict(nsites=2, off=1, ntot=2), "outside"),
             ("mesh", dict(ene=bad_mesh), "ascend")]
    for what, change, msg in cases:
        rc, err, _, _ = raw_call(bare, **dict(ok, **change))
        assert rc == _lib.ERR_ARG and re.search(msg, err), (what, rc, err)
        rc, _, m, q = raw_call(bare, **ok)
        assert rc == 0 and np.array_equal(m, m0) and np.array_equal(q, q0), what


DEVICE_SCRIPT = r"""
import sys, numpy as np, torch
torch.cuda.init(); torch.cuda.set_device(0)          # torch's HIP runtime first, as in bench.py
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from rslmtoasa_amd.green import Green
from test_gpu_moment_integrals import BareHandle, fermi_args, image, mesh
h = BareHandle()
rng = np.random.default_rng(4)
nop, nser, nen, nv1, n, off, ntot, npts = 7, 5, 300, 291, 2, 1, 4, 141
ene = mesh(nen)
spec = image(rng, nop, nen, ntot)
comb = np.asfortranarray(rng.standard_normal((nop, nser, n)))
edel, e1, fermi = fermi_args(ene, npts, 0.3)
gr = Green(h, ene)
kw = dict(nsites=n, site_offset=off)
hm, hc = gr.spectra_integrals(nv1, npts, edel, e1, fermi, spec=spec, comb=comb, **kw)
assert np.abs(hc[:, :, off:off + n]).max() > 0 and not hc[:, :, 0].any()
t_spec = torch.from_numpy(np.ascontiguousarray(spec.transpose(2, 1, 0))).cuda()      # Fortran (nop, nen, ntot)
t_comb = torch.from_numpy(np.ascontiguousarray(comb.transpose(2, 1, 0))).cuda()
t_mom = torch.full((ntot, nser, 3), -1.0, dtype=torch.float64, device="cuda")
t_cum = torch.full((ntot, nen, nser), -1.0, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
for s, c in ((t_spec, t_comb), (spec, t_comb), (t_spec, comb)):
    for out in ((t_mom.data_ptr(), t_cum.data_ptr()), (None, t_cum.data_ptr()), (t_mom.data_ptr(), None), None):
        t_mom.fill_(-1.0); t_cum.fill_(-1.0); torch.cuda.synchronize()
        m, q = gr.spectra_integrals(nv1, npts, edel, e1, fermi, spec=s, comb=c, nop=nop, nsites_total=ntot, out=out, **kw)
        m = t_mom.cpu().numpy().transpose(2, 1, 0) if out is not None and out[0] is not None else m
        q = t_cum.cpu().numpy().transpose(2, 1, 0) if out is not None and out[1] is not None else q
        assert np.array_equal(m, hm) and np.array_equal(q, hc)
h.close()
print("DEVICE_MEMORY_OK")
"""


def test_device_memory_gives_the_bits_of_host_memory():
    """spec, comb, mom and cum in device memory (tensors of another HIP runtime of the process), in every mixture with host arrays.  Own
    process: torch's HIP runtime has to be initialised before librsrec's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT, root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE_MEMORY_OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
