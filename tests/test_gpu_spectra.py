"""Operator spectra of the on-site Green function on the device (rsrec_block_spectra / rsrec_chebyshev_spectra, Green.block_spectra /
Green.chebyshev_spectra): spec(k, ie, s) = Im Tr(O_k g0(:,:,ie,s)) from the chains the recursion left on the GPU, no g0 formed.

Checkers: (1) numpy traces of the g0 the library's own Green kernels return for the same chains (device against device); (2) numpy
traces of the compiled reference's g0 (tests/golden/*_green.npz, every 40th energy of its mesh).

Bounds, per operator k, with q_k = the checker's values and terms_k = the largest sum_ij |O_k(j,i)| |g0(i,j)| (the size of what the
trace adds up):
  (1)  max(1e-12 largest |q_k|, 1e-13 terms_k): 1e-12 of the operator's largest value (tests/test_fortran_dropin.py's device-against-device
       bar); the second term is the rounding error any re-ordered sum of 324 products may have, 323 eps terms = 3.6e-14 terms, which is
       all there is where the trace vanishes by symmetry (d_x, d_y, L of collinear runs without spin-orbit coupling: noise on both sides);
  (2)  1e-10 sum_ij |O_k(j,i)| max|g0|: g0 itself agrees with the reference to 1e-10 of its largest element, element by element
       (test_gpu_green.py's bar; the spin-off-diagonal blocks of a collinear run are such noise, 1e-10 of the diagonal, in either code),
       which moves a trace by at most that times the operator's absolute sum.
Every case runs the fixtures' own sizes (1 to 5 sites, lld 20, 63 energies)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import load_golden, objects_from, problem_dict
from rslmtoasa_amd import _lib, bands
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.recursion import Recursion
from test_gpu_green import GREEN_CASES, base_case, load_green

pytestmark = pytest.mark.gpu

CHEB_CASES = ["bccFe_nsp2_cheb", "fccCu001_cheb"]
GREEN_WAVES = 4                                   # (site, energy) pairs per workgroup of the block kernel (kernels_green.hpp)
OPS21 = bands.stack(bands.ALL_OPERATORS)


def ops32():
    """The 21 named operators and 11 dense complex ones: the largest set a call takes."""
    rng = np.random.default_rng(11)
    extra = rng.normal(size=(11, 18, 18)) + 1j * rng.normal(size=(11, 18, 18))
    return np.concatenate([OPS21, extra])


def terms(ops, g0):
    return np.einsum("kji,ijes->kes", np.abs(ops), np.abs(g0)).max(axis=(1, 2))


def check(spec, ops, g0_dev, g0_ref, what):
    """The two comparisons of the module docstring; prints every figure before it asserts."""
    assert np.isfinite(spec).all() and spec.shape == (len(ops),) + g0_dev.shape[2:]
    q1, t1 = bands.traces(ops, g0_dev), terms(ops, g0_dev)
    e1, s1 = np.abs(spec - q1).max(axis=(1, 2)), np.abs(q1).max(axis=(1, 2))
    b1 = np.maximum(1e-12 * s1, 1e-13 * t1)
    print("%s vs own g0: worst err/bound %.3f (err %.3e)" % (what, (e1 / b1).max(), e1.max()))
    assert (e1 <= b1).all(), (what, e1, b1)
    if g0_ref is not None:
        q2, t2 = bands.traces(ops, g0_ref), np.abs(ops).sum(axis=(1, 2)) * np.abs(g0_ref).max()
        e2 = np.abs(spec - q2).max(axis=(1, 2))
        print("%s vs reference g0: worst err/scale %.3e" % (what, (e2 / t2).max()))
        assert (e2 <= 1e-10 * t2).all(), (what, e2, t2)


def make_rec(g):
    return Recursion(*objects_from(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"], emin=g["emin"], emax=g["emax"]), device=0)


_block = {}


def block_run(name):
    """One recursion per case, shared: the spectra of the 21 operators, the LDOS images, and g0 from rsrec_block_green for the same
    coefficients and the device's terminators."""
    if name not in _block:
        z, g = load_green(name), load_golden(base_case(name))
        rec = Recursion(*objects_from(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"]), device=0)
        rec.recur_b()
        n = int(z["nrec"])
        gr = Green(rec, z["ene"], sym_term=bool(z["sym_term"]))
        spec = gr.block_spectra(OPS21)
        again = gr.block_spectra(OPS21)
        ldos = gr.block_ldos()
        rec.zsqr()
        g0 = gr.block_green(ldos["a_inf"], ldos["b_inf"], nsites=n).copy()
        rec.close()
        _block[name] = dict(z=z, spec=spec, again=again, ldos=ldos, g0=g0)
    return _block[name]


@pytest.mark.parametrize("name", GREEN_CASES)
def test_block_spectra(name):
    """recur_b, then ONE call for the 21 operators, against both checkers; a second call gives the same bits."""
    r = block_run(name)
    check(r["spec"], OPS21, r["g0"], r["z"]["g0"], name)
    assert np.array_equal(r["spec"], r["again"])
    if name == "bccFe_nsp4_block":                 # the L rows carry signal here (spin-orbit coupling)
        assert np.abs(r["spec"][bands.ALL_OPERATORS.index("Lz")]).max() > 1e-3


@pytest.mark.parametrize("name", ["bccFe_nsp4_block", "fccCu001_block_hoh"])
def test_block_spectra_of_unit_operators_is_the_ldos(name):
    """The 18 diagonal unit operators give Im g0(j,j): -pi dosial of the merged LDOS stage, to 1e-13 of the largest value."""
    r = block_run(name)
    z, g = r["z"], load_golden(base_case(name))
    rec = Recursion(*objects_from(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"]), device=0)
    rec.recur_b()
    unit = np.zeros((18, 18, 18), np.complex128)
    unit[np.arange(18), np.arange(18), np.arange(18)] = 1.0
    spec = Green(rec, z["ene"], sym_term=bool(z["sym_term"])).block_spectra(unit)
    rec.close()
    ref = -np.pi * r["ldos"]["dosial"].transpose(1, 2, 0)              # (18, nen, nsites)
    err, scale = np.abs(spec - ref).max(), np.abs(ref).max()
    print("%s: |spec - (-pi dosial)| %.3e of %.3e" % (name, err, scale))
    assert err <= 1e-13 * scale


def test_block_spectra_shapes():
    """nen = 1 and nen = GREEN_WAVES + 1 (a second workgroup with one live wave), nop = 1, 21 and 32, a non-zero eta: against numpy traces of
    rsrec_block_green's g0; fewer operators or energies give the same bits for those they share."""
    name = "bccFe_nsp4_block"
    z, g = load_green(name), load_golden(name)
    rec = Recursion(*objects_from(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"]), device=0)
    rec.recur_b()
    n = int(z["nrec"])
    ene = np.ascontiguousarray(z["ene"][30:30 + GREEN_WAVES + 1])
    gr, gr1 = Green(rec, ene), Green(rec, ene[:1])
    o32 = ops32()
    eta = 2e-3j
    s32, s21, s1 = gr.block_spectra(o32), gr.block_spectra(OPS21), gr.block_spectra(o32[:1])
    e1 = gr1.block_spectra(o32)
    s_eta = gr.block_spectra(OPS21, eta=eta)
    ldos = gr.block_ldos()
    rec.zsqr()
    g0 = gr.block_green(ldos["a_inf"], ldos["b_inf"], nsites=n).copy()
    g0_eta = gr.block_green(ldos["a_inf"], ldos["b_inf"], eta=eta, nsites=n).copy()
    rec.close()
    assert s32.shape == (32, GREEN_WAVES + 1, n) and s1.shape == (1, GREEN_WAVES + 1, n) and e1.shape == (32, 1, n)
    check(s32, o32, g0, None, "nop 32, nen %d" % len(ene))
    assert np.array_equal(s21, s32[:21]) and np.array_equal(s1, s32[:1]) and np.array_equal(e1, s32[:, :1])
    check(s_eta, OPS21, g0_eta, None, "eta")
    assert np.abs(s_eta - s21).max() > 1e-6 * np.abs(s21).max()        # eta is not ignored


def test_block_spectra_image_is_zero_padded():
    """site_offset = 2 of 5 sites: untouched columns are exactly zero, the rank's columns carry the bits of the offset-0 call."""
    name = "fccCu001_block_hoh"                                          # two sites
    z, g = load_green(name), load_golden(name)
    rec = Recursion(*objects_from(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"]), device=0)
    rec.recur_b()
    gr = Green(rec, z["ene"])
    n, ntot, off = 2, 5, 2
    img = gr.block_spectra(OPS21, site_offset=off, nsites_total=ntot)
    local = gr.block_spectra(OPS21)
    with pytest.raises(_lib.RsrecError):                                 # image too small for the rank's sites
        gr.block_spectra(OPS21, site_offset=1, nsites_total=n)
    rec.close()
    assert img.shape == (21, len(z["ene"]), ntot) and np.abs(local).max() > 0
    assert np.array_equal(img[:, :, off:off + n], local)
    mask = np.ones(ntot, bool); mask[off:off + n] = False
    assert np.all(img[:, :, mask] == 0)
    assert np.array_equal(local, block_run(name)["spec"])               # ... and of another handle's call


_cheb = {}


def cheb_run(name):
    if name not in _cheb:
        z, g = load_green(name), load_golden(name)
        rec = make_rec(g)
        rec.chebyshev_recur()
        n = int(z["nrec"])
        gr = Green(rec, z["ene"])
        spec = gr.chebyshev_spectra(OPS21)
        again = gr.chebyshev_spectra(OPS21)
        s32 = gr.chebyshev_spectra(ops32())
        ldos = gr.chebyshev_ldos()
        g0 = gr.chebyshev_green(nsites=n).copy()
        rec.close()
        _cheb[name] = dict(z=z, spec=spec, again=again, s32=s32, ldos=ldos, g0=g0)
    return _cheb[name]


@pytest.mark.parametrize("name", CHEB_CASES)
def test_chebyshev_spectra(name):
    """chebyshev_recur, then ONE call, against both checkers; repeatable bit for bit; 32 operators; the diagonal unit operators would
    give the LDOS stage's numbers (checked through P0: the sum of its three rows is -pi dosia)."""
    r = cheb_run(name)
    check(r["spec"], OPS21, r["g0"], r["z"]["g0"], name)
    assert np.array_equal(r["spec"], r["again"])
    check(r["s32"], ops32(), r["g0"], None, name + " nop 32")
    assert np.array_equal(r["s32"][:21], r["spec"])
    p0 = r["spec"][:3].sum(axis=0)                                        # (nen, nsites)
    ref = -np.pi * r["ldos"]["dosia"].T
    assert np.abs(p0 - ref).max() <= 1e-12 * np.abs(ref).max()


def test_chebyshev_spectra_shapes_and_image():
    """nen = 1, nen = 65 (a second workgroup of the energy sum with one live thread), nop = 1; site_offset = 2 of 5."""
    name = "fccCu001_cheb"                                               # two sites
    r = cheb_run(name)
    z, g = r["z"], load_golden(name)
    rec = make_rec(g)
    rec.chebyshev_recur()
    n, ntot, off = 2, 5, 2
    gr = Green(rec, z["ene"])
    img = gr.chebyshev_spectra(OPS21, site_offset=off, nsites_total=ntot)
    one_op = gr.chebyshev_spectra(OPS21[:1])
    one_e = Green(rec, z["ene"][7:8]).chebyshev_spectra(OPS21)
    ene65 = np.linspace(z["ene"][5], z["ene"][-5], 65)
    s65 = Green(rec, ene65).chebyshev_spectra(OPS21)
    g65 = Green(rec, ene65).chebyshev_green(nsites=n).copy()
    with pytest.raises(_lib.RsrecError):
        gr.chebyshev_spectra(OPS21, site_offset=1, nsites_total=n)
    rec.close()
    assert np.array_equal(img[:, :, off:off + n], r["spec"])
    mask = np.ones(ntot, bool); mask[off:off + n] = False
    assert np.all(img[:, :, mask] == 0)
    assert np.array_equal(one_op, r["spec"][:1]) and np.array_equal(one_e, r["spec"][:, 7:8])
    check(s65, OPS21, g65, None, "nen 65")


def test_spectra_errors_launch_nothing():
    """No resident chains, the wrong kind of chains, nop = 0 and nop = 33: RsrecError before anything is queued (the timing of the last
    call, which every call that launches resets, stays what it was)."""
    name = "fccCu001_cheb"
    z, g = load_green(name), load_golden(name)
    rec = make_rec(g)
    gr = Green(rec, z["ene"])
    with pytest.raises(_lib.RsrecError, match="no block-Lanczos coefficients resident"):
        gr.block_spectra(OPS21)
    with pytest.raises(_lib.RsrecError, match="no Chebyshev moments resident"):
        gr.chebyshev_spectra(OPS21)
    rec.chebyshev_recur()
    t0 = rec.timing()
    assert t0["total_ms"] > 0
    with pytest.raises(_lib.RsrecError, match="no block-Lanczos coefficients resident"):
        gr.block_spectra(OPS21)
    for bad in (np.zeros((0, 18, 18), complex), np.zeros((33, 18, 18), complex)):
        with pytest.raises(_lib.RsrecError, match="nop"):
            gr.chebyshev_spectra(bad)
    assert rec.timing() == t0
    rec.recur_b()
    t1 = rec.timing()
    with pytest.raises(_lib.RsrecError, match="no Chebyshev moments resident"):
        gr.chebyshev_spectra(OPS21)
    for bad in (np.zeros((0, 18, 18), complex), np.zeros((33, 18, 18), complex)):
        with pytest.raises(_lib.RsrecError, match="nop"):
            gr.block_spectra(bad)
    assert rec.timing() == t1
    rec.close()


DEVICE_OUTPUT_SCRIPT = r"""
import sys, numpy as np, torch
torch.cuda.init(); torch.cuda.set_device(0)          # torch's HIP runtime first, as in bench.py
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import load_golden, objects_from, problem_dict
from test_gpu_green import load_green
from rslmtoasa_amd import bands
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.recursion import Recursion
ops = bands.stack(bands.ALL_OPERATORS)
t_ops = torch.from_numpy(np.ascontiguousarray(ops.transpose(0, 2, 1))).cuda()       # [k][column][row]
n, ntot, off = 2, 5, 2
for name, recur, call in (("fccCu001_block_hoh", "recur_b", "block_spectra"), ("fccCu001_cheb", "chebyshev_recur", "chebyshev_spectra")):
    z, g = load_green(name), load_golden(name)
    rec = Recursion(*objects_from(problem_dict(g), g["irec"], g["lld"], nsp=g["nsp"], emin=g["emin"], emax=g["emax"]), device=0)
    getattr(rec, recur)()
    gr = Green(rec, z["ene"])
    nen = len(z["ene"])
    host = getattr(gr, call)(ops, site_offset=off, nsites_total=ntot)
    t = torch.full((ntot, nen, len(ops)), -1.0, dtype=torch.float64, device="cuda")  # Fortran (nop, nen, ntot)
    torch.cuda.synchronize()
    assert getattr(gr, call)(ops, site_offset=off, nsites_total=ntot, out=t.data_ptr()) is None
    assert np.abs(host).max() > 0 and np.array_equal(t.cpu().numpy().transpose(2, 1, 0), host)
    t.fill_(-1.0); torch.cuda.synchronize()
    getattr(gr, call)(t_ops, site_offset=off, nsites_total=ntot, out=t.data_ptr())   # operators read from device memory
    assert np.array_equal(t.cpu().numpy().transpose(2, 1, 0), host)
    rec.close()
print("DEVICE_OUTPUT_OK")
"""


def test_spectra_device_outputs_match_host_outputs():
    """A device tensor handed over as ``out`` (what a collective would reduce) receives the bits of the host image, zeros included; the
    operators may lie in device memory as well.  Own process: torch's HIP runtime has to be initialised before librsrec's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", DEVICE_OUTPUT_SCRIPT, root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE_OUTPUT_OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
