"""What the Kubo moment tests (tests/test_gpu_kubo_diag.py, _multi.py, _tensor.py) share: a handle with the operators, scaling and random
vectors of one problem (Case), the golden and the ragged case, the calls of the four library entry points on a case, and the ragged
lattice with further seeded operators (Ragged) whose single-call moments are computed once.  Not a test module."""
import ctypes as C

import numpy as np
import pytest

from helpers import load_golden, objects_from, random_vec_coefficients
from rslmtoasa_amd.recursion import Recursion
from test_gpu_spmm_random import random_problem

DIAG = np.arange(18)


def ptr(a):
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def fcc(a):
    return None if a is None else np.asfortranarray(a, dtype=np.complex128)


def vec_err(mu, ref):
    return max(np.abs(mu[..., i] - ref[..., i]).max() / np.abs(ref[..., i]).max() for i in range(ref.shape[-1]))


def same_bits(a, b):
    return np.array_equal(np.ravel(a, order="K").view(np.float64), np.ravel(b, order="K").view(np.float64))


class Case:
    """A handle with the operators, scaling and random vectors of one problem; the moment calls go straight to the library."""

    def __init__(self, p, a, b, v_a, v_b, vo_a, vo_b, seeds, coefs, irec=(1,)):
        self.rec = Recursion(*objects_from(p, np.asarray(irec, np.int32), 4, nsp=int(p.get("nsp", 2))), device=0)
        self.a, self.b = float(a), float(b)
        self.ops = [fcc(v_a), fcc(vo_a), fcc(v_b), fcc(vo_b)]
        self.seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        self.coefs = np.ascontiguousarray(coefs, dtype=np.complex128)

    def call(self, name, cond_ll, out, vecs=None):
        """rsrec_kubo_moments / rsrec_kubo_moments_diag on vectors `vecs` (default: all) into `out` (numpy, torch, or None)."""
        rec = self.rec
        sel = slice(None) if vecs is None else vecs
        seeds, coefs = np.ascontiguousarray(self.seeds[sel]), np.ascontiguousarray(self.coefs[sel])
        nvec, nseed = seeds.shape
        fn = getattr(rec._L, name)
        return fn(rec._h, nvec, nseed, ptr(seeds), ptr(coefs), int(cond_ll), self.a, self.b, *[ptr(o) for o in self.ops], ptr(out))

    def full(self, cond_ll, vecs=None):
        nvec = len(self.seeds[slice(None) if vecs is None else vecs])
        mu = np.zeros((18, 18, cond_ll, cond_ll, nvec), np.complex128, order="F")
        self.rec._check(self.call("rsrec_kubo_moments", cond_ll, mu, vecs))
        return mu

    def diag(self, cond_ll, vecs=None):
        nvec = len(self.seeds[slice(None) if vecs is None else vecs])
        mu = np.zeros((18, cond_ll, cond_ll, nvec), np.complex128, order="F")
        self.rec._check(self.call("rsrec_kubo_moments_diag", cond_ll, mu, vecs))
        return mu

    def last_error(self):
        buf = C.create_string_buffer(512)
        self.rec._L.rsrec_last_error(self.rec._h, buf, 512)
        return buf.value


def golden_case(name):
    z = load_golden(name)
    p = {k: z[k] for k in ("nn", "iz", "ee", "lsham", "eeo", "enim") if k in z}
    p.update(nmax=0, hoh=int(z["hoh"]), nsp=int(z["nsp"]))
    if "rng" in z:
        seeds, coefs = random_vec_coefficients(z["rng"])
    else:
        seeds = np.asarray(z["atlist"], np.int32).reshape(-1, 1)
        coefs = np.ones(seeds.shape, np.complex128)
    return z, Case(p, z["acheb"], z["bcheb"], z["v_a"], z["v_b"], z.get("vo_a"), z.get("vo_b"), seeds, coefs, irec=z["atlist"])


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's (as bench.py does)
    torch.cuda.set_device(0)


KK_ODD = 75            # 18 kk = 1350 = 2 mod 4: the last k-step of the contraction ends in the zero block


def ragged_case(hoh):
    """Random ragged lattice with an ODD number of atoms, random velocity blocks, three random-phase vectors.  a bounds the operator
    norm (5 slots of 18 x 18 complex Gaussian blocks of deviation 0.28 each: < 15) with room, so the recurrences stay tame."""
    rng = np.random.default_rng(4242 + int(hoh))
    p = random_problem(rng, KK_ODD, 5, 2, 0, hoh, False)
    if hoh:                                                # (h - h o h: keep the second-order part small against a)
        p["eeo"] = np.asfortranarray(p["eeo"] * 0.1)

    def vel():
        return np.asfortranarray((rng.standard_normal((18, 18, 5, 2)) + 1j * rng.standard_normal((18, 18, 5, 2))) * 0.2)
    v_a, v_b = vel(), vel()
    vo_a, vo_b = (vel(), vel()) if hoh else (None, None)
    nvec = 3
    seeds = np.tile(np.arange(1, KK_ODD + 1, dtype=np.int32), (nvec, 1))
    coefs = np.exp(2j * np.pi * rng.random((nvec, KK_ODD))) / np.sqrt(KK_ODD)
    return Case(p, 60.0, 0.1, v_a, v_b, vo_a, vo_b, seeds, coefs)


def integrand_call(c, name, nvec, L, mu, z):
    ene = np.ascontiguousarray(z["ene"], np.float64)
    out = np.zeros((18, ene.size, nvec), np.complex128, order="F")
    rc = getattr(c.rec._L, name)(c.rec._h, nvec, L, ptr(mu), ene.size, ptr(ene), float(z["energy_min"]), float(z["energy_max"]), ptr(out))
    return rc, out


def stack(ops):
    """output operators (18, 18, nslots, ntype) -> (18, 18, nslots, ntype, nout), Fortran order; None if there are none (no hoh)"""
    return None if ops[0] is None else np.asfortranarray(np.stack(ops, axis=-1), dtype=np.complex128)


def multi_call(c, outs, cond_ll, out, vecs=None, nout=None, v_b="case", vo_b="case"):
    """rsrec_kubo_moments_diag_multi on the case's vectors with output operators outs = [(v, vo), ...]; returns the return code"""
    rec = c.rec
    sel = slice(None) if vecs is None else vecs
    seeds, coefs = np.ascontiguousarray(c.seeds[sel]), np.ascontiguousarray(c.coefs[sel])
    nvec, nseed = seeds.shape
    v_out = stack([o[0] for o in outs]) if outs else None
    vo_out = stack([o[1] for o in outs]) if outs else None
    vb = c.ops[2] if isinstance(v_b, str) else v_b
    vob = c.ops[3] if isinstance(vo_b, str) else vo_b
    return rec._L.rsrec_kubo_moments_diag_multi(rec._h, len(outs) if nout is None else nout, nvec, nseed, ptr(seeds), ptr(coefs), int(cond_ll), c.a, c.b,
                               ptr(v_out), ptr(vo_out), ptr(vb), ptr(vob), ptr(out))


def multi(c, outs, cond_ll, vecs=None):
    nvec = len(c.seeds[slice(None) if vecs is None else vecs])
    mu = np.zeros((18, cond_ll, cond_ll, nvec, len(outs)), np.complex128, order="F")
    c.rec._check(multi_call(c, outs, cond_ll, mu, vecs))
    return mu


def tensor_call(c, outs, ins, cond_ll, out, vecs=None, nin=None, nout=None):
    """rsrec_kubo_moments_diag_tensor on the case's vectors with operators outs, ins = [(v, vo), ...]; returns the return code"""
    rec = c.rec
    sel = slice(None) if vecs is None else vecs
    seeds, coefs = np.ascontiguousarray(c.seeds[sel]), np.ascontiguousarray(c.coefs[sel])
    nvec, nseed = seeds.shape
    v_out, vo_out = (stack([o[0] for o in outs]), stack([o[1] for o in outs])) if outs else (None, None)
    v_in, vo_in = (stack([o[0] for o in ins]), stack([o[1] for o in ins])) if ins else (None, None)
    return rec._L.rsrec_kubo_moments_diag_tensor(rec._h, len(ins) if nin is None else nin, len(outs) if nout is None else nout, nvec, nseed, ptr(seeds), ptr(coefs),
                               int(cond_ll), c.a, c.b, ptr(v_out), ptr(vo_out), ptr(v_in), ptr(vo_in), ptr(out))


def tensor(c, outs, ins, cond_ll, vecs=None):
    nvec = len(c.seeds[slice(None) if vecs is None else vecs])
    mu = np.zeros((18, cond_ll, cond_ll, nvec, len(outs), len(ins)), np.complex128, order="F")
    c.rec._check(tensor_call(c, outs, ins, cond_ll, mu, vecs))
    return mu


def single(c, out_op, in_op=None, cond_ll=None, vecs=None):
    """rsrec_kubo_moments_diag with (v_a, vo_a) = out_op and (v_b, vo_b) = in_op (default: the case's v_b)"""
    keep = c.ops
    c.ops = [out_op[0], out_op[1]] + (keep[2:] if in_op is None else [in_op[0], in_op[1]])
    try:
        return c.diag(cond_ll, vecs)
    finally:
        c.ops = keep


class Ragged:
    """The ragged lattice with three output operators: the case's v_a, its v_b used as an output operator, one more random operator
    seeded by `seed`.  Inputs: the case's v_b, or with_inputs its v_b, its v_a and one more random operator, so that no two of the nine
    sets are the same pair."""

    def __init__(self, hoh, seed, with_inputs):
        self.hoh = hoh
        self.c = c = ragged_case(hoh)
        rng = np.random.default_rng(seed + int(hoh))

        def vel():
            return np.asfortranarray((rng.standard_normal((18, 18, 5, 2)) + 1j * rng.standard_normal((18, 18, 5, 2))) * 0.2)

        def op():
            return (vel(), vel() if hoh else None)
        self.outs = [(c.ops[0], c.ops[1]), (c.ops[2], c.ops[3]), op()]
        self.ins = [(c.ops[2], c.ops[3])] + ([(c.ops[0], c.ops[1]), op()] if with_inputs else [])
        self.cache = {}

    def single(self, j, i, cond_ll, lchunk=0):
        """the single call's moments of the pair (out j, in i), computed once per (j, i, cond_ll, kubo_lchunk) and left unchanged"""
        key = (j, i, cond_ll, lchunk)
        if key not in self.cache:
            self.c.rec.set_option("kubo_lchunk", lchunk)
            try:
                mu = single(self.c, self.outs[j], self.ins[i], cond_ll)
            finally:
                self.c.rec.set_option("kubo_lchunk", 0)
            mu.setflags(write=False)
            self.cache[key] = mu
        return self.cache[key]


def ragged_pair(seed, with_inputs):
    """the body of a module's `ragged` fixture: a Ragged without and with hoh, closed at the end"""
    cases = {hoh: Ragged(hoh, seed, with_inputs) for hoh in (False, True)}
    yield cases
    for r in cases.values():
        r.c.rec.close()
