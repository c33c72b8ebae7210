"""Time of the Gauss-Legendre contour calls (kernels_contour.hpp) and, in the same run, of the path they replace.

    python tools/time_contour.py [--lld 20] [--npts 64] [--pairs 1 64 1024] [--sites 64] [--dims 22 22 22] [--reps 5] [--loop-pairs 4]

New path: one rsrec_exchange_contour call for all pairs from host coefficients (what the drop-in's arrays are), and one
rsrec_contour_occupation call for the on-site chains.  Replaced path, as the inherited routines drive the library: per pair and per point
one rsrec_terminator call on the pair's four chains (green.f90:341 sits inside the point loop) and four single-energy rsrec_block_green
calls, each uploading its chain's coefficients; for the occupations per point one terminator call on all sites and one block_green call per
site.  The replaced path is run on --loop-pairs pairs (it is linear in the pairs: every call is independent) and scaled to the pair count.

Both paths are timed as wall time around the calls after a warm-up call (the replaced path is dominated by call overhead and transfers,
which device events do not see); the new calls' device time from rsrec_get_timing is printed beside it.  One JSON line per row, medians
of --reps runs."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def old_path(rec, a_b, b_s, e0, eta, groups, sym_term=0):
    """The replaced sequence for `groups` groups of chains (a pair's four, or one site's one): per point a terminator call on the group,
    then one single-energy block_green call per chain."""
    L, h = rec._L, rec._h
    lld = a_b.shape[2]
    ene = np.array([e0])
    g0 = np.zeros((18, 18, 1, 1), np.complex128, order="F")
    for c0, nc in groups:
        ab = [np.asfortranarray(a_b[..., c0 + i:c0 + i + 1]) for i in range(nc)]
        bs = [np.asfortranarray(b_s[..., c0 + i:c0 + i + 1]) for i in range(nc)]
        abg, bsg = np.asfortranarray(a_b[..., c0:c0 + nc]), np.asfortranarray(b_s[..., c0:c0 + nc])
        a_inf, b_inf = np.zeros((18, 18, nc), order="F"), np.zeros((18, 18, nc), order="F")
        a0, b0 = np.zeros(nc), np.zeros(nc)
        for et in eta:
            rec._check(L.rsrec_terminator(h, nc, lld, P(abg), P(bsg), P(a_inf), P(b_inf), P(a0), P(b0)))
            for i in range(nc):
                ai, bi = np.asfortranarray(a_inf[..., i:i + 1]), np.asfortranarray(b_inf[..., i:i + 1])
                rec._check(L.rsrec_block_green(h, 1, lld, 1, P(ene), 0.0, float(et), sym_term, P(ai), P(bi), P(ab[i]), P(bs[i]), P(g0)))


def timed(fn, reps):
    fn()                                               # warm-up: buffers, code objects
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    import pair_cases as X
    from contour_reference import contour_eta
    from rslmtoasa_amd.exchange import Exchange, gauss_legendre
    ap = argparse.ArgumentParser()
    ap.add_argument("--lld", type=int, default=20)
    ap.add_argument("--npts", type=int, default=64)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--dims", type=int, nargs=3, default=[22, 22, 22])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-pairs", type=int, default=4)
    args = ap.parse_args()
    x, w = gauss_legendre(args.npts)
    eta = contour_eta(x)
    base = np.array([(1, 2), (1, 9), (3, 17), (5, 60)], np.int32)
    rec, g, ene, nv1, dpar = X.setup(base, lld=args.lld, dims=tuple(args.dims), channels=100)
    rec.zsqr()
    e0 = float(ene[50])
    ex = Exchange(rec, g)
    a16, b16 = rec.a_b[..., :16].copy(), rec.b2_b[..., :16].copy()
    lp = max(1, min(args.loop_pairs, 4))
    old_ms = timed(lambda: old_path(rec, a16, b16, e0, eta, [(4 * q, 4) for q in range(lp)]), max(1, args.reps // 2)) / lp
    for n in args.pairs:
        reps = (n + 3) // 4
        a_h = np.asfortranarray(np.tile(a16, (1, 1, 1, reps))[..., :4 * n])
        b_h = np.asfortranarray(np.tile(b16, (1, 1, 1, reps))[..., :4 * n])
        rec.lattice.ijpair = np.tile(base, (reps, 1))[:n]
        dmat = X.random_contour_dmat(n)
        dev = []

        def new():
            ex.contour(x, w, e0, dmat, coef=(a_h, b_h))
            dev.append(ex.timing()[0])
        new_ms = timed(new, args.reps)
        print(json.dumps(dict(stage="exchange_contour", lld=args.lld, npts=args.npts, pairs=n, new_wall_ms=new_ms, new_device_ms=float(np.median(dev[1:])),
                              replaced_wall_ms=old_ms * n, replaced_measured_on_pairs=lp, ratio=old_ms * n / new_ms)), flush=True)
    # occupations: --sites on-site chains (the pair chains serve: a chain is a chain to both paths)
    ns = args.sites
    reps = (ns + 15) // 16
    a_s = np.asfortranarray(np.tile(a16, (1, 1, 1, reps))[..., :ns])
    b_s = np.asfortranarray(np.tile(b16, (1, 1, 1, reps))[..., :ns])
    occ = np.zeros((18, ns), order="F")
    dev = []

    def new_occ():
        rec._check(rec._L.rsrec_contour_occupation(rec._h, 0, ns, args.lld, args.npts, P(x), P(w), e0, 0, -3.0, 1.8, None, None, P(a_s), P(b_s), 0, ns, P(occ), None))
        dev.append(rec.timing()["total_ms"])
    new_ms = timed(new_occ, args.reps)
    ls = min(ns, 8)
    old_occ = timed(lambda: old_path(rec, a_s, b_s, e0, eta, [(0, ls)]), max(1, args.reps // 2)) / ls * ns
    print(json.dumps(dict(stage="contour_occupation", lld=args.lld, npts=args.npts, sites=ns, new_wall_ms=new_ms, new_device_ms=float(np.median(dev[1:])),
                          replaced_wall_ms=old_occ, replaced_measured_on_sites=ls, ratio=old_occ / new_ms)), flush=True)
    rec.close()


if __name__ == "__main__":
    main()
