#!/usr/bin/env python3
"""Wall time of the Gilbert-damping traces (exchange%calculate_gilbert_damping, exchange.f90:674-694) behind the block pair recursion:
bcc Fe 22^3 cell, 64 atom pairs (256 chains), LL = 20, the reference's 2510-point mesh.

  --route damping  Exchange.damping(): one rsrec_damping call on the chains the pair recursion left on the device.  Also reports the
                   kernel-stage time (rsrec_get_timing out[5]) of rsrec_damping and of rsrec_exchange on the same chains: their Green
                   stage is the same, so the difference is the cost of the damping epilogue over the exchange epilogue + integration.
  --route g0       the only route without rsrec_damping: terminators and rsrec_block_green of the 4 x 64 chains into host memory
                   (g0(18,18,nE,256), 3.3 GB), then the traces in numpy (batched over the energies).  Uses nothing newer than
                   rsrec_block_green, so it runs unchanged in a checkout of an older commit.

Wall time around the call, `--warmup` calls first, median of `--reps`; one JSON line.

    python tools/time_damping.py --route damping --reps 5 --warmup 2
    python tools/time_damping.py --route g0 --reps 5 --warmup 2
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def traces_numpy(g0, tmat):
    """(18, nE, npairs) rows from g0 (18,18,nE,4*npairs) of i /= j pairs: green.f90:450-453, then exchange.f90:676-688, batched over nE."""
    import numpy as np
    npairs = g0.shape[3] // 4
    rows = np.zeros((18, g0.shape[2], npairs))
    for q in range(npairs):
        g = np.moveaxis(g0[..., 4 * q:4 * q + 4], 2, 0)
        d = g[..., 0] - g[..., 1]
        s = 1.0 / 1j * g[..., 2] - 1.0 / 1j * g[..., 3]
        gij, gji = (d + s) * 0.5, (d - s) * 0.5
        Aij = gij - np.conj(gji).transpose(0, 2, 1)
        Aji = gji - np.conj(gij).transpose(0, 2, 1)
        X = [np.matmul(tmat[:, :, k, 0, q], Aij) for k in range(3)]
        Y = [np.matmul(np.conj(tmat[:, :, l, 1, q]).T, Aji) for l in range(3)]
        for k in range(3):
            for l in range(3):
                t = np.einsum("eab,eba->e", X[k], Y[l])
                rows[3 * k + l, :, q], rows[9 + 3 * k + l, :, q] = t.real, t.imag
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--route", choices=("damping", "g0"), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=22)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--lld", type=int, default=20)
    args = ap.parse_args()

    import numpy as np
    import bench
    from rslmtoasa_amd import _lib
    from rslmtoasa_amd.exchange import Exchange
    from rslmtoasa_amd.green import Green
    from rslmtoasa_amd.lattice import bcc_supercell, spread_sites, supercell_positions
    from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion

    st = bench.load_stencil(False)
    n = args.cells
    nn = bcc_supercell((n, n, n), st["slot_vec"])
    kk = nn.shape[0]
    first = spread_sites(kk, args.pairs)
    pairs = np.stack([first, nn[first - 1, 1 + np.arange(args.pairs) % 14]], axis=1).astype(np.int32)      # every pair a neighbour pair, i /= j
    lat = Lattice(nn=nn, iz=np.ones(kk, np.int32), irec=first, nmax=0, ntype=1, cr=supercell_positions((n, n, n)))
    lat.ijpair = pairs
    ham = Hamiltonian(ee=st["ee"], lsham=st["lsham"], eeo=None, enim=None, hall=None, hallo=None, hoh=False)
    rec = Recursion(ham, lat, Control(lld=args.lld, nsp=2, recur="block"), Energy(energy_min=-3.0, energy_max=1.8), device=0)
    gz = np.load(os.path.join(ROOT, "tests", "golden", "bccFe_nsp2_block_green.npz"), allow_pickle=False)
    ene = float(gz["ene_full_first"]) + float(gz["ene_full_step"]) * np.arange(int(gz["nen_full"]))     # bench.py's mesh of the ldos leg
    gr = Green(rec, ene)
    t0 = time.perf_counter()
    rec.recur_b_ij()
    t_rec = time.perf_counter() - t0
    rng = np.random.default_rng(1)
    tmat = np.asfortranarray(rng.standard_normal((18, 18, 3, 2, args.pairs)) + 1j * rng.standard_normal((18, 18, 3, 2, args.pairs)))
    ief = len(ene) // 2
    x = Exchange(rec, gr)
    extra = {}

    if args.route == "damping":
        def call():
            return x.damping(tmat, ief, resident=True)[1]
    else:
        rec.zsqr()                                                            # (once, outside the timed call; rsrec_damping roots inside it)

        def call():
            a_inf, b_inf, _, _ = gr.terminator(nsites=4 * args.pairs)
            g0 = gr.block_green(a_inf, b_inf, nsites=4 * args.pairs)
            rows = traces_numpy(g0, tmat)
            return rows[:9].sum(axis=2)

    times, device_ms, kernel_ms = [], [], []
    for k in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        out = call()
        t = time.perf_counter() - t0
        if k >= args.warmup:
            tm = rec.timing()
            times.append(t * 1e3); device_ms.append(tm["total_ms"]); kernel_ms.append(tm["rest_ms"] if args.route == "damping" else tm["hop_ms"])
    assert np.isfinite(out).all() and out.shape == (9, len(ene))
    if args.route == "damping":
        dpar = np.zeros((4, 3, 2, args.pairs), order="F")
        dpar[:2], dpar[2:] = 0.1, 0.2
        kx = []
        for k in range(args.warmup + args.reps):
            x.compute(float(ene[ief]), 2 * ((len(ene) - 10) // 2) + 1, dpar, resident=True)
            if k >= args.warmup:
                kx.append(rec.timing()["rest_ms"])
        extra = {"exchange_kernel_ms_median": statistics.median(kx), "exchange_kernel_ms": kx,
                 "damping_minus_exchange_kernel_ms": statistics.median(kernel_ms) - statistics.median(kx)}
    rec.close()
    print(json.dumps({"route": args.route, "library": _lib.LIB_PATH, "cells": n, "pairs": args.pairs, "lld": args.lld, "energies": len(ene),
                      "warmup": args.warmup, "reps": args.reps, "wall_ms_median": statistics.median(times), "wall_ms": times,
                      "device_ms_median": statistics.median(device_ms), "kernel_ms_median": statistics.median(kernel_ms), "kernel_ms": kernel_ms,
                      "recursion_wall_s": t_rec, "checksum": float(np.abs(out).sum()), **extra}))


if __name__ == "__main__":
    main()
